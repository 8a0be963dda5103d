/*
 * pairs_plan_core_main.c -- the paired-end clause of host/handoff_core.h as a stand-alone program, for a plain build and one under
 * AddressSanitizer: bmh_ho_pairs over a region table's offsets in table_plan_kernel's shape -- slices of SLICE reads, each folded on
 * its own, the folds merged -- with the offsets in a heap block of exactly n_reads + 1 entries, so that a look one entry past the
 * table is an error the sanitizer reports.  The slices are merged forwards, backwards and from the middle outwards: the three must
 * agree, or the program fails.
 *
 *   pairs_plan_core_main FILE SLICE
 *
 * FILE (little endian, written by tests/test_pairs_plan_core_cpu.py):
 *   int32 magic 0x50414952, int32 n_reads, int64 count[n_reads]
 * Prints one line:  reads N pairs P pair_kmax K
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/handoff_core.h"

static int fail(const char *why)
{
	fprintf(stderr, "pairs_plan_core_main: %s\n", why);
	return 2;
}

int main(int argc, char **argv)
{
	int32_t head[2];
	int64_t *cnt = 0, *part = 0, n, slice, ns, s, r, pairs = 0, fwd = BMH_HO_PAIRS_INIT, bwd = BMH_HO_PAIRS_INIT, mid = BMH_HO_PAIRS_INIT;
	uint64_t *roff = 0;
	FILE *f;
	if (argc != 3 || (slice = atoll(argv[2])) < 1) return fail("usage: pairs_plan_core_main FILE SLICE");
	if (!(f = fopen(argv[1], "rb"))) return fail("cannot open the case file");
	if (fread(head, 4, 2, f) != 2 || head[0] != 0x50414952 || head[1] < 0) return fail("bad header");
	n = head[1];
	cnt = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n ? n : 1));
	roff = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n + 1)); /* exactly the table's n + 1 offsets */
	if (!cnt || !roff || fread(cnt, 8, (size_t)n, f) != (size_t)n) return fail("bad counts");
	fclose(f);
	roff[0] = 0;
	for (r = 0; r < n; ++r) {
		if (cnt[r] < 0) return fail("a negative count");
		roff[r + 1] = roff[r] + (uint64_t)cnt[r];
		pairs += bmh_ho_first_mate(r, n);
	}
	free(cnt);
	ns = (n + slice - 1) / slice;
	part = (int64_t *)malloc(sizeof(int64_t) * (size_t)(ns ? ns : 1));
	if (!part) return fail("out of memory");
	for (s = 0; s < ns; ++s) {
		const int64_t r1 = (s + 1) * slice < n ? (s + 1) * slice : n;
		part[s] = BMH_HO_PAIRS_INIT;
		bmh_ho_pairs(roff, s * slice, r1, n, &part[s]);
	}
	for (s = 0; s < ns; ++s) bmh_ho_pairs_merge(&fwd, part[s]), bmh_ho_pairs_merge(&bwd, part[ns - 1 - s]);
	for (s = 0; s < ns; ++s) bmh_ho_pairs_merge(&mid, part[(ns / 2 + (s & 1 ? -(s + 1) / 2 : (s + 1) / 2) + ns) % ns]);
	free(part);
	free(roff);
	if (fwd != bwd || fwd != mid) return fail("the merge depends on its order");
	printf("reads %lld pairs %lld pair_kmax %lld\n", (long long)n, (long long)pairs, (long long)fwd);
	return 0;
}
