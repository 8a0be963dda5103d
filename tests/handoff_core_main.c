/*
 * handoff_core_main.c -- host/handoff_core.h as a stand-alone program, for a plain build and one under AddressSanitizer: the reduction
 * table_plan_kernel makes over a batch's regions, in its own shape -- one read at a time into the part of its group of 64, the parts
 * merged at the end -- with every read's vector in a heap block of exactly its size, so that a read one record past a vector is an
 * error the sanitizer reports.  An empty vector has no block at all: the rule must not look at it.
 *
 *   handoff_core_main FILE
 *
 * FILE (little endian, written by tests/test_handoff_core_cpu.py):
 *   int32 magic 0x48414e44, int32 n_reads, bmh_sam_opt_t (96 bytes), int32 count[n_reads], then the regions of all reads, 64 bytes each
 * Prints one line:  reads N total T kmax K opool_cap C neg F
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/handoff_core.h"

static int fail(const char *why)
{
	fprintf(stderr, "handoff_core_main: %s\n", why);
	return 2;
}

int main(int argc, char **argv)
{
	int32_t head[2], *cnt = 0;
	bmh_sam_opt_t o;
	bmh_ho_plan_t all = BMH_HO_PLAN_INIT, part = BMH_HO_PLAN_INIT;
	const bmh_ho_plan_t init = BMH_HO_PLAN_INIT;
	FILE *f;
	int r, n;
	if (argc != 2) return fail("usage: handoff_core_main FILE");
	if (sizeof(o) != 96 || sizeof(bmh_alnreg_t) != 64 || sizeof(bmh_ho_plan_t) != 32) return fail("record sizes");
	if (!(f = fopen(argv[1], "rb"))) return fail("cannot open the case file");
	if (fread(head, 4, 2, f) != 2 || head[0] != 0x48414e44 || fread(&o, sizeof(o), 1, f) != 1) return fail("bad header");
	n = head[1];
	if (n < 0) return fail("bad read count");
	cnt = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 1));
	if (!cnt || fread(cnt, 4, (size_t)n, f) != (size_t)n) return fail("bad counts");
	for (r = 0; r < n; ++r) {
		const size_t m = (size_t)cnt[r];
		bmh_alnreg_t *a = m ? (bmh_alnreg_t *)malloc(m * sizeof(bmh_alnreg_t)) : 0;
		if (cnt[r] < 0 || (m && (!a || fread(a, sizeof(bmh_alnreg_t), m, f) != m))) return fail("bad regions");
		bmh_ho_read(&o, a, (int64_t)m, &part);
		free(a);
		if ((r & 63) == 63 || r == n - 1) bmh_ho_merge(&all, &part), part = init;
	}
	fclose(f);
	free(cnt);
	printf("reads %d total %lld kmax %lld opool_cap %lld neg %d\n", n, (long long)all.total, (long long)all.kmax, (long long)all.opool_cap, (int)all.neg);
	return 0;
}
