/*
 * pestat_core_main.c -- host/pestat_core.h as a stand-alone program, for a plain build and one under AddressSanitizer:
 * bmh_ps_candidate and the drop-exact move of pestat_collect_kernel over the vector pairs of a case file, every slice in a heap
 * block of exactly its size, so that a read or a write one record past a slice is an error the sanitizer reports.
 *
 *   pestat_core_main FILE
 *
 * FILE (little endian, written by tests/test_pestat_cand_cpu.py):
 *   int32 magic 0x50455354, int32 drop_exact, int32 match, int32 n_reads, int64 l_pac, bmh_sam_opt_t (96 bytes)
 *   int32 l_seq[n_reads], int32 count[n_reads], then the regions of all reads, 64 bytes each
 * Prints one line:  pairs P nonzero Z removed R digest D   (D: sum of (word + 0x9E3779B97F4A7C15) * (2 i + 1) modulo 2^64)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/pestat_core.h"

static int fail(const char *why)
{
	fprintf(stderr, "pestat_core_main: %s\n", why);
	return 2;
}

/* the move as the kernel makes it: record by record, ascending, inside the slice; returns the count it leaves */
static size_t drop_exact(bmh_alnreg_t *a, size_t n, int l_seq, int match, long *removed)
{
	size_t k;
	if (!bmh_ps_is_exact(a, n, l_seq, match)) return n;
	for (k = 0; k + 1 < n; ++k) a[k] = a[k + 1];
	++*removed;
	return n - 1;
}

int main(int argc, char **argv)
{
	int32_t head[4], *len = 0, *cnt = 0;
	int64_t l_pac;
	bmh_sam_opt_t o;
	FILE *f;
	long removed = 0, nonzero = 0;
	uint64_t digest = 0;
	int r, n, np, p;
	if (argc != 2) return fail("usage: pestat_core_main FILE");
	if (sizeof(o) != 96 || sizeof(bmh_alnreg_t) != 64) return fail("record sizes");
	if (!(f = fopen(argv[1], "rb"))) return fail("cannot open the case file");
	if (fread(head, 4, 4, f) != 4 || head[0] != 0x50455354 || fread(&l_pac, 8, 1, f) != 1 || fread(&o, sizeof(o), 1, f) != 1) return fail("bad header");
	n = head[3], np = n >> 1;
	if (n < 0) return fail("bad read count");
	len = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 1)), cnt = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 1));
	if (!len || !cnt || fread(len, 4, (size_t)n, f) != (size_t)n || fread(cnt, 4, (size_t)n, f) != (size_t)n) return fail("bad tables");
	for (p = 0; p < np; ++p) {
		bmh_alnreg_t *a[2];
		size_t m[2];
		uint32_t w;
		for (r = 0; r < 2; ++r) { /* an exact block per slice (none for an empty one: the rule must not look at it) */
			m[r] = (size_t)cnt[2 * p + r];
			a[r] = m[r] ? (bmh_alnreg_t *)malloc(m[r] * sizeof(bmh_alnreg_t)) : 0;
			if (m[r] && (!a[r] || fread(a[r], sizeof(bmh_alnreg_t), m[r], f) != m[r])) return fail("bad regions");
			if (head[1] && drop_exact(a[r], m[r], len[2 * p + r], head[2], &removed) != m[r]) { /* ... and exact again for the rule */
				bmh_alnreg_t *b = --m[r] ? (bmh_alnreg_t *)malloc(m[r] * sizeof(bmh_alnreg_t)) : 0;
				if (m[r] && !b) return fail("out of memory");
				if (m[r]) memcpy(b, a[r], m[r] * sizeof(bmh_alnreg_t));
				free(a[r]), a[r] = b;
			}
		}
		w = bmh_ps_candidate(&o, l_pac, a[0], m[0], a[1], m[1]);
		nonzero += w != 0;
		digest += ((uint64_t)w + 0x9E3779B97F4A7C15ull) * (2 * (uint64_t)p + 1);
		free(a[0]), free(a[1]);
	}
	fclose(f);
	free(len), free(cnt);
	printf("pairs %d nonzero %ld removed %ld digest %llu\n", np, nonzero, removed, (unsigned long long)digest);
	return 0;
}
