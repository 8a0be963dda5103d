/*
 * sort_paths_main.c -- stand-alone check of bmh_dedup_core (host/dedup_core.h over host/sort_exact.h) for a sanitizer build:
 * tests/test_sort_paths_cpu.py compiles it with gcc -fsanitize=address,undefined and runs it as a child process.
 *
 * Input file (little endian, written by the test from tests/golden/sort_paths_golden.npz):
 *   int32 n_cases
 *   per case:   int32 n, int32 n_levels, n records of sizeof(bmh_alnreg_t)
 *     per level: float mask_level_redun, int32 m, m x int32 index of the expected survivors into the case's records, in order
 * Every run gets its records in a heap block of exactly n records and its range stack in a heap block of exactly
 * bmh_sort_stack_len(n) entries, so an access past either is the sanitizer's to report.  Exit status 0: every run reproduced
 * its expected survivors byte for byte.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/dedup_core.h"

static int rd(void *p, size_t sz, size_t n, FILE *f) { return fread(p, sz, n, f) == n; }

int main(int argc, char **argv)
{
	FILE *f;
	int32_t n_cases, c, runs = 0, bad = 0;
	if (argc != 2 || !(f = fopen(argv[1], "rb"))) {
		fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
		return 2;
	}
	if (!rd(&n_cases, 4, 1, f)) return 2;
	for (c = 0; c < n_cases; ++c) {
		int32_t n, n_levels, l;
		bmh_alnreg_t *in;
		if (!rd(&n, 4, 1, f) || !rd(&n_levels, 4, 1, f) || n < 0) return 2;
		in = (bmh_alnreg_t *)malloc(sizeof(*in) * (size_t)n);
		if (n && (!in || !rd(in, sizeof(*in), (size_t)n, f))) return 2;
		for (l = 0; l < n_levels; ++l) {
			float level;
			int32_t m, k, got, *want;
			bmh_alnreg_t *a;
			bmh_sort_stk_t *stk;
			if (!rd(&level, 4, 1, f) || !rd(&m, 4, 1, f) || m < 0 || m > n) return 2;
			want = (int32_t *)malloc(sizeof(*want) * (size_t)m);
			if (m && (!want || !rd(want, 4, (size_t)m, f))) return 2;
			a = (bmh_alnreg_t *)malloc(sizeof(*a) * (size_t)n);
			stk = (bmh_sort_stk_t *)malloc(sizeof(*stk) * bmh_sort_stack_len((size_t)n));
			if ((n && !a) || !stk) return 2;
			if (n) memcpy(a, in, sizeof(*a) * (size_t)n);
			got = bmh_dedup_core(n, a, level, stk);
			++runs;
			if (got != m) {
				fprintf(stderr, "case %d level %g: %d survivors, expected %d\n", c, level, got, m);
				++bad;
			} else
				for (k = 0; k < m; ++k)
					if (want[k] < 0 || want[k] >= n || memcmp(&a[k], &in[want[k]], sizeof(*a))) {
						fprintf(stderr, "case %d level %g: survivor %d is not record %d\n", c, level, k, want[k]);
						++bad;
						break;
					}
			free(stk);
			free(a);
			free(want);
		}
		free(in);
	}
	fclose(f);
	printf("%d runs, %d differ\n", runs, bad);
	return bad ? 1 : 0;
}
