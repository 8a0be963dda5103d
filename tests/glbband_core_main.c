/*
 * glbband_core_main.c -- stand-alone check of host/glbband_core.h for a plain and a sanitizer build:
 * tests/test_global_band_cpu.py compiles it with gcc, links the oracle (liborc.so) and runs it as a child process.
 *
 * For every task it takes w_eff = bmh_glbband_weff(...) with the query and the target each in a heap block of exactly its
 * length (an eight-base load past either end is the sanitizer's to report) and checks
 *   the range    |qlen - tlen| <= w_eff <= w where the rule applies, w_eff == w where it does not, and
 *   the result   orc_global with w_eff == orc_global with w: score, n_cigar and every CIGAR word (mode bit 0), and
 *   the split    the lower bound joined from eight parts, as the device's eight lanes per task take it, is that of one part
 *                (a difference counts as a range error).
 *
 * Input file (little endian, written by the test):
 *   int32 n_cases
 *   per case: bmh_params_t, int32 mode, int64 pool_bytes, the pool, int32 n_tasks, bmh_glb_task_t[n_tasks]
 *     mode bit 0: compare the oracle's results; bit 1: print every w_eff
 * Output: per case one line "case C: N tasks, P applied, R narrowed, B range errors, D differ, cells X -> Y", X and Y the sums of
 * ceil((2w+2)/8) * tlen and ceil((2w_eff+2)/8) * tlen -- the 8-slot blocks a lane kernel computes -- and with mode bit 1 a line
 * "weff C: ..." with every task's w_eff.  Exit status 0: no range error and no difference in any case.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/glbband_core.h"
#include "../include/bwamem_hip.h"
#include "../oracle/ksw_oracle.h"

static int rd(void *p, size_t sz, size_t n, FILE *f) { return n == 0 || fread(p, sz, n, f) == n; }

static uint8_t *exact(const uint8_t *src, int n) /* a block of exactly n bytes (1 for an empty sequence) */
{
	uint8_t *p = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);
	if (!p) exit(2);
	if (n > 0) memcpy(p, src, (size_t)n);
	return p;
}

int main(int argc, char **argv)
{
	FILE *f;
	int32_t n_cases, c;
	long long bad_total = 0;
	if (argc != 2 || !(f = fopen(argv[1], "rb"))) {
		fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
		return 2;
	}
	if (!rd(&n_cases, 4, 1, f)) return 2;
	for (c = 0; c < n_cases; ++c) {
		bmh_params_t P;
		int32_t mode, n_tasks, k;
		int64_t pool_bytes;
		uint8_t *pool;
		bmh_glb_task_t *tasks;
		orc_scoring_t sc;
		int amax, rule;
		long long applied = 0, narrowed = 0, bad = 0, differ = 0, cells0 = 0, cells1 = 0;
		if (!rd(&P, sizeof(P), 1, f) || !rd(&mode, 4, 1, f) || !rd(&pool_bytes, 8, 1, f) || pool_bytes < 0) return 2;
		pool = (uint8_t *)malloc((size_t)pool_bytes + 1);
		if (!pool || !rd(pool, 1, (size_t)pool_bytes, f) || !rd(&n_tasks, 4, 1, f) || n_tasks < 0) return 2;
		tasks = (bmh_glb_task_t *)malloc(sizeof(*tasks) * ((size_t)n_tasks + 1));
		if (!tasks || !rd(tasks, sizeof(*tasks), (size_t)n_tasks, f)) return 2;
		sc.o_del = P.o_del, sc.e_del = P.e_del, sc.o_ins = P.o_ins, sc.e_ins = P.e_ins, sc.zdrop = P.zdrop, sc.m = 5, sc.mat = P.mat;
		amax = bmh_glbband_amax(P.mat);
		rule = bmh_glbband_applies(amax, P.o_del, P.e_del, P.o_ins, P.e_ins);
		if (mode & 2) printf("weff %d:", c);
		for (k = 0; k < n_tasks; ++k) {
			const bmh_glb_task_t *t = tasks + k;
			const int qlen = t->qlen, tlen = t->tlen, w = t->w, ad = abs(qlen - tlen);
			uint8_t *q, *tg;
			int we;
			if (t->q_off + (uint64_t)qlen > (uint64_t)pool_bytes || t->t_off + (uint64_t)tlen > (uint64_t)pool_bytes) return 2;
			q = exact(pool + t->q_off, qlen), tg = exact(pool + t->t_off, tlen);
			we = bmh_glbband_weff(P.mat, P.o_del, P.e_del, P.o_ins, P.e_ins, q, qlen, tg, tlen, w);
			if (mode & 2) printf(" %d", we);
			if (qlen >= 1 && tlen >= 1) { /* the device's split: eight parts of a multiple of eight pairs, joined in order */
				const bmh_gb_walk_t wk = bmh_glbband_walk(P.o_del, P.e_del, P.o_ins, P.e_ins, q, qlen, tg, tlen);
				const int per = ((wk.n + 63) / 64) * 8;
				bmh_gb_part_t acc = {0, 0, 0};
				int g;
				for (g = 0; g < 8; ++g) {
					const int from = g * per < wk.n ? g * per : wk.n, to = from + per < wk.n ? from + per : wk.n;
					const bmh_gb_part_t nx = bmh_glbband_part(P.mat, &wk, from, to);
					bmh_glbband_join(&acc, &nx);
				}
				bad += acc.s1 + acc.b - wk.gap != bmh_glbband_lb(P.mat, P.o_del, P.e_del, P.o_ins, P.e_ins, q, qlen, tg, tlen);
			}
			if (rule && w >= ad && qlen >= 1 && tlen >= 1) {
				++applied;
				bad += !(ad <= we && we <= w);
			} else bad += we != w;
			narrowed += we < w;
			cells0 += (long long)((2 * (w > 0 ? w : 0) + 2 + 7) / 8) * tlen;
			cells1 += (long long)((2 * (we > 0 ? we : 0) + 2 + 7) / 8) * tlen;
			if ((mode & 1) && we != w) {
				int n0 = 0, n1 = 0;
				uint32_t *c0 = NULL, *c1 = NULL;
				const int s0 = orc_global(&sc, qlen, q, tlen, tg, w, &n0, &c0);
				const int s1 = orc_global(&sc, qlen, q, tlen, tg, we, &n1, &c1);
				if (s0 != s1 || n0 != n1 || (n0 > 0 && memcmp(c0, c1, sizeof(uint32_t) * (size_t)n0))) {
					if (++differ <= 5)
						fprintf(stderr, "case %d task %d: qlen %d tlen %d w %d w_eff %d: score %d / %d, n_cigar %d / %d\n", c, k, qlen, tlen, w, we,
						        s0, s1, n0, n1);
				}
				free(c0), free(c1);
			}
			free(q), free(tg);
		}
		if (mode & 2) printf("\n");
		printf("case %d: %d tasks, %lld applied, %lld narrowed, %lld range errors, %lld differ, cells %lld -> %lld\n", c, n_tasks, applied,
		       narrowed, bad, differ, cells0, cells1);
		bad_total += bad + differ;
		free(pool), free(tasks);
	}
	fclose(f);
	return bad_total ? 1 : 0;
}
