/*
 * extband_core_main.c -- stand-alone check of host/extband_core.h for a plain and a sanitizer build: tests/test_ext_band_cpu.py compiles
 * it with gcc, links the oracle (liborc.so) and runs it as a child process.
 *
 * For every task the band w_eff comes from the header, the oracle runs the task at its own w and at w_eff, each with the query and
 * the target in heap blocks of exactly their lengths, and the six outputs must be equal.
 *
 * Usage:
 *   extband_core_main file cases.bin      cases written by the test (little endian):
 *       int32 n_cases; per case: bmh_params_t, int32 mode, int64 pool_bytes, the pool, int32 n_tasks, bmh_ext_task_t[n_tasks]
 *       mode bit 1: print every task's w_eff ("bands C: ...")
 *   extband_core_main exhaustive Q T      every pair of sequences over two letters, query <= Q, target <= T, h0 in {0,1,3,6,8,9,12,20},
 *                                         w in {1,2,3,100}, zdrop in {0,2,12,100}: one case per scoring of scorings[]
 *   extband_core_main random N SEED       N related pairs: indels, mismatch bursts, N, small z-drop, truncated targets, h0 its own or
 *                                         one of {8,12,20,30,80}, a scoring of scorings[] each: one case
 * Output per case: "case C: N tasks, D differ, K narrowed, bands B, cells X0 X1" (K: tasks with w_eff < w; B: the sum of their w_eff;
 * cells: the oracle's, at w and at w_eff).  Exit status 0: no difference in any case.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/extband_core.h"
#include "../include/bwamem_hip.h"
#include "../oracle/ksw_oracle.h"

typedef struct {
	long long n, differ, narrowed, bands, cells[2];
} tally_t;

static uint8_t *exact(const uint8_t *src, int n, int rev) /* a block of exactly n bytes (1 for an empty sequence); rev: src points at base 0 and runs downwards */
{
	uint8_t *p = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);
	int k;
	if (!p) exit(2);
	for (k = 0; k < n; ++k) p[k] = rev ? src[-k] : src[k];
	return p;
}

/* one task through the header and the oracle at both bands; returns w_eff */
static int one(const bmh_params_t *P, tally_t *T, int qlen, const uint8_t *q, int tlen, const uint8_t *t, int w, int end_bonus, int h0, const char *what)
{
	orc_scoring_t sc;
	orc_extend_out_t o[2];
	orc_extend_stats_t st[2] = {{0, 0}, {0, 0}};
	const int we = bmh_extband_weff(P->mat, P->o_del, P->e_del, P->o_ins, P->e_ins, P->zdrop, q, qlen, t, tlen, h0, w);
	sc.o_del = P->o_del, sc.e_del = P->e_del, sc.o_ins = P->o_ins, sc.e_ins = P->e_ins, sc.zdrop = P->zdrop, sc.m = 5, sc.mat = P->mat;
	orc_extend(&sc, qlen, q, tlen, t, w, end_bonus, h0, &o[0], &st[0]);
	orc_extend(&sc, qlen, q, tlen, t, we, end_bonus, h0, &o[1], &st[1]);
	T->cells[0] += st[0].cells, T->cells[1] += st[1].cells;
	if ((we > w || we < 0 || memcmp(&o[0], &o[1], sizeof(o[0])) != 0) && ++T->differ <= 5)
		fprintf(stderr, "%s: qlen %d tlen %d w %d h0 %d w_eff %d: at w %d %d %d %d %d %d, at w_eff %d %d %d %d %d %d\n", what, qlen, tlen, w, h0, we,
		        o[0].score, o[0].qle, o[0].tle, o[0].gtle, o[0].gscore, o[0].max_off, o[1].score, o[1].qle, o[1].tle, o[1].gtle, o[1].gscore,
		        o[1].max_off);
	if (we < w) ++T->narrowed, T->bands += we;
	++T->n;
	return we;
}

static int report(int c, const tally_t *T)
{
	printf("case %d: %lld tasks, %lld differ, %lld narrowed, bands %lld, cells %lld %lld\n", c, T->n, T->differ, T->narrowed, T->bands,
	       T->cells[0], T->cells[1]);
	return T->differ != 0;
}

static void fill_mat(bmh_params_t *P, int a, int b)
{
	int x, y;
	for (x = 0; x < 5; ++x)
		for (y = 0; y < 5; ++y) P->mat[x * 5 + y] = (int8_t)(x == 4 || y == 4 ? -1 : x == y ? a : -b);
}

/* {a, b, o_del, e_del, o_ins, e_ins}: bwa's default, o = 0, asymmetric, A = 3, all ones, a zero open on one side only, e = 0 on both
 * sides, e = 0 on one */
#define N_SCORINGS 8
static const int scorings[N_SCORINGS][6] = {{1, 4, 6, 1, 6, 1}, {1, 4, 0, 1, 0, 1}, {1, 4, 6, 1, 4, 2}, {3, 4, 5, 2, 5, 2},
                                            {1, 1, 1, 1, 1, 1}, {2, 3, 0, 2, 3, 1}, {1, 4, 6, 0, 6, 0}, {1, 4, 3, 0, 6, 1}};

static void scoring(bmh_params_t *P, int s, int zdrop)
{
	memset(P, 0, sizeof(*P));
	fill_mat(P, scorings[s][0], scorings[s][1]);
	P->a = scorings[s][0], P->o_del = scorings[s][2], P->e_del = scorings[s][3], P->o_ins = scorings[s][4], P->e_ins = scorings[s][5];
	P->zdrop = zdrop, P->w = 100;
}

static int exhaustive(int qmax, int tmax)
{
	static const int h0s[8] = {0, 1, 3, 6, 8, 9, 12, 20}, ws[4] = {1, 2, 3, 100}, zs[4] = {0, 2, 12, 100};
	int s, ql, tl, a, b, c, k, fail = 0;
	unsigned qb, tb;
	for (s = 0; s < N_SCORINGS; ++s) {
		tally_t T;
		memset(&T, 0, sizeof(T));
		for (c = 0; c < 4; ++c) {
			bmh_params_t P;
			scoring(&P, s, zs[c]);
			for (ql = 1; ql <= qmax; ++ql)
				for (qb = 0; qb < 1u << ql; ++qb)
					for (tl = 1; tl <= tmax; ++tl)
						for (tb = 0; tb < 1u << tl; ++tb) {
							uint8_t *q = (uint8_t *)malloc((size_t)ql), *t = (uint8_t *)malloc((size_t)tl);
							if (!q || !t) exit(2);
							for (k = 0; k < ql; ++k) q[k] = qb >> k & 1;
							for (k = 0; k < tl; ++k) t[k] = tb >> k & 1;
							for (a = 0; a < 8; ++a)
								for (b = 0; b < 4; ++b) one(&P, &T, ql, q, tl, t, ws[b], 0, h0s[a], "exhaustive");
							free(q), free(t);
						}
		}
		fail |= report(s, &T);
	}
	return fail;
}

static uint64_t rng_state;
static uint32_t rnd(void) /* splitmix64 */
{
	uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
	z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ z >> 27) * 0x94d049bb133111ebull;
	return (uint32_t)((z ^ z >> 31) >> 16);
}
static int below(int n) { return n > 0 ? (int)(rnd() % (uint32_t)n) : 0; }

static int random_pairs(long long n, uint64_t seed)
{
	static const int zs[5] = {0, 3, 10, 30, 100}, ws[6] = {1, 2, 5, 20, 50, 100}, hs[5] = {8, 12, 20, 30, 80};
	tally_t T;
	long long it;
	memset(&T, 0, sizeof(T));
	rng_state = seed;
	for (it = 0; it < n; ++it) {
		bmh_params_t P;
		const int ql = 1 + (below(4) ? below(150) : below(12)), alpha = below(5) ? 4 : 1 + below(2);
		const int psub = below(3) ? below(4) : below(4) ? 1 + below(8) : 10 + below(30), pindel = below(3) ? below(3) : 3 + below(8);
		const int pn = below(4) ? 0 : 1 + below(20);
		uint8_t *q = (uint8_t *)malloc((size_t)ql), *t = (uint8_t *)malloc((size_t)(3 * ql + 64));
		int tl = 0, k, burst = 0, want;
		if (!q || !t) exit(2);
		scoring(&P, below(N_SCORINGS), zs[below(5)]);
		for (k = 0; k < ql; ++k) q[k] = (uint8_t)(below(100) < pn ? 4 : below(alpha));
		for (k = 0; k < ql && tl < 3 * ql + 32; ++k) { /* the target: the query with mismatches (in bursts), indels and N */
			const int r = below(100);
			if (burst > 0 || r < psub) {
				if (burst <= 0 && !below(4)) burst = 2 + below(10);
				--burst;
				t[tl++] = (uint8_t)below(4);
			} else if (r < psub + pindel) {
				int len = 1 + below(below(3) ? 2 : 12);
				if (below(2)) k += len - 1;
				else
					while (len-- > 0 && tl < 3 * ql + 32) t[tl++] = (uint8_t)below(alpha);
			} else t[tl++] = (uint8_t)(below(100) < pn ? 4 : q[k] > 3 ? below(4) : q[k]);
		}
		want = below(4) == 0 ? below(tl + 1) : tl + below(ql + 20); /* a truncated target, or a tail of other bases as mem_chain2aln's max_gap leaves */
		while (tl < want && tl < 3 * ql + 64) t[tl++] = (uint8_t)below(alpha);
		tl = want < tl ? want : tl;
		if (tl < 1) t[0] = 0, tl = 1;
		{
			uint8_t *tx = exact(t, tl, 0);
			one(&P, &T, ql, q, tl, tx, ws[below(6)], below(3) ? 5 : below(12), below(2) ? hs[below(5)] : below(5) ? below(121) : below(4), "random");
			free(tx);
		}
		free(q), free(t);
	}
	return report(0, &T);
}

static int rd(void *p, size_t sz, size_t n, FILE *f) { return n == 0 || fread(p, sz, n, f) == n; }

static int from_file(const char *path)
{
	FILE *f = fopen(path, "rb");
	int32_t n_cases, c;
	int fail = 0;
	if (!f || !rd(&n_cases, 4, 1, f)) return 2;
	for (c = 0; c < n_cases; ++c) {
		bmh_params_t P;
		int32_t mode, n_tasks, k;
		int64_t pool_bytes;
		uint8_t *pool;
		bmh_ext_task_t *tasks;
		tally_t T;
		memset(&T, 0, sizeof(T));
		if (!rd(&P, sizeof(P), 1, f) || !rd(&mode, 4, 1, f) || !rd(&pool_bytes, 8, 1, f) || pool_bytes < 0) return 2;
		pool = (uint8_t *)malloc((size_t)pool_bytes + 1);
		if (!pool || !rd(pool, 1, (size_t)pool_bytes, f) || !rd(&n_tasks, 4, 1, f) || n_tasks < 0) return 2;
		tasks = (bmh_ext_task_t *)malloc(sizeof(*tasks) * ((size_t)n_tasks + 1));
		if (!tasks || !rd(tasks, sizeof(*tasks), (size_t)n_tasks, f)) return 2;
		if (mode & 2) printf("bands %d:", c);
		for (k = 0; k < n_tasks; ++k) {
			const bmh_ext_task_t *t = tasks + k;
			const int qr = t->flags & BMH_F_QREV, tr = t->flags & BMH_F_TREV, ql = t->qlen, tl = t->tlen;
			uint8_t *q, *tg;
			int we;
			if (t->flags & BMH_F_TPAC) return 2;
			if ((qr ? t->q_off + 1 < (uint64_t)ql || t->q_off >= (uint64_t)pool_bytes : t->q_off + (uint64_t)ql > (uint64_t)pool_bytes) ||
			    (tr ? t->t_off + 1 < (uint64_t)tl || t->t_off >= (uint64_t)pool_bytes : t->t_off + (uint64_t)tl > (uint64_t)pool_bytes))
				return 2;
			q = exact(pool + t->q_off, ql, qr), tg = exact(pool + t->t_off, tl, tr);
			we = one(&P, &T, ql, q, tl, tg, t->w, t->end_bonus, t->h0, "file");
			if (mode & 2) printf(" %d", we);
			free(q), free(tg);
		}
		if (mode & 2) printf("\n");
		fail |= report(c, &T);
		free(pool), free(tasks);
	}
	fclose(f);
	return fail;
}

int main(int argc, char **argv)
{
	if (argc == 3 && !strcmp(argv[1], "file")) return from_file(argv[2]);
	if (argc == 4 && !strcmp(argv[1], "exhaustive")) return exhaustive(atoi(argv[2]), atoi(argv[3]));
	if (argc == 4 && !strcmp(argv[1], "random")) return random_pairs(atoll(argv[2]), strtoull(argv[3], NULL, 10));
	fprintf(stderr, "usage: %s file cases.bin | exhaustive Q T | random N SEED\n", argv[0]);
	return 2;
}
