/*
 * extstop_core_main.c -- stand-alone check of host/extstop_core.h for a plain and a sanitizer build: tests/test_ext_stop_cpu.py compiles
 * it with gcc, links the oracle (liborc.so) and runs it as a child process.
 *
 * ext() below is a plain restatement of ksw_extend2 (reference bwa-0.7.8/ksw.c:379-476) that can end a flank by the header's rule:
 *   form 0   never (the reference's rows),
 *   form 1   the bound taken per cell,
 *   form 2   the bound taken per block of eight columns counted from the query's right end, as the lane kernels take it.
 * For every task all three run, each with the query and the target in heap blocks of exactly their lengths, and
 *   form 0 must give the oracle's six outputs, rows and cells (the restatement is the oracle's equal),
 *   forms 1 and 2 must give the oracle's six outputs,
 *   rows(form 1) <= rows(form 2) <= rows(form 0), and where the rule does not apply all three are equal.
 *
 * Usage:
 *   extstop_core_main file cases.bin      cases written by the test (little endian):
 *       int32 n_cases; per case: bmh_params_t, int32 mode, int64 pool_bytes, the pool, int32 n_tasks, bmh_ext_task_t[n_tasks]
 *       mode bit 1: print every task's rows of form 2 ("rows C: ...")
 *   extstop_core_main exhaustive Q T      every pair of sequences over two letters, query <= Q, target <= T, h0 in {0,1,3,9},
 *                                         w in {1,2,100}, zdrop in {0,2,100}: one case per scoring of scorings[]
 *   extstop_core_main random N SEED       N related pairs: indels, mismatch bursts, N, small z-drop, truncated targets, h0 up to 120,
 *                                         a scoring of scorings[] each: one case
 * Output per case: "case C: N tasks, D differ, O order errors, K cut, rows R0 R1 R2, cells X0 X1 X2" (sums per form; cut: tasks
 * whose form 2 ran fewer rows than form 0).  Exit status 0: no difference and no order error in any case.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/extstop_core.h"
#include "../include/bwamem_hip.h"
#include "../oracle/ksw_oracle.h"

typedef struct {
	int out[6]; /* score, qle, tle, gtle, gscore, max_off */
	int rows;
	long long cells;
} ext_t;

typedef struct {
	int h, e;
} eh_t;

static ext_t ext(const bmh_params_t *P, int form, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int w, int end_bonus, int h0)
{
	const int o_del = P->o_del, e_del = P->e_del, o_ins = P->o_ins, e_ins = P->e_ins, zdrop = P->zdrop;
	const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
	const int factor = bmh_extstop_factor(form != 0, P->mat, o_del, e_del, o_ins, e_ins);
	eh_t *eh = (eh_t *)calloc((size_t)qlen + 1, sizeof(eh_t));
	int i, j, beg, end, max, max_i, max_j, max_ins, max_del, max_ie, gscore, max_off;
	ext_t r;
	if (!eh) exit(2);
	if (h0 < 0) h0 = 0;
	eh[0].h = h0;
	if (qlen >= 1) eh[1].h = h0 > oe_ins ? h0 - oe_ins : 0;
	for (j = 2; j <= qlen && eh[j - 1].h > e_ins; ++j) eh[j].h = eh[j - 1].h - e_ins;
	for (i = 0, max = 0; i < 25; ++i) max = max > P->mat[i] ? max : P->mat[i];
	max_ins = (int)((double)(qlen * max + end_bonus - o_ins) / e_ins + 1.);
	max_ins = max_ins > 1 ? max_ins : 1;
	w = w < max_ins ? w : max_ins;
	max_del = (int)((double)(qlen * max + end_bonus - o_del) / e_del + 1.);
	max_del = max_del > 1 ? max_del : 1;
	w = w < max_del ? w : max_del;
	max = h0, max_i = max_j = -1, max_ie = -1, gscore = -1, max_off = 0;
	beg = 0, end = qlen;
	r.rows = 0, r.cells = 0;
	for (i = 0; i < tlen; ++i) {
		int t, f = 0, h1, m = 0, mj = -1, u;
		const int8_t *srow = P->mat + (target[i] > 4 ? 4 : target[i]) * 5;
		h1 = h0 - (o_del + e_del * (i + 1));
		if (h1 < 0) h1 = 0;
		if (beg < i - w) beg = i - w;
		if (end > i + w + 1) end = i + w + 1;
		if (end > qlen) end = qlen;
		++r.rows, r.cells += end > beg ? end - beg : 0;
		u = bmh_extstop_first(h1, factor, qlen - beg);
		for (j = beg; j < end; ++j) {
			eh_t *p = &eh[j];
			int h = p->h, e = p->e;
			p->h = h1;
			h += srow[query[j] > 4 ? 4 : query[j]];
			h = h > e ? h : e;
			h = h > f ? h : f;
			h1 = h;
			mj = m > h ? mj : j;
			m = m > h ? m : h;
			t = h - oe_del;
			t = t > 0 ? t : 0;
			e -= e_del;
			e = e > t ? e : t;
			p->e = e;
			t = h - oe_ins;
			t = t > 0 ? t : 0;
			f -= e_ins;
			f = f > t ? f : t;
			if (form == 1) u = bmh_extstop_block(u, h, factor, qlen - 1 - j);
			else if ((qlen - 1 - j) % 8 == 0 || j == end - 1) /* the block's last column, or the row's: m is the maximum up to here */
				u = bmh_extstop_block(u, m, factor, (qlen - 1 - j) / 8 * 8 + 7);
		}
		eh[end].h = h1, eh[end].e = 0;
		if (j == qlen) {
			max_ie = gscore > h1 ? max_ie : i;
			gscore = gscore > h1 ? gscore : h1;
		}
		if (m == 0) break;
		if (m > max) {
			max = m, max_i = i, max_j = mj;
			max_off = max_off > abs(mj - i) ? max_off : abs(mj - i);
		} else if (zdrop > 0) {
			if (i - max_i > mj - max_j) {
				if (max - m - ((i - max_i) - (mj - max_j)) * e_del > zdrop) break;
			} else {
				if (max - m - ((mj - max_j) - (i - max_i)) * e_ins > zdrop) break;
			}
		}
		if (form && bmh_extstop_test(u, max, gscore)) break;
		for (j = mj; j >= beg && eh[j].h; --j) {}
		beg = j + 1;
		for (j = mj + 2; j <= end && eh[j].h; ++j) {}
		end = j;
	}
	free(eh);
	r.out[0] = max, r.out[1] = max_j + 1, r.out[2] = max_i + 1, r.out[3] = max_ie + 1, r.out[4] = gscore, r.out[5] = max_off;
	return r;
}

typedef struct {
	long long n, differ, order, cut, rows[3], cells[3];
} tally_t;

static uint8_t *exact(const uint8_t *src, int n, int rev) /* a block of exactly n bytes (1 for an empty sequence); rev: src points at base 0 and runs downwards */
{
	uint8_t *p = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);
	int k;
	if (!p) exit(2);
	for (k = 0; k < n; ++k) p[k] = rev ? src[-k] : src[k];
	return p;
}

/* one task through the oracle and the three forms; returns form 2's rows */
static int one(const bmh_params_t *P, tally_t *T, int qlen, const uint8_t *q, int tlen, const uint8_t *t, int w, int end_bonus, int h0, const char *what)
{
	orc_scoring_t sc;
	orc_extend_out_t o;
	orc_extend_stats_t st = {0, 0};
	ext_t r[3];
	int want[6], f, bad = 0;
	const int applies = bmh_extstop_factor(1, P->mat, P->o_del, P->e_del, P->o_ins, P->e_ins) != BMH_EXTSTOP_OFF;
	sc.o_del = P->o_del, sc.e_del = P->e_del, sc.o_ins = P->o_ins, sc.e_ins = P->e_ins, sc.zdrop = P->zdrop, sc.m = 5, sc.mat = P->mat;
	orc_extend(&sc, qlen, q, tlen, t, w, end_bonus, h0, &o, &st);
	want[0] = o.score, want[1] = o.qle, want[2] = o.tle, want[3] = o.gtle, want[4] = o.gscore, want[5] = o.max_off;
	for (f = 0; f < 3; ++f) {
		r[f] = ext(P, f, qlen, q, tlen, t, w, end_bonus, h0);
		bad |= memcmp(r[f].out, want, sizeof(want)) != 0;
		T->rows[f] += r[f].rows, T->cells[f] += r[f].cells;
	}
	bad |= r[0].rows != st.rows || r[0].cells != st.cells;
	if (bad && ++T->differ <= 5)
		fprintf(stderr, "%s: qlen %d tlen %d w %d h0 %d: oracle %d %d %d %d %d %d rows %d, form 2 %d %d %d %d %d %d rows %d\n", what, qlen, tlen, w, h0,
		        want[0], want[1], want[2], want[3], want[4], want[5], st.rows, r[2].out[0], r[2].out[1], r[2].out[2], r[2].out[3], r[2].out[4],
		        r[2].out[5], r[2].rows);
	if (!(r[1].rows <= r[2].rows && r[2].rows <= r[0].rows) || (!applies && r[1].rows != r[0].rows)) ++T->order;
	T->cut += r[2].rows < r[0].rows;
	++T->n;
	return r[2].rows;
}

static int report(int c, const tally_t *T)
{
	printf("case %d: %lld tasks, %lld differ, %lld order errors, %lld cut, rows %lld %lld %lld, cells %lld %lld %lld\n", c, T->n, T->differ,
	       T->order, T->cut, T->rows[0], T->rows[1], T->rows[2], T->cells[0], T->cells[1], T->cells[2]);
	return T->differ || T->order;
}

static void fill_mat(bmh_params_t *P, int a, int b)
{
	int x, y;
	for (x = 0; x < 5; ++x)
		for (y = 0; y < 5; ++y) P->mat[x * 5 + y] = (int8_t)(x == 4 || y == 4 ? -1 : x == y ? a : -b);
}

/* {a, b, o_del, e_del, o_ins, e_ins}: bwa's default, o = 0, asymmetric, A = 3, all ones, a zero open on one side only */
static const int scorings[6][6] = {{1, 4, 6, 1, 6, 1}, {1, 4, 0, 1, 0, 1}, {1, 4, 6, 1, 4, 2}, {3, 4, 5, 2, 5, 2}, {1, 1, 1, 1, 1, 1}, {2, 3, 0, 2, 3, 1}};

static void scoring(bmh_params_t *P, int s, int zdrop)
{
	memset(P, 0, sizeof(*P));
	fill_mat(P, scorings[s][0], scorings[s][1]);
	P->a = scorings[s][0], P->o_del = scorings[s][2], P->e_del = scorings[s][3], P->o_ins = scorings[s][4], P->e_ins = scorings[s][5];
	P->zdrop = zdrop, P->w = 100;
}

static int exhaustive(int qmax, int tmax)
{
	static const int h0s[4] = {0, 1, 3, 9}, ws[3] = {1, 2, 100}, zs[3] = {0, 2, 100};
	int s, ql, tl, a, b, c, k, fail = 0;
	unsigned qb, tb;
	for (s = 0; s < 6; ++s) {
		tally_t T;
		memset(&T, 0, sizeof(T));
		for (c = 0; c < 3; ++c) {
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
							for (a = 0; a < 4; ++a)
								for (b = 0; b < 3; ++b) one(&P, &T, ql, q, tl, t, ws[b], 0, h0s[a], "exhaustive");
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
	static const int zs[5] = {0, 3, 10, 30, 100}, ws[6] = {1, 2, 5, 20, 50, 100};
	tally_t T;
	long long it;
	memset(&T, 0, sizeof(T));
	rng_state = seed;
	for (it = 0; it < n; ++it) {
		bmh_params_t P;
		const int ql = 1 + (below(4) ? below(150) : below(12)), alpha = below(5) ? 4 : 1 + below(2);
		const int psub = below(4) ? 1 + below(8) : 10 + below(30), pindel = below(3) ? below(3) : 3 + below(8), pn = below(4) ? 0 : 1 + below(20);
		uint8_t *q = (uint8_t *)malloc((size_t)ql), *t = (uint8_t *)malloc((size_t)(3 * ql + 64));
		int tl = 0, k, burst = 0, want;
		if (!q || !t) exit(2);
		scoring(&P, below(6), zs[below(5)]);
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
			one(&P, &T, ql, q, tl, tx, ws[below(6)], below(3) ? 5 : below(12), below(5) ? below(121) : below(4), "random");
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
		if (mode & 2) printf("rows %d:", c);
		for (k = 0; k < n_tasks; ++k) {
			const bmh_ext_task_t *t = tasks + k;
			const int qr = t->flags & BMH_F_QREV, tr = t->flags & BMH_F_TREV, ql = t->qlen, tl = t->tlen;
			uint8_t *q, *tg;
			int rows;
			if (t->flags & BMH_F_TPAC) return 2;
			if ((qr ? t->q_off + 1 < (uint64_t)ql || t->q_off >= (uint64_t)pool_bytes : t->q_off + (uint64_t)ql > (uint64_t)pool_bytes) ||
			    (tr ? t->t_off + 1 < (uint64_t)tl || t->t_off >= (uint64_t)pool_bytes : t->t_off + (uint64_t)tl > (uint64_t)pool_bytes))
				return 2;
			q = exact(pool + t->q_off, ql, qr), tg = exact(pool + t->t_off, tl, tr);
			rows = one(&P, &T, ql, q, tl, tg, t->w, t->end_bonus, t->h0, "file");
			if (mode & 2) printf(" %d", rows);
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
