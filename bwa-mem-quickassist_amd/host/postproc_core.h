/*
 * postproc_core.h -- pass A of phase 2 (what gets printed, and with which mapQ) as ONE text for its two forms: the host routines
 * of host/sam_post.c (gcc: bmh_mark_primary_se, bmh_approx_mapq_se, bmh_pair, bmh_decide_batch) and the device kernel behind
 * bmh_decide_device (csrc/decide.hip, hipcc, one lane per read or pair).
 *   bmh_pp_mark        mem_mark_primary_se     reference bwa-0.7.8/bwamem.c:445-475 (hash_64: utils.h:98-109)
 *   bmh_pp_mapq        mem_approx_mapq_se      bwamem.c:1023-1047
 *   bmh_pp_pair        mem_pair                bwamem_pair.c:177-238 (mem_infer_dir :25-32)
 *   bmh_pp_want_se     the selection of mem_reg2sam_se, bwamem.c:1057-1062
 *   bmh_pp_unit_se/pe  worker2's two branches (bwamem.c:1285-1293) up to that selection: for a pair the tail of mem_sam_pe
 *                      (bwamem_pair.c:264-331: multi-hit test, pair against single ends, q_pe, q_se, the tandem-repeat cap)
 * Nothing is allocated: the z[] list of the marking (n ints), the v[] keys of the pairing (n0 + n1 records) and the range stack of
 * the two exact introsorts (sort_exact.h, bmh_sort_stack_len entries) are the caller's.  Under hipcc every routine is
 * __host__ __device__ and always inlined; the C subset used is what lets gcc compile the same text.
 *
 * mem_pair's second vector is gone.  The reference collects every proper pair in u, sorts u by (x, y) and reads the last two
 * records and a count off it.  y = k<<32|i is unique, so that order is total and the sorted u is determined by u's set: the walk
 * below keeps the two largest records as it meets them, and a second walk counts n_sub (every record but the best one whose q lies
 * within one event of the runner-up's).
 *
 * Floating point, where the two builds could part:
 *  - log and erfc never run on the device (ocml and glibc do not promise the same last bit).  Every value the decisions need has an
 *    integer argument, so the host tabulates them with its own libm (bmh_pp_fill_log, bmh_pp_fill_term below, gcc only) and the
 *    device looks them up: BMH_PP_LOG(t, k) is log((double)k), BMH_PP_TERM(t, o, pes, dir, dist) is the insert-size term of
 *    mem_pair for orientation dir at distance dist in [low, high].  Under gcc the two macros are the libm expressions themselves.
 *    q is then (double)(s_i + s_k) + term + .499 on both sides: two IEEE additions.
 *  - contraction: hipcc's default for gfx950 fuses a multiply and a following add into one fused multiply-add, gcc for x86-64 does
 *    not.  Every routine that holds such a pair (... * tmp * tmp + .499, 4.343 * log + .499, mapq * identity * identity + .499,
 *    MEM_MAPQ_COEF * ... * log + .499) starts with BMH_PP_NOCONTRACT (#pragma clang fp contract(off)); divisions are correctly
 *    rounded on both sides.
 *  - double -> int: x86 turns NaN, the infinities and out-of-range doubles into INT32_MIN, the GPU's conversion saturates and turns
 *    NaN into 0.  Every (int) of a double goes through bmh_pp_d2i, which gives INT32_MIN for anything not strictly inside
 *    (-2147483649, 2147483648): std == 0, erfc -> 0, seedcov == 0 with mapQ_coef_len <= 0.
 *  - the single-precision test e_min - b_max >= min_l * mask_level and the double test score < a[secondary].score * .5 are one
 *    multiply and a compare each: nothing to contract, IEEE on both sides.  Keep them as they are.
 */
#ifndef BMH_POSTPROC_CORE_H
#define BMH_POSTPROC_CORE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bwamem_hip.h"
#include "sort_exact.h"

#ifdef __HIPCC__
#define BMH_PP_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_PP_HD
#endif
#ifdef __clang__
#define BMH_PP_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define BMH_PP_NOCONTRACT
#endif

#define BMH_PP_MAPQ_COEF 30.0 /* MEM_MAPQ_COEF, bwamem.h:11 */

typedef struct { uint64_t x, y; } bmh_pair64_t; /* pair64_t, utils.h:45 */

/* the device's tables (unused under gcc): logk[k] = log((double)k), k = 0..n_log-1; term[term_off[dir] + dist - pes[dir].low] for
 * every orientation that has not failed */
typedef struct bmh_pp_tab {
	const double *logk, *term;
	int64_t term_off[4];
	int64_t n_log, n_term;
} bmh_pp_tab_t;

#ifdef __HIPCC__
#define BMH_PP_LOG(t, k) ((t)->logk[k])
#define BMH_PP_TERM(t, o, pes, dir, dist) ((t)->term[(t)->term_off[dir] + ((dist) - (int64_t)(pes)[dir].low)])
#else
/* bwamem_pair.c:213-214 as sam_post.c spelled it: ns in a double of its own, .721 = 1/log(4) */
static inline double bmh_pp_term_libm(const bmh_sam_opt_t *o, const bmh_pestat_t *p, int64_t dist)
{
	const double ns = (dist - p->avg) / p->std;
	return .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * o->a;
}
#define BMH_PP_LOG(t, k) log((double)(k))
#define BMH_PP_TERM(t, o, pes, dir, dist) bmh_pp_term_libm((o), &(pes)[dir], (dist))
/* the tables, by the same libm and the same expressions */
static inline void bmh_pp_fill_log(double *logk, int64_t k0, int64_t k1)
{
	int64_t k;
	for (k = k0; k < k1; ++k) logk[k] = BMH_PP_LOG(0, (int)k);
}
static inline void bmh_pp_fill_term(const bmh_sam_opt_t *o, const bmh_pestat_t *pes, const int64_t term_off[4], double *term)
{
	int d;
	int64_t dist;
	for (d = 0; d < 4; ++d) {
		if (pes[d].failed) continue;
		for (dist = pes[d].low; dist <= pes[d].high; ++dist) term[term_off[d] + (dist - pes[d].low)] = BMH_PP_TERM(0, o, pes, d, dist);
	}
}
#endif

/* what both forms of the batch call refuse as BMH_E_ARG (host only) */
static inline int bmh_pp_check_args(const bmh_sam_opt_t *o, const bmh_pestat_t *pes, int n, const bmh_alnreg_v *regs, const int64_t *roff,
                                    const bmh_pairdec_t *pd, const int32_t *reg_mapq, const int32_t *n_want, const int32_t *want_k)
{
	int64_t at = 0;
	int i;
	if (!o || n < 0) return BMH_E_ARG;
	if ((o->flag & BMH_MEM_F_PE) && ((n & 1) || !pes || (n > 0 && !pd))) return BMH_E_ARG;
	if (n > 0 && (!regs || !roff || !reg_mapq || !n_want || !want_k)) return BMH_E_ARG;
	for (i = 0; i < n; ++i) {
		if ((regs[i].n && !regs[i].a) || regs[i].n > 0x7fffffffu || roff[i] != at) return BMH_E_ARG;
		at += (int64_t)regs[i].n;
	}
	return n > 0 && roff[n] != at ? BMH_E_ARG : BMH_OK;
}

/* entries of orientation d's run of the pair table (0 for one that failed or has an empty window) */
BMH_PP_HD static inline int64_t bmh_pp_term_len(const bmh_pestat_t *p) { return p->failed || p->high < p->low ? 0 : (int64_t)p->high - p->low + 1; }

BMH_PP_HD static inline int bmh_pp_imin(int a, int b) { return a < b ? a : b; }
BMH_PP_HD static inline int bmh_pp_imax(int a, int b) { return a > b ? a : b; }

BMH_PP_HD static inline int bmh_pp_d2i(double x) { return x > -2147483649. && x < 2147483648. ? (int)x : INT32_MIN; }

BMH_PP_HD static inline uint64_t bmh_pp_hash_64(uint64_t key) /* utils.h:98-109 */
{
	key += ~(key << 32);
	key ^= (key >> 22);
	key += ~(key << 13);
	key ^= (key >> 8);
	key += (key << 3);
	key ^= (key >> 15);
	key += ~(key << 27);
	key ^= (key >> 31);
	return key;
}

BMH_PP_HD static inline int bmh_pp_gap_tmp(const bmh_sam_opt_t *o) /* the largest single-event penalty, bwamem.c:455-457 */
{
	int tmp = o->a + o->b;
	tmp = o->o_del + o->e_del > tmp ? o->o_del + o->e_del : tmp;
	return o->o_ins + o->e_ins > tmp ? o->o_ins + o->e_ins : tmp;
}

/* ---- orders (bwamem.c:386-393, utils.c:45).  hipcc takes them as callables the sort inlines, gcc as functions. */
BMH_PP_HD static inline int bmh_pp_lt_score_hash(const void *x, const void *y)
{
	const bmh_alnreg_t *a = (const bmh_alnreg_t *)x, *b = (const bmh_alnreg_t *)y;
	return a->score > b->score || (a->score == b->score && a->hash < b->hash);
}
BMH_PP_HD static inline int bmh_pp_lt_pair64(const void *p, const void *q)
{
	const bmh_pair64_t *a = (const bmh_pair64_t *)p, *b = (const bmh_pair64_t *)q;
	return a->x < b->x || (a->x == b->x && a->y < b->y);
}
#ifdef __HIPCC__
struct bmh_pp_lt_score_hash_t {
	BMH_PP_HD int operator()(const void *a, const void *b) const { return bmh_pp_lt_score_hash(a, b); }
};
struct bmh_pp_lt_pair64_t {
	BMH_PP_HD int operator()(const void *a, const void *b) const { return bmh_pp_lt_pair64(a, b); }
};
#define BMH_PP_LT_SCORE_HASH bmh_pp_lt_score_hash_t()
#define BMH_PP_LT_PAIR64 bmh_pp_lt_pair64_t()
#else
#define BMH_PP_LT_SCORE_HASH bmh_pp_lt_score_hash
#define BMH_PP_LT_PAIR64 bmh_pp_lt_pair64
#endif

/* ---- bwamem.c:445-475 over a[0..n); z: n ints; stk: bmh_sort_stack_len(n) entries (unused for n < 3) */
BMH_PP_HD static inline void bmh_pp_mark(const bmh_sam_opt_t *o, int n, bmh_alnreg_t *a, int64_t id, int *z, bmh_sort_stk_t *stk)
{
	int i, k, nz = 0, tmp;
	if (n == 0) return;
	for (i = 0; i < n; ++i) a[i].sub = 0, a[i].secondary = -1, a[i].hash = bmh_pp_hash_64((uint64_t)(id + i));
	bmh_sort_exact_stk(a, (size_t)n, sizeof(*a), BMH_PP_LT_SCORE_HASH, stk);
	tmp = bmh_pp_gap_tmp(o);
	z[nz++] = 0;
	for (i = 1; i < n; ++i) {
		for (k = 0; k < nz; ++k) {
			const int j = z[k];
			const int b_max = bmh_pp_imax(a[j].qb, a[i].qb), e_min = bmh_pp_imin(a[j].qe, a[i].qe);
			if (e_min > b_max) { /* overlap on the query */
				const int min_l = bmh_pp_imin(a[i].qe - a[i].qb, a[j].qe - a[j].qb);
				if (e_min - b_max >= min_l * o->mask_level) { /* significant */
					if (a[j].sub == 0) a[j].sub = a[i].score;
					if (a[j].score - a[i].score <= tmp) ++a[j].sub_n;
					break;
				}
			}
		}
		if (k == nz) z[nz++] = i;
		else a[i].secondary = z[k];
	}
}

/* the alignment length mem_approx_mapq_se takes logarithms of (bwamem.c:1029) */
BMH_PP_HD static inline int bmh_pp_len(const bmh_alnreg_t *a) { return a->qe - a->qb > a->re - a->rb ? a->qe - a->qb : (int)(a->re - a->rb); }

/* ---- bwamem.c:1023-1047 */
BMH_PP_HD static inline int bmh_pp_mapq(const bmh_sam_opt_t *o, const bmh_alnreg_t *a, const bmh_pp_tab_t *t)
{
	BMH_PP_NOCONTRACT
	int mapq, l, sub = a->sub ? a->sub : o->min_seed_len * o->a;
	double identity;
	(void)t;
	sub = a->csub > sub ? a->csub : sub;
	if (sub >= a->score) return 0;
	l = bmh_pp_len(a);
	identity = 1. - (double)(l * o->a - a->score) / (o->a + o->b) / l;
	if (a->score == 0) mapq = 0;
	else if (o->mapQ_coef_len > 0) {
		double tmp;
		tmp = l < o->mapQ_coef_len ? 1. : o->mapQ_coef_fac / BMH_PP_LOG(t, l);
		tmp *= identity * identity;
		mapq = bmh_pp_d2i(6.02 * (a->score - sub) / o->a * tmp * tmp + .499);
	} else {
		mapq = bmh_pp_d2i(BMH_PP_MAPQ_COEF * (1. - (double)sub / a->score) * BMH_PP_LOG(t, a->seedcov) + .499);
		mapq = identity < 0.95 ? bmh_pp_d2i(mapq * identity * identity + .499) : mapq;
	}
	if (a->sub_n > 0) mapq = (int)((unsigned)mapq - (unsigned)bmh_pp_d2i(4.343 * BMH_PP_LOG(t, a->sub_n + 1) + .499)); /* (wraps as the reference's does) */
	if (mapq > 60) mapq = 60;
	if (mapq < 0) mapq = 0;
	return mapq;
}

/* ---- bwamem_pair.c:25-32 */
BMH_PP_HD static inline int bmh_pp_infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist)
{
	const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
	const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2; /* read 2 on the strand of read 1 */
	*dist = p2 > b1 ? p2 - b1 : b1 - p2;
	return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

BMH_PP_HD static inline int bmh_pp_raw_mapq(int diff, int a) /* bwamem_pair.c:238 */
{
	return bmh_pp_d2i(6.02 * diff / a + .499);
}

/* ---- bwamem_pair.c:177-238 over the two ends' vectors a0[0..n0), a1[0..n1); v: n0 + n1 records; stk: bmh_sort_stack_len(n0 + n1)
 * entries.  Returns the best pair's score (0 = none), *sub / *n_sub as mem_pair, z[] the chosen hit of each end (untouched if none). */
BMH_PP_HD static inline int bmh_pp_pair(const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t *pes, const bmh_pp_tab_t *t, int n0,
                                        const bmh_alnreg_t *a0, int n1, const bmh_alnreg_t *a1, uint64_t id, int *sub, int *n_sub, int z[2],
                                        bmh_pair64_t *v, bmh_sort_stk_t *stk)
{
	BMH_PP_NOCONTRACT
	const size_t nv = (size_t)n0 + (size_t)n1;
	const int tmp = bmh_pp_gap_tmp(o);
	bmh_pair64_t best = {0, 0}, second = {0, 0};
	size_t i, nu = 0;
	int r, y[4], pass;
	(void)t;
	for (r = 0, nu = 0; r < 2; ++r) {
		const bmh_alnreg_t *a = r ? a1 : a0;
		const size_t n = (size_t)(r ? n1 : n0);
		for (i = 0; i < n; ++i) {
			const bmh_alnreg_t *e = &a[i];
			bmh_pair64_t *key = &v[nu++];
			key->x = (uint64_t)(e->rb < l_pac ? e->rb : (l_pac << 1) - 1 - e->rb); /* forward position */
			key->y = (uint64_t)e->score << 32 | (uint64_t)(i << 2) | (uint64_t)((e->rb >= l_pac) << 1) | (uint64_t)r;
		}
	}
	bmh_sort_exact_stk(v, nv, sizeof(bmh_pair64_t), BMH_PP_LT_PAIR64, stk);
	*sub = 0, *n_sub = 0;
	/* pass 0: the two largest records of u; pass 1 (if there is one): n_sub */
	for (pass = 0, nu = 0; pass < 2; ++pass) {
		const int sub_q = (int)(second.x >> 32);
		if (pass && nu == 0) break;
		y[0] = y[1] = y[2] = y[3] = -1;
		for (i = 0; i < nv; ++i) {
			for (r = 0; r < 2; ++r) { /* direction */
				const int dir = r << 1 | (int)(v[i].y >> 1 & 1);
				int which, k;
				if (pes[dir].failed) continue;
				which = r << 1 | (int)((v[i].y & 1) ^ 1);
				if (y[which] < 0) continue; /* no earlier hit of that kind */
				for (k = y[which]; k >= 0; --k) {
					int64_t dist;
					int q;
					bmh_pair64_t p;
					if ((int)(v[k].y & 3) != which) continue;
					dist = (int64_t)v[i].x - (int64_t)v[k].x;
					if (dist > pes[dir].high) break;
					if (dist < pes[dir].low) continue;
					q = bmh_pp_d2i((double)((v[i].y >> 32) + (v[k].y >> 32)) + BMH_PP_TERM(t, o, pes, dir, dist) + .499);
					if (q < 0) q = 0;
					p.y = (uint64_t)k << 32 | i;
					if (pass) { /* u[0..n-2] of the sorted vector: every record but the best */
						if (p.y != best.y && sub_q - q <= tmp) ++*n_sub;
						continue;
					}
					/* the reference's mem_pair takes the pair id as an `int` (bwamem_pair.c:177) and shifts it as one */
					p.x = (uint64_t)q << 32 | (bmh_pp_hash_64(p.y ^ (uint64_t)(int64_t)(int32_t)((uint32_t)(int32_t)id << 8)) & 0xffffffffU);
					if (nu == 0 || bmh_pp_lt_pair64(&best, &p)) second = best, best = p;
					else if (nu == 1 || bmh_pp_lt_pair64(&second, &p)) second = p;
					++nu;
				}
			}
			y[v[i].y & 3] = (int)i;
		}
		if (nu < 2) break; /* *sub = 0 and nothing to count */
		*sub = (int)(second.x >> 32);
	}
	if (nu) { /* at least one proper pair */
		const size_t bi = (size_t)(best.y >> 32), bk = (size_t)(best.y << 32 >> 32);
		z[v[bi].y & 1] = (int)(v[bi].y << 32 >> 34); /* index of the best pair */
		z[v[bk].y & 1] = (int)(v[bk].y << 32 >> 34);
		return (int)(best.x >> 32);
	}
	return 0;
}

/* ---- the regions mem_reg2sam_se prints, bwamem.c:1057-1062 (k = 0 first: it is also the `h` of mem_sam_pe's no_pairing): their
 * indices into want_k[0..n), returns how many */
BMH_PP_HD static inline int bmh_pp_want_se(const bmh_sam_opt_t *o, int n, const bmh_alnreg_t *a, int32_t *want_k)
{
	int k, nw = 0;
	for (k = 0; k < n; ++k) {
		const bmh_alnreg_t *p = &a[k];
		if (p->score < o->T) continue;
		if (p->secondary >= 0 && !(o->flag & BMH_MEM_F_ALL)) continue;
		if (p->secondary >= 0 && p->score < a[p->secondary].score * .5) continue;
		if (p->rb < 0 || p->re < 0) continue; /* mem_reg2aln then writes an unmapped record, bwamem.c:1172 */
		want_k[nw++] = k;
	}
	return nw;
}

/* ---- one single-end read: worker2's SE branch (bwamem.c:1285-1289) up to the selection.  reg_mapq, want_k: n entries each */
BMH_PP_HD static inline void bmh_pp_unit_se(const bmh_sam_opt_t *o, const bmh_pp_tab_t *t, int64_t id, int n, bmh_alnreg_t *a, int *z,
                                           bmh_sort_stk_t *stk, int32_t *reg_mapq, int32_t *n_want, int32_t *want_k)
{
	int j;
	bmh_pp_mark(o, n, a, id, z, stk);
	*n_want = bmh_pp_want_se(o, n, a, want_k);
	for (j = 0; j < n; ++j) reg_mapq[j] = bmh_pp_mapq(o, &a[j], t);
}

/* ---- one pair: mem_sam_pe after its rescue block (bwamem_pair.c:264-331) up to the selection.  id is the pair's, the reads' are
 * id<<1|r.  n[r], a[r], z[r] (n[r] ints), reg_mapq[r], want_k[r] (n[r] entries): end r's; v: n[0] + n[1] records; stk for n[0] + n[1]. */
BMH_PP_HD static inline void bmh_pp_unit_pe(const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t *pes, const bmh_pp_tab_t *t, uint64_t id,
                                           const int n[2], bmh_alnreg_t *const a[2], int *const z[2], bmh_pair64_t *v, bmh_sort_stk_t *stk,
                                           bmh_pairdec_t *d, int32_t *const reg_mapq[2], int32_t n_want[2], int32_t *const want_k[2])
{
	BMH_PP_NOCONTRACT
	int sub_o = 0, n_sub = 0, oo = 0, r, j, go_pair = 0;
	bmh_pp_mark(o, n[0], a[0], (int64_t)(id << 1 | 0), z[0], stk);
	bmh_pp_mark(o, n[1], a[1], (int64_t)(id << 1 | 1), z[1], stk);
	d->paired = 0, d->z[0] = d->z[1] = 0, d->q_se[0] = d->q_se[1] = 0, d->extra_flag = 1;
	d->score = d->sub = d->n_sub = d->q_pe = 0, d->rsv[0] = d->rsv[1] = 0;
	if (!(o->flag & BMH_MEM_F_NOPAIRING) && n[0] && n[1]) {
		oo = bmh_pp_pair(o, l_pac, pes, t, n[0], a[0], n[1], a[1], id, &sub_o, &n_sub, d->z, v, stk);
		d->score = oo, d->sub = sub_o, d->n_sub = n_sub;
	}
	if (oo > 0) {
		int is_multi[2], q_pe, score_un;
		for (r = 0; r < 2; ++r) { /* more than one good hit at an end even after rescue? */
			for (j = 1; j < n[r]; ++j)
				if (a[r][j].secondary < 0 && a[r][j].score >= o->T) break;
			is_multi[r] = j < n[r];
		}
		if (!is_multi[0] && !is_multi[1]) {
			go_pair = 1;
			score_un = a[0][0].score + a[1][0].score - o->pen_unpaired;
			sub_o = sub_o > score_un ? sub_o : score_un;
			q_pe = bmh_pp_raw_mapq(oo - sub_o, o->a);
			if (n_sub > 0) q_pe -= bmh_pp_d2i(4.343 * BMH_PP_LOG(t, n_sub + 1) + .499);
			if (q_pe < 0) q_pe = 0;
			if (q_pe > 60) q_pe = 60;
			d->q_pe = q_pe;
			if (oo > score_un) { /* the pair wins */
				bmh_alnreg_t *c[2];
				c[0] = &a[0][d->z[0]], c[1] = &a[1][d->z[1]];
				for (r = 0; r < 2; ++r) {
					if (c[r]->secondary >= 0) c[r]->sub = a[r][c[r]->secondary].score, c[r]->secondary = -2;
					d->q_se[r] = bmh_pp_mapq(o, c[r], t);
				}
				for (r = 0; r < 2; ++r) d->q_se[r] = d->q_se[r] > q_pe ? d->q_se[r] : q_pe < d->q_se[r] + 40 ? q_pe : d->q_se[r] + 40;
				d->extra_flag |= 2;
				for (r = 0; r < 2; ++r) { /* cap at the tandem-repeat score */
					const int cap = bmh_pp_raw_mapq(c[r]->score - c[r]->csub, o->a);
					d->q_se[r] = d->q_se[r] < cap ? d->q_se[r] : cap;
				}
			} else { /* the two best single-end hits win */
				d->z[0] = d->z[1] = 0;
				d->q_se[0] = bmh_pp_mapq(o, &a[0][0], t);
				d->q_se[1] = bmh_pp_mapq(o, &a[1][0], t);
			}
		}
	}
	d->paired = go_pair;
	for (r = 0; r < 2; ++r) {
		if (go_pair) {
			const bmh_alnreg_t *ar = &a[r][d->z[r]];
			n_want[r] = 0;
			if (ar->rb >= 0 && ar->re >= 0) want_k[r][0] = d->z[r], n_want[r] = 1;
		} else n_want[r] = bmh_pp_want_se(o, n[r], a[r], want_k[r]);
		for (j = 0; j < n[r]; ++j) reg_mapq[r][j] = bmh_pp_mapq(o, &a[r][j], t);
	}
}

#endif
