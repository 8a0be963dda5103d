/*
 * glbband_core.h -- the band a ksw_global2 task (reference bwa-0.7.8/ksw.c:501-584) needs for its result, as ONE text for the
 * device (csrc/global_kernel.hip, hipcc: the first pass of the global dispatcher's sort) and for a C test program
 * (tests/glbband_core_main.c, gcc).  DESIGN.md §4.6 has the argument; in short:
 *
 *   LB     the score of the best path with at most one gap, of length |qlen - tlen|, taken over every place the gap can stand.
 *          That path stays between the diagonals 0 and qlen - tlen, so it exists in every band w' >= |qlen - tlen|, and the
 *          optimum of the full band and of every such narrower band is at least LB.
 *   UB(d)  no path that touches a diagonal d past both end points can score more: it holds at least d inserted (deleted) bases
 *          and, to come back, d - delta deleted (d + delta inserted) ones, at least one gap of either kind, and at most
 *          qlen - d (tlen - d) aligned pairs of at most A = max(mat) each.  UB falls as d grows.
 *   w_eff  the smallest w' in [|delta|, w] with UB+(w'+1) < LB and UB-(w'+1) < LB, else w.  STRICTLY less: every path of the
 *          full band that leaves the band w_eff is then worse than one inside it, so the optimum, and the traceback's every
 *          comparison (ties included), are those of the full band.
 *
 * The rule leaves w alone when w < |delta| (the reference's result is then the band's doing), when a sequence is empty, when
 * A <= 0 (fewer pairs would not mean a lower bound) and when a gap cost is negative.
 * mat is the 5 x 5 matrix, s(x, y) = mat[x * 5 + y] with x the target's base code and y the query's (ksw.c:514-517); codes
 * above 4 are read as 4.  Plain C, no allocation; under hipcc __host__ __device__ and always inlined.
 */
#ifndef BMH_GLBBAND_CORE_H
#define BMH_GLBBAND_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define BMH_GB_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_GB_HD
#endif

BMH_GB_HD static inline int bmh_gb_code(int b) { return b > 4 ? 4 : b; }

/* the largest entry of mat[25] */
BMH_GB_HD static inline int bmh_glbband_amax(const int8_t *mat)
{
	int k, a = mat[0];
	for (k = 1; k < 25; ++k) a = mat[k] > a ? mat[k] : a;
	return a;
}

BMH_GB_HD static inline uint64_t bmh_gb_ld8(const uint8_t *p) /* eight bases with one (unaligned) load; little endian on both sides */
{
	uint64_t v;
	__builtin_memcpy(&v, p, 8);
	return v;
}

/* LB: one forward pass.  With n = min(qlen, tlen) pairs and the gap in front of pair x, the score is
 *   sum_{p<x} s0(p) + sum_{p>=x} s1(p) - gap  =  sum_p s1(p) + max over x of sum_{p<x} (s0(p) - s1(p)) - gap,
 * s0(p) the pair on the main diagonal, s(t[p], q[p]), and s1(p) the pair on the diagonal of the far corner: s(t[p], q[p + delta])
 * behind an insertion (delta > 0), s(t[p - delta], q[p]) behind a deletion.  The running sum of s0 - s1 and its maximum over
 * x = 0..n give the best place.  Equal lengths: s0 = s1, no gap, one sum.
 * The pass is cut into parts that are joined in order, so that several lanes can share one task (the device gives a task to eight
 * lanes: their loads then fall into the same few cache lines at the same time); the host walks one part. */
typedef struct {
	const uint8_t *t0, *q0, *t1, *q1; /* pair p of s0 is (t0[p], q0[p]), of s1 (t1[p], q1[p]) */
	int n, two, gap;                  /* pairs; s0 != s1 (delta != 0); the gap's cost */
} bmh_gb_walk_t;
typedef struct {
	int s1, d, b; /* over the part's pairs: sum of s1, sum of s0 - s1, and the largest sum of s0 - s1 over a (possibly empty) prefix */
} bmh_gb_part_t;

BMH_GB_HD static inline bmh_gb_walk_t bmh_glbband_walk(int o_del, int e_del, int o_ins, int e_ins, const uint8_t *q, int qlen, const uint8_t *t,
                                                       int tlen)
{
	const int delta = qlen - tlen;
	bmh_gb_walk_t w;
	w.t0 = t, w.q0 = q, w.t1 = delta < 0 ? t - delta : t, w.q1 = delta > 0 ? q + delta : q;
	w.n = delta > 0 ? tlen : qlen, w.two = delta != 0;
	w.gap = delta > 0 ? o_ins + e_ins * delta : delta < 0 ? o_del + e_del * -delta : 0;
	return w;
}

BMH_GB_HD static inline bmh_gb_part_t bmh_glbband_part(const int8_t *mat, const bmh_gb_walk_t *w, int from, int to) /* pairs [from, to) */
{
	bmh_gb_part_t r;
	int p = from, k, s1 = 0, run = 0, best = 0;
	for (; p + 8 <= to; p += 8) {
		const uint64_t a1 = bmh_gb_ld8(w->t1 + p), b1 = bmh_gb_ld8(w->q1 + p);
		uint64_t a0 = 0, b0 = 0;
		if (w->two) a0 = bmh_gb_ld8(w->t0 + p), b0 = bmh_gb_ld8(w->q0 + p);
		for (k = 0; k < 8; ++k) {
			const int v1 = mat[bmh_gb_code((int)(a1 >> (8 * k) & 255)) * 5 + bmh_gb_code((int)(b1 >> (8 * k) & 255))];
			s1 += v1;
			if (w->two) {
				run += mat[bmh_gb_code((int)(a0 >> (8 * k) & 255)) * 5 + bmh_gb_code((int)(b0 >> (8 * k) & 255))] - v1;
				best = run > best ? run : best;
			}
		}
	}
	for (; p < to; ++p) {
		const int v1 = mat[bmh_gb_code(w->t1[p]) * 5 + bmh_gb_code(w->q1[p])];
		s1 += v1;
		if (w->two) {
			run += mat[bmh_gb_code(w->t0[p]) * 5 + bmh_gb_code(w->q0[p])] - v1;
			best = run > best ? run : best;
		}
	}
	r.s1 = s1, r.d = run, r.b = best;
	return r;
}

/* acc holds the pairs in front of nx's: acc <- both */
BMH_GB_HD static inline void bmh_glbband_join(bmh_gb_part_t *acc, const bmh_gb_part_t *nx)
{
	acc->b = acc->d + nx->b > acc->b ? acc->d + nx->b : acc->b;
	acc->d += nx->d, acc->s1 += nx->s1;
}

BMH_GB_HD static inline int bmh_glbband_lb(const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins, const uint8_t *q, int qlen,
                                           const uint8_t *t, int tlen)
{
	const bmh_gb_walk_t w = bmh_glbband_walk(o_del, e_del, o_ins, e_ins, q, qlen, t, tlen);
	const bmh_gb_part_t r = bmh_glbband_part(mat, &w, 0, w.n);
	return r.s1 + r.b - w.gap;
}

/* the smallest w' >= |delta| whose outside is strictly worse than LB, from the lower bound and the lengths alone
 *   UB+(d) = A (qlen - d)         - (o_ins + e_ins d)           - (o_del + e_del (d - delta)) < LB
 *   UB-(d) = A (qlen - d - delta) - (o_ins + e_ins (d + delta)) - (o_del + e_del d)           < LB
 * both read K d > X with K = A + e_ins + e_del > 0: the smallest such d is floor(X / K) + 1, so w' = d - 1 >= floor(X / K);
 * X < 0 asks nothing beyond |delta|. */
BMH_GB_HD static inline int bmh_glbband_from_lb(int amax, int o_del, int e_del, int o_ins, int e_ins, int qlen, int tlen, int w, int lb)
{
	const int delta = qlen - tlen, ad = delta < 0 ? -delta : delta;
	const long long K = (long long)amax + e_ins + e_del; /* (64 bits: the reference's own terms o + e * len fit an int, their sums here need not) */
	const long long xp = (long long)amax * qlen - o_ins - o_del + (long long)e_del * delta - lb;
	const long long xm = (long long)amax * tlen - o_ins - o_del - (long long)e_ins * delta - lb;
	long long need = ad;
	if (xp >= 0 && xp / K > need) need = xp / K;
	if (xm >= 0 && xm / K > need) need = xm / K;
	return need < w ? (int)need : w;
}

/* the scoring's part of "does the rule apply", the same for a whole batch; the lengths' and w's part is per task (bmh_glbband_weff) */
BMH_GB_HD static inline int bmh_glbband_applies(int amax, int o_del, int e_del, int o_ins, int e_ins)
{
	return amax > 0 && o_del >= 0 && e_del >= 0 && o_ins >= 0 && e_ins >= 0;
}

BMH_GB_HD static inline int bmh_glbband_weff(const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins, const uint8_t *q, int qlen,
                                             const uint8_t *t, int tlen, int w)
{
	const int delta = qlen - tlen, ad = delta < 0 ? -delta : delta;
	const int amax = bmh_glbband_amax(mat);
	if (w < ad || qlen < 1 || tlen < 1 || !bmh_glbband_applies(amax, o_del, e_del, o_ins, e_ins)) return w;
	return bmh_glbband_from_lb(amax, o_del, e_del, o_ins, e_ins, qlen, tlen, w,
	                           bmh_glbband_lb(mat, o_del, e_del, o_ins, e_ins, q, qlen, t, tlen));
}

#endif
