/*
 * extband_core.h -- the band a ksw_extend2 flank (reference bwa-0.7.8/ksw.c:379-476) needs for its six outputs, as ONE text for the
 * device (csrc/extend_dispatch.hip, hipcc: the band pass in front of the extension dispatcher's sort) and for a C test program
 * (tests/extband_core_main.c, gcc).  DESIGN.md §4.3 has the argument; in short, with A = max(mat), s(x, y) = mat[x * 5 + y], h0
 * floored at 0 and the plain diagonal of the flank, pairs p = 0 .. qlen-1 (needs tlen >= qlen):
 *
 *   P(p)      = h0 + sum_{k<=p} s(t[k], q[k]), P(-1) = h0         the diagonal's score behind pair p
 *   pen_total = A qlen - sum_{k<qlen} s(t[k], q[k])               what the whole diagonal loses against qlen best matches
 *   G(w')     = min(o_ins + e_ins (w'+1), o_del + e_del (w'+1))   the cheapest gap that leaves the band w'
 *   T(w')     = max(o_ins + e_ins w', o_del + e_del w'), T(0) = 0 the dearest single gap inside it
 *
 *   w_eff = the smallest w' in [0, w) with
 *     (2) G(w') > pen_total                 whatever touches a diagonal past +-w' stays strictly below the plain diagonal, in every row
 *                                           and in what it can still reach at the query's end;
 *     (3) h0 >= G(w')                       0.7.8 adds a score to a zero H without a zero test (ksw.c:430), so paths restart from zero
 *                                           cells: a restart is then as low as a cell outside the band;
 *     (4) min_{-1<=p<qlen} P(p) > T(w')     every cell inside the band is positive in the full run and in the narrow one, so neither
 *                                           run's zero scan (ksw.c:463-466) closes the interval inside the band;
 *     (5) zdrop <= 0, or pen_total + max(o_ins + e_ins (w'+1), o_del + e_del (w'+1)) <= zdrop
 *                                           neither run z-drops while the band is on the query: both reach row qlen-1;
 *   else w.  (1): the task is left alone unless A >= 0, the four gap costs are >= 0 and tlen >= qlen >= 1.
 *
 * (2) gets easier as w' grows, (3)-(5) harder, so the smallest w' that meets (2) is the only candidate.  w is the band as the task
 * carries it: the reference's own clamps (ksw.c:398-406) only lower it, a consumer takes min(clamped w, w_eff), and a w' at or above
 * the clamped band changes nothing.
 *
 * The walk is cut into parts that are joined in order, so that several lanes can share one task.  Plain C, no allocation; under
 * hipcc __host__ __device__ and always inlined.
 */
#ifndef BMH_EXTBAND_CORE_H
#define BMH_EXTBAND_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define BMH_XB_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_XB_HD
#endif

/* the largest entry of mat[25] */
BMH_XB_HD static inline int bmh_extband_amax(const int8_t *mat)
{
	int k, a = mat[0];
	for (k = 1; k < 25; ++k) a = mat[k] > a ? mat[k] : a;
	return a;
}

/* the scoring's part of (1), the same for a whole batch */
BMH_XB_HD static inline int bmh_extband_applies(int amax, int o_del, int e_del, int o_ins, int e_ins)
{
	return amax >= 0 && o_del >= 0 && e_del >= 0 && o_ins >= 0 && e_ins >= 0;
}

typedef struct {
	int sum, mn; /* over the part's pairs: the sum of s, and the smallest sum of s over a (possibly empty) prefix */
} bmh_xb_part_t;

/* one more pair behind the part's */
BMH_XB_HD static inline void bmh_extband_pair(bmh_xb_part_t *r, int s)
{
	r->sum += s;
	r->mn = r->sum < r->mn ? r->sum : r->mn;
}

/* acc holds the pairs in front of nx's: acc <- both */
BMH_XB_HD static inline void bmh_extband_join(bmh_xb_part_t *acc, const bmh_xb_part_t *nx)
{
	acc->mn = acc->sum + nx->mn < acc->mn ? acc->sum + nx->mn : acc->mn;
	acc->sum += nx->sum;
}

/* the smallest k >= 0 with o + e (k+1) > pen, or -1 if there is none (e == 0 and o <= pen) */
BMH_XB_HD static inline int bmh_xb_need(int o, int e, int pen)
{
	if (pen < o) return 0;
	return e > 0 ? (pen - o) / e : -1;
}

/* w_eff from the walk over all qlen pairs: sum and mn as in bmh_xb_part_t.  The scoring must pass bmh_extband_applies. */
BMH_XB_HD static inline int bmh_extband_from_walk(int amax, int o_del, int e_del, int o_ins, int e_ins, int zdrop, int qlen, int tlen, int h0,
                                                  int w, int sum, int mn)
{
	int pen, ki, kd, k, g_ins, g_del, G, X, T;
	if (qlen < 1 || tlen < qlen || w < 1) return w;
	if (h0 < 0) h0 = 0;
	pen = amax * qlen - sum;
	ki = bmh_xb_need(o_ins, e_ins, pen), kd = bmh_xb_need(o_del, e_del, pen);
	if (ki < 0 || kd < 0) return w;
	k = ki > kd ? ki : kd; /* (2) */
	if (k >= w) return w;
	g_ins = o_ins + e_ins * (k + 1), g_del = o_del + e_del * (k + 1);
	G = g_ins < g_del ? g_ins : g_del, X = g_ins > g_del ? g_ins : g_del;
	T = k < 1 ? 0 : (g_ins - e_ins > g_del - e_del ? g_ins - e_ins : g_del - e_del);
	if (h0 < G) return w;                     /* (3) */
	if (h0 + mn <= T) return w;               /* (4) */
	if (zdrop > 0 && pen + X > zdrop) return w; /* (5) */
	return k;
}

BMH_XB_HD static inline int bmh_xb_code(int b) { return b > 4 ? 4 : b; }

/* the whole rule for one task on the host: q and t point at base 0 and run upwards */
BMH_XB_HD static inline int bmh_extband_weff(const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins, int zdrop, const uint8_t *q, int qlen,
                                             const uint8_t *t, int tlen, int h0, int w)
{
	const int amax = bmh_extband_amax(mat);
	bmh_xb_part_t r = {0, 0};
	int p;
	if (!bmh_extband_applies(amax, o_del, e_del, o_ins, e_ins) || qlen < 1 || tlen < qlen) return w;
	for (p = 0; p < qlen; ++p) bmh_extband_pair(&r, mat[bmh_xb_code(t[p]) * 5 + bmh_xb_code(q[p])]);
	return bmh_extband_from_walk(amax, o_del, e_del, o_ins, e_ins, zdrop, qlen, tlen, h0, w, r.sum, r.mn);
}

/* the byte a launch carries per task: 255 stands for "255 or wider", which leaves the task's own band alone */
BMH_XB_HD static inline int bmh_extband_byte(int w_eff) { return w_eff < 0 || w_eff > 254 ? 255 : w_eff; }

/* the sort's class of a band (3 bits): <= 1, 3, 5, 7, 11, 15, 23, wider */
BMH_XB_HD static inline int bmh_extband_class(int b)
{
	return b <= 1 ? 0 : b <= 3 ? 1 : b <= 5 ? 2 : b <= 7 ? 3 : b <= 11 ? 4 : b <= 15 ? 5 : b <= 23 ? 6 : 7;
}

#endif
