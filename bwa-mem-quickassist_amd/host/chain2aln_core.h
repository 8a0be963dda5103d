/*
 * chain2aln_core.h -- the arithmetic of the chains-to-regions driver that must agree bit for bit between its two forms:
 * the host driver (host/chain2aln_batch.c, gcc) and the device driver (csrc/chain2reg.hip, hipcc, one lane per read).
 *   cal_max_gap              reference bwa-0.7.8/bwamem.c:544-551
 *   the chain window         bwamem.c:740-755
 *   mem_chain2aln_short      bwamem.c:504-527, the part before its ksw_align2: does the chain qualify, and for which intervals
 *   the containment test     bwamem.c:769-784 (seed_near_region) and :788-799 (seeds_conflict, has_conflicting_seed)
 *   may_conflict             the driver's own question before a chain's earlier seeds are decided
 *   seedcov                  bwamem.c:870-874
 * A chain is given as its seed array and count, which is what both drivers hold.  Nothing is allocated.  Under hipcc every
 * routine is __host__ __device__ and always inlined; the C subset used is what lets gcc compile the same text.
 *
 * Floating point: cal_max_gap divides a double by an int and adds 1., and the .95 test multiplies an int by a double and
 * compares.  Neither expression holds a multiply followed by an add, so there is nothing a compiler could contract into a
 * fused multiply-add, and neither build uses fast-math: IEEE double division, addition and multiplication give the same
 * bits on both sides.  Keep the expression forms as they are.
 */
#ifndef BMH_CHAIN2ALN_CORE_H
#define BMH_CHAIN2ALN_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bwamem_hip.h"

#ifdef __HIPCC__
#define BMH_C2A_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_C2A_HD
#endif

#define BMH_MEM_SHORT_EXT 50 /* bwamem.c:491-492 */
#define BMH_MEM_SHORT_LEN 200

BMH_C2A_HD static inline int bmh_c2a_imin(int a, int b) { return a < b ? a : b; }
BMH_C2A_HD static inline int bmh_c2a_imax(int a, int b) { return a > b ? a : b; }

/* bwamem.c:544-551 */
BMH_C2A_HD static inline int bmh_c2a_cal_max_gap(const bmh_params_t *p, int qlen)
{
	int l_del = (int)((double)(qlen * p->a - p->o_del) / p->e_del + 1.);
	int l_ins = (int)((double)(qlen * p->a - p->o_ins) / p->e_ins + 1.);
	int l = bmh_c2a_imax(bmh_c2a_imax(l_del, l_ins), 1);
	return bmh_c2a_imin(l, p->w << 1);
}

/* bwamem.c:740-755: the reference window [rmax0, rmax1) of a chain of n >= 1 seeds.  Returns 0, or -1 if it comes out empty-handed
 * (rmax1 < rmax0: seeds outside the doubled coordinate). */
BMH_C2A_HD static inline int bmh_c2a_window(const bmh_params_t *p, int64_t l_pac, int l_query, int n, const bmh_seed_t *seeds,
                                            int64_t *rmax0_, int64_t *rmax1_)
{
	int64_t rmax0 = l_pac << 1, rmax1 = 0;
	int i;
	for (i = 0; i < n; ++i) {
		const bmh_seed_t *t = &seeds[i];
		const int rest = l_query - t->qbeg - t->len;
		const int64_t b = t->rbeg - (t->qbeg + bmh_c2a_cal_max_gap(p, t->qbeg));
		const int64_t e = t->rbeg + t->len + (rest + bmh_c2a_cal_max_gap(p, rest));
		if (b < rmax0) rmax0 = b;
		if (e > rmax1) rmax1 = e;
	}
	if (rmax0 < 0) rmax0 = 0;
	if (rmax1 > l_pac << 1) rmax1 = l_pac << 1;
	if (rmax0 < l_pac && l_pac < rmax1) { /* crossing the forward-reverse boundary: cut at the first seed's strand */
		if (seeds[0].rbeg < l_pac) rmax1 = l_pac;
		else rmax0 = l_pac;
	}
	*rmax0_ = rmax0, *rmax1_ = rmax1;
	return rmax1 < rmax0 ? -1 : 0;
}

typedef struct { /* what mem_chain2aln_short hands to its ksw_align2 and keeps for the verdict */
	int32_t sqb, sqe, seedcov;
	int64_t srb, sre;
} bmh_c2a_short_t;

/* The part of mem_chain2aln_short before its ksw_align2 (bwamem.c:504-527): does the chain qualify, and for which query /
 * reference intervals?  Returns 1 and fills *o if a Smith-Waterman is to be run. */
BMH_C2A_HD static inline int bmh_c2a_short_candidate(const bmh_params_t *p, int64_t l_pac, int l_query, int n, const bmh_seed_t *seeds,
                                                     bmh_c2a_short_t *o)
{
	int i, qb = l_query, qe = 0, cov = 0;
	int64_t rb = l_pac << 1, re = 0;
	if (n <= 0) return 0;
	for (i = 0; i < n; ++i) {
		const bmh_seed_t *s = &seeds[i];
		qb = qb < s->qbeg ? qb : s->qbeg;
		qe = qe > s->qbeg + s->len ? qe : s->qbeg + s->len;
		rb = rb < s->rbeg ? rb : s->rbeg;
		re = re > s->rbeg + s->len ? re : s->rbeg + s->len;
		cov += s->len;
	}
	qb -= BMH_MEM_SHORT_EXT, qe += BMH_MEM_SHORT_EXT;
	if (qb <= 10 || qe >= l_query - 10) return 0; /* ksw_align2 cannot align to the ends */
	rb -= BMH_MEM_SHORT_EXT, re += BMH_MEM_SHORT_EXT;
	rb = rb > 0 ? rb : 0;
	re = re < l_pac << 1 ? re : l_pac << 1;
	if (rb < l_pac && l_pac < re) {
		if (seeds[0].rbeg < l_pac) re = l_pac;
		else rb = l_pac;
	}
	if ((re - rb) - (qe - qb) > BMH_MEM_SHORT_EXT || (qe - qb) - (re - rb) > BMH_MEM_SHORT_EXT) return 0;
	if (qe - qb >= p->w * 4 || re - rb >= p->w * 4) return 0;
	if (qe - qb >= BMH_MEM_SHORT_LEN || re - rb >= BMH_MEM_SHORT_LEN) return 0;
	o->sqb = qb, o->sqe = qe, o->srb = rb, o->sre = re, o->seedcov = cov;
	return 1;
}

/* bwamem.c:769-784 over the n regions the read has so far */
BMH_C2A_HD static inline int bmh_c2a_seed_near_region(const bmh_params_t *p, const bmh_seed_t *s, const bmh_alnreg_t *a, size_t n)
{
	size_t i;
	for (i = 0; i < n; ++i) {
		const bmh_alnreg_t *r = &a[i];
		int64_t rd;
		int qd, w, g;
		if (s->rbeg < r->rb || s->rbeg + s->len > r->re || s->qbeg < r->qb || s->qbeg + s->len > r->qe) continue;
		qd = s->qbeg - r->qb, rd = s->rbeg - r->rb;
		g = bmh_c2a_cal_max_gap(p, qd < rd ? qd : (int)rd);
		w = bmh_c2a_imin(g, p->w);
		if (qd - rd < w && rd - qd < w) return 1;
		qd = r->qe - (s->qbeg + s->len), rd = r->re - (s->rbeg + s->len);
		g = bmh_c2a_cal_max_gap(p, qd < rd ? qd : (int)rd);
		w = bmh_c2a_imin(g, p->w);
		if (qd - rd < w && rd - qd < w) return 1;
	}
	return 0;
}

/* the overlap test of bwamem.c:793-794 */
BMH_C2A_HD static inline int bmh_c2a_seeds_conflict(const bmh_seed_t *s, const bmh_seed_t *t)
{
	if (t->len < s->len * .95) return 0; /* double compare, bwamem.c:792 */
	if (s->qbeg <= t->qbeg && s->qbeg + s->len - t->qbeg >= s->len >> 2 && t->qbeg - s->qbeg != t->rbeg - s->rbeg) return 1;
	if (t->qbeg <= s->qbeg && t->qbeg + t->len - s->qbeg >= s->len >> 2 && s->qbeg - t->qbeg != s->rbeg - t->rbeg) return 1;
	return 0;
}

/* bwamem.c:788-799: does another, not-skipped, long-enough seed overlap s off-diagonal?  srt: the chain's (len, index) keys in
 * ascending order, 0 where a seed was skipped; k: the position of s in it */
BMH_C2A_HD static inline int bmh_c2a_has_conflicting_seed(const bmh_seed_t *seeds, int n, const uint64_t *srt, int k, const bmh_seed_t *s)
{
	int i;
	for (i = k + 1; i < n; ++i) {
		if (srt[i] == 0) continue;
		if (bmh_c2a_seeds_conflict(s, &seeds[(uint32_t)srt[i]])) return 1;
	}
	return 0;
}

/* the same question asked BEFORE the chain's earlier seeds have been decided: every seed that sorts after `si`
 * (longer, or as long with a larger index) counts, skipped or not -- a superset of the conflicts the reference will see */
BMH_C2A_HD static inline int bmh_c2a_may_conflict(const bmh_seed_t *seeds, int n, int si)
{
	const bmh_seed_t *s = &seeds[si];
	const uint64_t key = (uint64_t)s->len << 32 | (uint32_t)si;
	int i;
	for (i = 0; i < n; ++i) {
		const uint64_t ki = (uint64_t)seeds[i].len << 32 | (uint32_t)i;
		if (ki <= key || ki == 0) continue;
		if (bmh_c2a_seeds_conflict(s, &seeds[i])) return 1;
	}
	return 0;
}

/* bwamem.c:870-874: the summed length of the chain's seeds that lie inside the region */
BMH_C2A_HD static inline int bmh_c2a_seedcov(const bmh_seed_t *seeds, int n, const bmh_alnreg_t *a)
{
	int i, cov = 0;
	for (i = 0; i < n; ++i) {
		const bmh_seed_t *t = &seeds[i];
		if (t->qbeg >= a->qb && t->qbeg + t->len <= a->qe && t->rbeg >= a->rb && t->rbeg + t->len <= a->re) cov += t->len;
	}
	return cov;
}

#endif
