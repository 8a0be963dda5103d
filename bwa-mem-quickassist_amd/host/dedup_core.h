/*
 * dedup_core.h -- mem_sort_and_dedup (reference bwa-0.7.8/bwamem.c:395-436) as ONE text for its two forms: the host routine
 * bmh_sort_and_dedup (host/sam_post.c, gcc) and the device kernel behind bmh_sort_dedup_batch and the chains-to-regions driver
 * (csrc/chain2reg.hip, hipcc, one lane per read).
 *   the two orders      bwamem.c:386-393 (alnreg_slt2: by re; alnreg_slt: score descending, then rb, then qb)
 *   the routine         sort by re, mask the redundant one of two overlapping regions, compact, sort by (score, rb, qb), mask
 *                       identical hits, compact
 * Both sorts are klib's introsort restated exchange for exchange (sort_exact.h): regions with equal re, or equal (score, rb,
 * qb), are common, the loops below treat neighbours asymmetrically, so which of two tied records comes first decides which
 * one survives.  The range stack is the caller's (bmh_sort_stack_len(n) entries); nothing is allocated.  Under hipcc the
 * routine is __host__ __device__ and always inlined; the C subset used is what lets gcc compile the same text.
 *
 * Floating point: the redundancy test multiplies a float by an int64_t converted to float and compares the single-precision
 * product with an int64_t converted to float.  There is no add behind the multiply, so nothing can be contracted into a fused
 * multiply-add, and neither build uses fast-math: IEEE single multiplication and the int64 -> float conversion (round to
 * nearest even) give the same bits on both sides.  Keep the expression as it is: not in double, not in integers.
 */
#ifndef BMH_DEDUP_CORE_H
#define BMH_DEDUP_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bwamem_hip.h"
#include "sort_exact.h"

#ifdef __HIPCC__
#define BMH_DD_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_DD_HD
#endif

/* ---- orders (bwamem.c:386-393).  hipcc takes them as callables the sort inlines, gcc as functions. */
BMH_DD_HD static inline int bmh_dd_lt_re(const void *x, const void *y) { return ((const bmh_alnreg_t *)x)->re < ((const bmh_alnreg_t *)y)->re; }
BMH_DD_HD static inline int bmh_dd_lt_score_pos(const void *x, const void *y)
{
	const bmh_alnreg_t *a = (const bmh_alnreg_t *)x, *b = (const bmh_alnreg_t *)y;
	return a->score > b->score || (a->score == b->score && (a->rb < b->rb || (a->rb == b->rb && a->qb < b->qb)));
}
#ifdef __HIPCC__
struct bmh_dd_lt_re_t {
	BMH_DD_HD int operator()(const void *a, const void *b) const { return bmh_dd_lt_re(a, b); }
};
struct bmh_dd_lt_score_pos_t {
	BMH_DD_HD int operator()(const void *a, const void *b) const { return bmh_dd_lt_score_pos(a, b); }
};
#define BMH_DD_LT_RE bmh_dd_lt_re_t()
#define BMH_DD_LT_SCORE_POS bmh_dd_lt_score_pos_t()
#else
#define BMH_DD_LT_RE bmh_dd_lt_re
#define BMH_DD_LT_SCORE_POS bmh_dd_lt_score_pos
#endif

/* ---- bwamem.c:395-436 over a[0..n); stk: bmh_sort_stack_len(n) entries (unused for n < 3).  Returns the regions kept. */
BMH_DD_HD static inline int bmh_dedup_core(int n, bmh_alnreg_t *a, float mask_level_redun, bmh_sort_stk_t *stk)
{
	int m, i, j;
	if (n <= 1) return n;
	bmh_sort_exact_stk(a, (size_t)n, sizeof(*a), BMH_DD_LT_RE, stk);
	for (i = 1; i < n; ++i) {
		bmh_alnreg_t *p = &a[i];
		if (p->rb >= a[i - 1].re) continue;
		for (j = i - 1; j >= 0 && p->rb < a[j].re; --j) {
			bmh_alnreg_t *q = &a[j];
			int64_t orr, oq, mr, mq;
			if (q->qe == q->qb) continue; /* already excluded */
			orr = q->re - p->rb;                                  /* overlap on the reference */
			oq = q->qb < p->qb ? q->qe - p->qb : p->qe - q->qb;   /* overlap on the query */
			mr = q->re - q->rb < p->re - p->rb ? q->re - q->rb : p->re - p->rb;
			mq = q->qe - q->qb < p->qe - p->qb ? q->qe - q->qb : p->qe - p->qb;
			if (orr > mask_level_redun * mr && oq > mask_level_redun * mq) { /* one of the two is redundant */
				if (p->score < q->score) {
					p->qe = p->qb;
					break;
				} else q->qe = q->qb;
			}
		}
	}
	for (i = 0, m = 0; i < n; ++i)
		if (a[i].qe > a[i].qb) {
			if (m != i) a[m++] = a[i];
			else ++m;
		}
	n = m;
	bmh_sort_exact_stk(a, (size_t)n, sizeof(*a), BMH_DD_LT_SCORE_POS, stk);
	for (i = 1; i < n; ++i) /* identical hits */
		if (a[i].score == a[i - 1].score && a[i].rb == a[i - 1].rb && a[i].qb == a[i - 1].qb) a[i].qe = a[i].qb;
	for (i = 1, m = 1; i < n; ++i)
		if (a[i].qe > a[i].qb) {
			if (m != i) a[m++] = a[i];
			else ++m;
		}
	return m;
}

#endif
