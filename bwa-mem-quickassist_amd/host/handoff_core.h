/*
 * handoff_core.h -- what phase 2 must know of a batch's regions before its first launch, as ONE text for its two forms: the host's
 * walk over the caller's vectors (decide_table_sizes and oriented_cap, csrc/api.hip, also built by gcc for tests/handoff_core_main.c)
 * and table_plan_kernel (csrc/chain2reg.hip, hipcc, one lane per read) over the regions that stay on the device between
 * bmh_reads_sam_device's two phases.
 *   bmh_ho_log_index     the entry of the log table a region's mapQ reads (bmh_pp_mapq): its length where mapQ_coef_len is set and the
 *                        length reaches it, else 0; seedcov without mapQ_coef_len.  Negative = the refusal (log of a negative number)
 *   bmh_ho_oriented_cap  the oriented bytes a region the pass B kernels accept can have: query and reference span, each cut to 0..65535
 *   bmh_ho_read          one read's vector folded into a bmh_ho_plan_t
 *   bmh_ho_merge         two plans into one: the maximum, the sums, the flag
 *   bmh_ho_pair_kmax     the paired-end clause: the square of a pair's region count, for decide_table_sizes' callers with mates
 *   bmh_ho_pair, bmh_ho_pairs, bmh_ho_pairs_merge   the clause folded over a batch of mates: one pair, a slice of a region table, two
 *                        folds into one.  table_plan_kernel (csrc/chain2reg.hip) folds it over the table mate rescue leaves on the device
 *                        (bmh_pairs_sam_device); tests/pairs_plan_core_main.c runs it stand-alone
 * A plan starts as BMH_HO_PLAN_INIT.  Integer arithmetic only, nothing is allocated and no libc is called.  Under hipcc the routines
 * are __host__ __device__ and always inlined.
 */
#ifndef BMH_HANDOFF_CORE_H
#define BMH_HANDOFF_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bwamem_hip.h"
#include "postproc_core.h"

#ifdef __HIPCC__
#define BMH_HO_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_HO_HD
#endif

#define BMH_HO_TAB_MAX ((int64_t)1 << 20) /* entries a decide table may have */

typedef struct bmh_ho_plan {
	int64_t kmax;      /* the largest index of the log table any region asks for, at least 1 */
	int64_t opool_cap; /* sum of bmh_ho_oriented_cap */
	int64_t total;     /* regions */
	int32_t neg;       /* 1: a region asks for a negative index */
	int32_t rsv;
} bmh_ho_plan_t; /* 32 bytes */

#define BMH_HO_PLAN_INIT {1, 0, 0, 0, 0}

BMH_HO_HD static inline int64_t bmh_ho_log_index(const bmh_sam_opt_t *o, const bmh_alnreg_t *a)
{
	if (o->mapQ_coef_len > 0) {
		const int l = bmh_pp_len(a);
		return l < o->mapQ_coef_len ? 0 : (int64_t)l;
	}
	return (int64_t)a->seedcov;
}

BMH_HO_HD static inline int64_t bmh_ho_clamp16(int64_t x) { return x < 0 ? 0 : x > 65535 ? 65535 : x; }

BMH_HO_HD static inline int64_t bmh_ho_oriented_cap(const bmh_alnreg_t *a)
{
	return bmh_ho_clamp16((int64_t)a->qe - a->qb) + bmh_ho_clamp16(a->re - a->rb);
}

/* a[0..nv) is one read's vector.  A region with a negative index sets the flag and adds nothing else to kmax */
BMH_HO_HD static inline void bmh_ho_read(const bmh_sam_opt_t *o, const bmh_alnreg_t *a, int64_t nv, bmh_ho_plan_t *p)
{
	int64_t j;
	for (j = 0; j < nv; ++j) {
		const int64_t idx = bmh_ho_log_index(o, &a[j]), sub = (int64_t)(a[j].sub_n > 0 ? a[j].sub_n : 0) + nv + 1;
		if (idx < 0) p->neg = 1;
		else if (idx > p->kmax) p->kmax = idx;
		if (sub > p->kmax) p->kmax = sub;
		p->opool_cap += bmh_ho_oriented_cap(&a[j]);
	}
	p->total += nv;
}

BMH_HO_HD static inline void bmh_ho_merge(bmh_ho_plan_t *p, const bmh_ho_plan_t *q)
{
	if (q->kmax > p->kmax) p->kmax = q->kmax;
	p->opool_cap += q->opool_cap, p->total += q->total, p->neg |= q->neg;
}

/* mem_pair's n * n over the regions of both mates: past 1024 the square is out of the table anyway (and of int64 at 2^32) */
BMH_HO_HD static inline int64_t bmh_ho_pair_kmax(int64_t n0, int64_t n1)
{
	const int64_t m = n0 + n1;
	return m > 1024 ? BMH_HO_TAB_MAX : m * m + 1;
}

/* The clause folded over a batch: *pk starts as BMH_HO_PAIRS_INIT (no pair seen: the clause adds nothing), a pair raises it to its
 * bmh_ho_pair_kmax, and two folds merge to their maximum -- in any order and grouping.  At most BMH_HO_TAB_MAX + 1: 21 bits. */
#define BMH_HO_PAIRS_INIT 0

BMH_HO_HD static inline void bmh_ho_pair(int64_t n0, int64_t n1, int64_t *pk)
{
	const int64_t v = bmh_ho_pair_kmax(n0, n1);
	if (v > *pk) *pk = v;
}

BMH_HO_HD static inline void bmh_ho_pairs_merge(int64_t *pk, int64_t q)
{
	if (q > *pk) *pk = q;
}

/* read r of n_reads speaks for its pair: it is even and its mate exists.  An odd trailing read has no pair and adds nothing */
BMH_HO_HD static inline int bmh_ho_first_mate(int64_t r, int64_t n_reads) { return !(r & 1) && r + 1 < n_reads; }

/* Reads [r0, r1) of a table whose read r holds roff[r + 1] - roff[r] regions, n_reads in all: every first mate among them folds its
 * pair, whichever slice its mate falls into */
BMH_HO_HD static inline void bmh_ho_pairs(const uint64_t *roff, int64_t r0, int64_t r1, int64_t n_reads, int64_t *pk)
{
	int64_t r;
	for (r = r0; r < r1; ++r)
		if (bmh_ho_first_mate(r, n_reads)) bmh_ho_pair((int64_t)(roff[r + 1] - roff[r]), (int64_t)(roff[r + 2] - roff[r + 1]), pk);
}

#endif
