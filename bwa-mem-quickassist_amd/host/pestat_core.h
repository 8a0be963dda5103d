/*
 * pestat_core.h -- the pair walk of mem_pestat (reference bwa-0.7.8/bwamem_pair.c:46-62) as ONE text for its two forms: the host
 * routines bmh_pestat / bmh_pestat_candidates (host/sam_post.c, gcc) and pestat_collect_kernel (csrc/pestat.hip, hipcc, one lane per
 * pair) behind bmh_pestat_device and the chains-to-regions calls.
 *   bmh_ps_sub          cal_sub (bwamem_pair.c:32-44): the score of the first other region that overlaps the head region by
 *                       mask_level of the shorter one, else min_seed_len * a
 *   bmh_ps_candidate    the tests of :58-62 in their order; the answer is one word: 0 = no candidate, else dir << 30 | is
 *   bmh_ps_is_exact     the test of mem_test_and_remove_exact (bwamem.c:438-443); the move is the caller's, who owns the slice
 * What mem_pestat does with the candidates (the sort, the percentiles, the ordered sums) is bmh_pestat_from_candidates, host only.
 * Nothing is allocated and no libc is called.  Under hipcc the routines are __host__ __device__ and always inlined.
 *
 * Floating point: cal_sub compares an int with the single-precision product of an int converted to float and mask_level.  One
 * multiply and no add behind it, so nothing can be contracted, and neither build uses fast-math: the bits are the same on both
 * sides.  MIN_RATIO * score is a double product compared with an int converted to double, again one multiply.  Keep both
 * expressions as they are.
 *
 * The word needs max_ins < 2^30 (bit 30 and 31 carry the orientation): BMH_PS_MAX_INS.  The callers that hand words on refuse a
 * larger value with BMH_E_RANGE; bmh_pestat, which keeps its candidates as 64-bit values, does not need it.
 */
#ifndef BMH_PESTAT_CORE_H
#define BMH_PESTAT_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bwamem_hip.h"
#include "postproc_core.h"

#ifdef __HIPCC__
#define BMH_PS_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_PS_HD
#endif

#define BMH_PS_MIN_RATIO 0.8 /* MIN_RATIO, bwamem_pair.c:14 */
#define BMH_PS_MAX_INS ((1 << 30) - 1)
#define BMH_PS_DIR(w) ((int)((w) >> 30))
#define BMH_PS_IS(w) ((int64_t)((w) & 0x3fffffffu))

/* ---- bwamem_pair.c:32-44 over a[0..n), n >= 1 */
BMH_PS_HD static inline int bmh_ps_sub(const bmh_sam_opt_t *o, const bmh_alnreg_t *a, size_t n)
{
	size_t j;
	for (j = 1; j < n; ++j) {
		const int b_max = bmh_pp_imax(a[j].qb, a[0].qb), e_min = bmh_pp_imin(a[j].qe, a[0].qe);
		if (e_min > b_max) {
			const int min_l = bmh_pp_imin(a[j].qe - a[j].qb, a[0].qe - a[0].qb);
			if (e_min - b_max >= min_l * o->mask_level) break;
		}
	}
	return j < n ? a[j].score : o->min_seed_len * o->a;
}

/* ---- bwamem_pair.c:58-62 (and :69-70) for the pair of vectors a0[0..n0), a1[0..n1) */
/* the orientation 0..3 and *is in 1..max_ins, or -1 for no candidate (any max_ins) */
BMH_PS_HD static inline int bmh_ps_pair(const bmh_sam_opt_t *o, int64_t l_pac, const bmh_alnreg_t *a0, size_t n0, const bmh_alnreg_t *a1, size_t n1, int64_t *is)
{
	int dir;
	if (n0 == 0 || n1 == 0) return -1;
	if (bmh_ps_sub(o, a0, n0) > BMH_PS_MIN_RATIO * a0[0].score) return -1;
	if (bmh_ps_sub(o, a1, n1) > BMH_PS_MIN_RATIO * a1[0].score) return -1;
	dir = bmh_pp_infer_dir(l_pac, a0[0].rb, a1[0].rb, is);
	return *is && *is <= o->max_ins ? dir : -1;
}
/* the same as a word; o->max_ins <= BMH_PS_MAX_INS is the caller's to check */
BMH_PS_HD static inline uint32_t bmh_ps_candidate(const bmh_sam_opt_t *o, int64_t l_pac, const bmh_alnreg_t *a0, size_t n0, const bmh_alnreg_t *a1, size_t n1)
{
	int64_t is = 0;
	const int dir = bmh_ps_pair(o, l_pac, a0, n0, a1, n1, &is);
	return dir < 0 ? 0 : (uint32_t)dir << 30 | (uint32_t)is;
}

/* ---- bwamem.c:438-443 with MEM_F_NO_EXACT set: 1 if the head region of a[0..n) is the read's exact match (the caller then moves
 * a[1..n) down by one and decrements its count) */
BMH_PS_HD static inline int bmh_ps_is_exact(const bmh_alnreg_t *a, size_t n, int l_seq, int match) { return n != 0 && a[0].truesc == l_seq * match; }

#endif
