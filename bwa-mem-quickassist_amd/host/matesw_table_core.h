/*
 * matesw_table_core.h -- what mate rescue decides about a pair before its first round, as ONE text for its two forms: the host's walk
 * over the caller's vectors (bmh_matesw_device, csrc/matesw.hip, also built by gcc for tests/matesw_table_core_main.c) and
 * mt_filter_kernel (csrc/matesw.hip, hipcc, one lane per pair) over a flat region table that stays on the device.
 *   bmh_mt_nb       |b[i]|: the candidate hits of one end, bwamem_pair.c:252-259 -- the regions that score within pen_unpaired of the
 *                   vector's first, the first max_matesw of them
 *   bmh_mt_busy     does any mem_matesw invocation of the pair get past bwamem_pair.c:122?  Only such pairs are rescued at all
 *   bmh_mt_cap      the records an active vector's arena slice holds: an invocation inserts at most four regions into the mate's
 *                   vector and de-duplication only shrinks
 *   bmh_mt_refuse   the per-read refusals of an active pair: what validate_sw (csrc/api.hip) would answer each of the read's tasks,
 *                   which depends on the read's length and the parameters only
 *   bmh_mt_pair     all of it for one pair
 * Integer arithmetic only, nothing is allocated and no libc is called.  Under hipcc the routines are __host__ __device__ and always
 * inlined.
 */
#ifndef BMH_MATESW_TABLE_CORE_H
#define BMH_MATESW_TABLE_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bwamem_hip.h"
#include "matesw_core.h"

#ifdef __HIPCC__
#define BMH_MT_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_MT_HD
#endif

/* refusal codes of one read, in the order they are tested */
enum {
	BMH_MT_R_NONE = 0,
	BMH_MT_R_LEN = 1,   /* outside 1..65535 bases */
	BMH_MT_R_SCORE = 2, /* l_seq * max(mat) reaches the 16-bit score range and the wide switch does not take the read */
	BMH_MT_R_GAPS = 3   /* a byte-mode read under gap penalties that wrap in 8 bits */
};

typedef struct bmh_mt_rule { /* what the refusals need of the context */
	int32_t a;           /* the match score: l_seq * a < 250 is byte mode (bwamem_pair.c:147) */
	int32_t max_mat;     /* largest entry of the scoring matrix */
	int32_t score_limit; /* l_seq * max_mat must stay below this */
	int32_t wide_sw;     /* bmh_ctx_set_wide_sw is on: word-mode reads past the limit are taken */
	int32_t wraps;       /* o_del + e_del or o_ins + e_ins past 255 */
	int32_t rsv;
} bmh_mt_rule_t;

typedef struct bmh_mt_pair {
	int32_t nb[2];     /* candidate hits per end */
	int32_t busy;      /* the pair needs rescue */
	int32_t refuse[2]; /* per read, BMH_MT_R_*; BMH_MT_R_NONE for the reads of a pair that is not busy */
	int32_t rsv;
	int64_t cap[2];    /* slice capacities; what they would be if the pair is not busy */
} bmh_mt_pair_t;

BMH_MT_HD static inline int32_t bmh_mt_nb(const bmh_alnreg_t *a, int64_t n, int pen_unpaired, int max_matesw)
{
	const int32_t maxm = max_matesw > 0 ? max_matesw : 0;
	int32_t nb = 0;
	int64_t j;
	for (j = 0; j < n && nb < maxm; ++j) nb += a[j].score >= a[0].score - pen_unpaired;
	return nb;
}

/* v[0..nv) against the mate's vector ma[0..nma): is there a candidate hit of v whose invocation is not over at :122 */
BMH_MT_HD static inline int bmh_mt_busy_end(int64_t l_pac, const bmh_pestat_t pes[4], const bmh_alnreg_t *v, int64_t nv, const bmh_alnreg_t *ma,
                                            int64_t nma, int pen_unpaired, int max_matesw)
{
	int nb = 0, skip[4];
	int64_t j;
	for (j = 0; j < nv; ++j) {
		if (v[j].score < v[0].score - pen_unpaired) continue;
		if (nb++ >= max_matesw) break;
		if (bmh_msw_skip(l_pac, pes, v[j].rb, ma, (int32_t)nma, skip) != 4) return 1;
	}
	return 0;
}

BMH_MT_HD static inline int bmh_mt_busy(int64_t l_pac, const bmh_pestat_t pes[4], const bmh_alnreg_t *a0, int64_t n0, const bmh_alnreg_t *a1, int64_t n1,
                                        int pen_unpaired, int max_matesw)
{
	return bmh_mt_busy_end(l_pac, pes, a0, n0, a1, n1, pen_unpaired, max_matesw) || bmh_mt_busy_end(l_pac, pes, a1, n1, a0, n0, pen_unpaired, max_matesw);
}

BMH_MT_HD static inline int64_t bmh_mt_cap(int64_t n, int32_t nb_mate) { return n + 4 * (int64_t)nb_mate; }

BMH_MT_HD static inline int bmh_mt_refuse(const bmh_mt_rule_t *r, int64_t l_seq)
{
	int xbyte;
	if (l_seq < 1 || l_seq > 65535) return BMH_MT_R_LEN;
	xbyte = l_seq * r->a < 250;
	if (!(r->wide_sw && !xbyte) && l_seq * r->max_mat >= r->score_limit) return BMH_MT_R_SCORE;
	if (xbyte && r->wraps) return BMH_MT_R_GAPS;
	return BMH_MT_R_NONE;
}

/* vectors of at most 2^31 - 1 regions each */
BMH_MT_HD static inline void bmh_mt_pair(int64_t l_pac, const bmh_pestat_t pes[4], const bmh_matesw_opt_t *o, const bmh_mt_rule_t *r, const bmh_alnreg_t *a0,
                                         int64_t n0, const bmh_alnreg_t *a1, int64_t n1, int64_t l_seq0, int64_t l_seq1, bmh_mt_pair_t *out)
{
	out->nb[0] = bmh_mt_nb(a0, n0, o->pen_unpaired, o->max_matesw), out->nb[1] = bmh_mt_nb(a1, n1, o->pen_unpaired, o->max_matesw);
	out->cap[0] = bmh_mt_cap(n0, out->nb[1]), out->cap[1] = bmh_mt_cap(n1, out->nb[0]);
	out->busy = bmh_mt_busy(l_pac, pes, a0, n0, a1, n1, o->pen_unpaired, o->max_matesw);
	out->refuse[0] = out->busy ? bmh_mt_refuse(r, l_seq0) : BMH_MT_R_NONE;
	out->refuse[1] = out->busy ? bmh_mt_refuse(r, l_seq1) : BMH_MT_R_NONE;
	out->rsv = 0;
}

#endif
