/*
 * matesw_core.h -- what the two mate-rescue drivers must agree on bit for bit, as ONE text: the host driver bmh_matesw_batch
 * (host/matesw_batch.c, gcc) and the device driver bmh_matesw_device (csrc/matesw.hip, hipcc, one lane per pair).
 *   mem_infer_dir       bwamem_pair.c:23-30
 *   mem_matesw          bwamem_pair.c:109-175: the skip test over the mate's vector (:112-121), the window of an orientation
 *                       (:123-142), the ksw_align2 call (:144-147) as a bmh_sw_task_t, the region of its result (:150-166), the
 *                       score-sorted insert, mem_sort_and_dedup behind every orientation once a call was made (:168)
 *   its caller          the block of mem_sam_pe at bwamem_pair.c:251-263, as a resumable machine per pair: bmh_msw_plan writes down
 *                       the next invocations that need Smith-Waterman as things stand, bmh_msw_fold_step folds one invocation
 *                       against the vector as it is then
 * Plain C, no allocation, no floating point of its own (the redundancy test inside bmh_dedup_core is dedup_core.h's).  Under hipcc
 * every routine is __host__ __device__ and always inlined; the C subset used is what lets gcc compile the same text.
 */
#ifndef BMH_MATESW_CORE_H
#define BMH_MATESW_CORE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bwamem_hip.h"
#include "dedup_core.h"

#ifdef __HIPCC__
#define BMH_MS_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_MS_HD
#endif

enum { BMH_MSW_LOOKAHEAD = 8 }; /* invocations planned per pair and round */
/* plan codes of one orientation */
enum {
	BMH_MSW_NONE = 0,   /* not computed: the orientation was skipped when the invocation was planned */
	BMH_MSW_CALL = 1,   /* a ksw_align2 call; the driver replaces it by index + 1 of the call's result */
	BMH_MSW_EMPTY = -2, /* re == rb: the call counts, scores 0 and inserts nothing (no GPU work) */
	BMH_MSW_NOCALL = -3 /* window inverted or bridging the strands: bns_get_seq hands back nothing, no call (:144) */
};
/* what bmh_msw_fold_step answers */
enum {
	BMH_MSW_FOLDED = 0,      /* one invocation folded, the cursor moved on: call again */
	BMH_MSW_DONE = 1,        /* the pair has no invocation left */
	BMH_MSW_STOP_PLAN = 2,   /* the next invocation that needs Smith-Waterman is beyond this round's plan */
	BMH_MSW_STOP_NEEDED = 3, /* ... is planned, but an orientation skipped then is needed now: planned afresh in the next round */
	BMH_MSW_FULL = 4,        /* the mate's array has no room for what the invocation may insert; nothing was changed */
	BMH_MSW_BAD = 5          /* a plan points past the results (cannot happen) */
};

typedef struct { /* one planned mem_matesw invocation: hit j of end i against the mate !i; 88 bytes */
	int32_t i, j;
	int32_t plan[4]; /* per orientation: a plan code, or > 0: index + 1 of its ksw_align2 result */
	int64_t rb[4], re[4];
} bmh_msw_inv_t;

typedef struct { /* a pair's machine between rounds */
	int32_t i, j; /* next invocation to fold */
	int32_t n;    /* sum of mem_matesw's return values */
	int32_t done;
	int32_t n_inv, rsv;
	bmh_msw_inv_t inv[BMH_MSW_LOOKAHEAD];
} bmh_msw_pair_t;

typedef struct { /* a pair as the routines below see it */
	const bmh_alnreg_t *b[2]; /* per end its candidate hits (:252-257), copied before anything changed ... */
	int32_t nb[2];            /* ... the first min(count, max_matesw) of them (:258-259) */
	bmh_alnreg_t *a[2];       /* the two region vectors, */
	int32_t n[2], cap[2];     /* their lengths (updated by the fold) and the records their arrays hold */
	int32_t l_seq[2];
} bmh_msw_io_t;

typedef struct { /* mem_sort_and_dedup behind an orientation: the caller's function, or fn == NULL: bmh_dedup_core at `level` over stk */
	bmh_dedup_fn fn;
	void *user;
	float level;
	bmh_sort_stk_t *stk; /* bmh_sort_stack_len(cap) entries */
} bmh_msw_dedup_t;

/* mem_infer_dir, bwamem_pair.c:23-30 */
BMH_MS_HD static inline int bmh_msw_infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist)
{
	const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
	const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
	*dist = p2 > b1 ? p2 - b1 : b1 - p2;
	return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

/* bwamem_pair.c:112-121 for a hit at a_rb against the mate's vector ma[0..n); returns how many orientations are skipped (4: the
 * invocation returns 0 at :122) */
BMH_MS_HD static inline int bmh_msw_skip(int64_t l_pac, const bmh_pestat_t pes[4], int64_t a_rb, const bmh_alnreg_t *ma, int32_t n, int skip[4])
{
	int32_t k;
	int r;
	for (r = 0; r < 4; ++r) skip[r] = pes[r].failed ? 1 : 0;
	for (k = 0; k < n; ++k) {
		int64_t dist;
		r = bmh_msw_infer_dir(l_pac, a_rb, ma[k].rb, &dist);
		if (dist >= pes[r].low && dist <= pes[r].high) skip[r] = 1;
	}
	return skip[0] + skip[1] + skip[2] + skip[3];
}

BMH_MS_HD static inline int bmh_msw_is_rev(int r) { return (r >> 1) != (r & 1); }

/* bwamem_pair.c:123-142 for orientation r: the window [*rb, *re) and its plan code.  bns_get_seq hands back re - rb bases unless the
 * interval is inverted or bridges the two strands (bntseq.c:358-375); only then does mem_matesw call ksw_align2 (:144). */
BMH_MS_HD static inline int bmh_msw_window(int64_t l_pac, const bmh_pestat_t *pe, int r, int64_t a_rb, int l_ms, int64_t *rb_, int64_t *re_)
{
	const int is_rev = bmh_msw_is_rev(r), is_larger = !(r >> 1);
	int64_t rb, re;
	if (!is_rev) {
		rb = is_larger ? a_rb + pe->low : a_rb - pe->high;
		re = (is_larger ? a_rb + pe->high : a_rb - pe->low) + l_ms;
	} else {
		rb = (is_larger ? a_rb + pe->low : a_rb - pe->high) - l_ms;
		re = is_larger ? a_rb + pe->high : a_rb - pe->low;
	}
	if (rb < 0) rb = 0;
	if (re > l_pac << 1) re = l_pac << 1;
	*rb_ = rb, *re_ = re;
	if (re == rb) return BMH_MSW_EMPTY;
	return re > rb && (rb >= l_pac || re <= l_pac) ? BMH_MSW_CALL : BMH_MSW_NOCALL;
}

/* the ksw_align2 of a BMH_MSW_CALL (:144-147) against the resident reference: the window as a BMH_F_TPAC target, the mate where
 * it lies in the pool (mate_off), reverse-complemented in place of the copy of :130-133 */
BMH_MS_HD static inline void bmh_msw_task(int a, int min_seed_len, int l_ms, int r, uint64_t mate_off, int64_t rb, int64_t re, bmh_sw_task_t *t)
{
	const int is_rev = bmh_msw_is_rev(r);
	t->q_off = is_rev ? mate_off + (uint64_t)l_ms - 1 : mate_off;
	t->t_off = (uint64_t)rb;
	t->tlen = (uint32_t)(re - rb), t->qlen = (uint16_t)l_ms;
	t->flags = (uint16_t)(BMH_F_TPAC | (is_rev ? BMH_F_QREV | BMH_F_QCOMP : 0));
	t->xtra = BMH_SW_XSUBO | BMH_SW_XSTART | (l_ms * a < 250 ? BMH_SW_XBYTE : 0) | (uint32_t)(min_seed_len * a); /* :147 */
	t->rsv = 0;
}

/* bwamem_pair.c:150-166: the region of a result, every other byte zero.  Returns 0 where the reference makes none. */
BMH_MS_HD static inline int bmh_msw_region(int64_t l_pac, int l_ms, int r, int64_t rb, int min_seed_len, const bmh_sw_result_t *aln, bmh_alnreg_t *b)
{
	const int is_rev = bmh_msw_is_rev(r);
	if (!(aln->score >= min_seed_len && aln->qb >= 0)) return 0;
	memset(b, 0, sizeof(*b));
	b->qb = is_rev ? l_ms - (aln->qe + 1) : aln->qb;
	b->qe = is_rev ? l_ms - aln->qb : aln->qe + 1;
	b->rb = is_rev ? (l_pac << 1) - (rb + aln->te + 1) : rb + aln->tb;
	b->re = is_rev ? (l_pac << 1) - (rb + aln->tb) : rb + aln->te + 1;
	b->score = aln->score, b->csub = aln->score2, b->secondary = -1;
	b->seedcov = (int32_t)((b->re - b->rb < b->qe - b->qb ? b->re - b->rb : b->qe - b->qb) >> 1);
	return 1;
}

/* kv_push and the move of :161-165 in one: b goes in front of the first region that scores less; a holds n + 1 records */
BMH_MS_HD static inline int32_t bmh_msw_insert(bmh_alnreg_t *a, int32_t n, const bmh_alnreg_t *b)
{
	int32_t i, at;
	for (at = 0; at < n; ++at)
		if (a[at].score < b->score) break;
	for (i = n; i > at; --i) a[i] = a[i - 1];
	a[at] = *b;
	return n + 1;
}

/* where the cursor (i, j) comes to rest: on the next candidate hit, or at i == 2 */
BMH_MS_HD static inline void bmh_msw_settle(const bmh_msw_io_t *io, int32_t *i, int32_t *j)
{
	while (*i < 2 && !(*j < io->nb[*i])) ++*i, *j = 0;
}

/* The planning rule: from the pair's cursor on, up to BMH_MSW_LOOKAHEAD invocations that need Smith-Waterman as things stand.  The
 * first of them is planned against exactly the state it will be folded in; the later ones AHEAD, against a vector that earlier
 * folds may still change -- ksw_align2 is pure and its inputs do not depend on that state, so a result computed ahead is THE
 * result, and the fold uses what it then needs.  Writes s->n_inv and s->inv[] (BMH_MSW_CALL where a task is wanted); returns the
 * number of those, *win_bytes (nullable) the sum of their window lengths. */
BMH_MS_HD static inline int bmh_msw_plan(int64_t l_pac, const bmh_pestat_t pes[4], const bmh_msw_io_t *io, bmh_msw_pair_t *s, uint64_t *win_bytes)
{
	int32_t ii = s->i, jj = s->j;
	int want = 0, r;
	uint64_t wb = 0;
	s->n_inv = 0;
	for (;;) {
		bmh_msw_inv_t *e;
		int skip[4], l_ms;
		int64_t a_rb;
		bmh_msw_settle(io, &ii, &jj);
		if (ii >= 2 || s->n_inv >= BMH_MSW_LOOKAHEAD) break;
		a_rb = io->b[ii][jj].rb, l_ms = io->l_seq[!ii];
		if (bmh_msw_skip(l_pac, pes, a_rb, io->a[!ii], io->n[!ii], skip) == 4) { ++jj; continue; } /* :122, returns 0 */
		e = &s->inv[s->n_inv++];
		e->i = ii, e->j = jj;
		for (r = 0; r < 4; ++r) {
			e->plan[r] = BMH_MSW_NONE, e->rb[r] = e->re[r] = 0;
			if (skip[r]) continue;
			e->plan[r] = bmh_msw_window(l_pac, &pes[r], r, a_rb, l_ms, &e->rb[r], &e->re[r]);
			if (e->plan[r] == BMH_MSW_CALL) ++want, wb += (uint64_t)(e->re[r] - e->rb[r]);
		}
		++jj;
	}
	if (win_bytes) *win_bytes = wb;
	return want;
}

/* The fold rule, one invocation per call, in the reference's order (:109-175): skip[] is re-derived against the mate's vector as
 * it is NOW; invocations that return at :122 are passed over; the next one is folded if this round planned it and every
 * orientation it needs now was computed then.  res[0..n_res): the round's ksw_align2 results. */
BMH_MS_HD static inline int bmh_msw_fold_step(int64_t l_pac, const bmh_pestat_t pes[4], int min_seed_len, bmh_msw_io_t *io, bmh_msw_pair_t *s,
                                              const bmh_sw_result_t *res, uint32_t n_res, const bmh_msw_dedup_t *dd)
{
	for (;;) {
		const bmh_msw_inv_t *e = 0;
		bmh_alnreg_t *ma;
		int skip[4], n = 0, l_ms, v, r, m, room = 0;
		int32_t nma;
		bmh_msw_settle(io, &s->i, &s->j);
		if (s->i >= 2) {
			s->done = 1;
			return BMH_MSW_DONE;
		}
		m = !s->i, ma = io->a[m], nma = io->n[m], l_ms = io->l_seq[m];
		if (bmh_msw_skip(l_pac, pes, io->b[s->i][s->j].rb, ma, nma, skip) == 4) { ++s->j; continue; } /* :122, returns 0 */
		for (v = 0; v < s->n_inv; ++v)
			if (s->inv[v].i == s->i && s->inv[v].j == s->j) e = &s->inv[v];
		if (!e) return BMH_MSW_STOP_PLAN;
		for (r = 0; r < 4; ++r) {
			if (skip[r]) continue;
			if (e->plan[r] == BMH_MSW_NONE) return BMH_MSW_STOP_NEEDED; /* (a dedup removed the region that covered it) */
			if (e->plan[r] > 0) {
				if ((uint32_t)e->plan[r] - 1 >= n_res) return BMH_MSW_BAD;
				++room;
			}
		}
		if (room > io->cap[m] - nma) return BMH_MSW_FULL;
		for (r = 0; r < 4; ++r) {
			if (skip[r]) continue;
			if (e->plan[r] > 0) {
				bmh_alnreg_t b;
				if (bmh_msw_region(l_pac, l_ms, r, e->rb[r], min_seed_len, &res[e->plan[r] - 1], &b)) nma = bmh_msw_insert(ma, nma, &b);
				++n;
			} else if (e->plan[r] == BMH_MSW_EMPTY) ++n;
			if (n) { /* :168 */
#ifndef __HIP_DEVICE_COMPILE__
				if (dd->fn) nma = dd->fn(dd->user, nma, ma);
				else
#endif
					nma = bmh_dedup_core(nma, ma, dd->level, dd->stk);
			}
		}
		io->n[m] = nma;
		s->n += n;
		++s->j;
		return BMH_MSW_FOLDED;
	}
}

#endif
