/*
 * regplan_core.h -- what pass B of phase 2 decides WITHOUT reading a sequence byte, as ONE text for its two forms: the host
 * routines of host/sam_post.c and host/reg2cigar_batch.c (gcc) and the planning kernels behind bmh_wanted_cigar_device
 * (csrc/wanted.hip, hipcc, one lane per wanted region).
 *   bmh_rp_pos2rid     bns_pos2rid             reference bwa-0.7.8/bntseq.c:316-330
 *   bmh_rp_xref_test   bwa_fix_xref2's test    bwa.c:184-197 (strand bridge, fm, cb, ce, is a fix needed, the clamped cb / ce)
 *   bmh_rp_xref_cut    its walk and verdict    bwa.c:199-218, :221
 *   bmh_rp_infer_bw    infer_bw                bwamem.c:884-891
 *   bmh_rp_first_band  mem_reg2aln's band      bwamem.c:1187-1191, or reg_w for bwa_fix_xref2's single call (bwa.c:198)
 *   bmh_rp_try_band    bwa_gen_cigar2's band   bwa.c:116-125
 *   bmh_rp_plan/_emit  one region's record and tasks as bmh_region_cigar_batch takes them
 * Nothing is allocated.  Under hipcc every routine is __host__ __device__ and always inlined; the C subset used is what lets gcc
 * compile the same text.
 *
 * Floating point, as postproc_core.h's head comment lays down: the three (int)((double)x / r + c) go through bmh_pp_d2i, the
 * routines that hold them carry BMH_PP_NOCONTRACT (a division and an addition: nothing to fuse, but the rule is one), and the
 * division is correctly rounded on both sides.
 *
 * Integers: the reference computes l * a - score in int.  Here every such expression is the reference's for coordinates up to
 * 65535 and scores the extension kernels can give; (q + r - a) << 1 is written * 2 (the same value, defined when negative), a
 * band shifted by the try number saturates at INT32_MAX instead of overflowing (it only ever feeds a minimum with a value below
 * 2^17), and the single-try case takes reg_w BEFORE any arithmetic touches truesc == INT32_MIN.
 */
#ifndef BMH_REGPLAN_CORE_H
#define BMH_REGPLAN_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bwamem_hip.h"
#include "postproc_core.h"

#define BMH_RP_HD BMH_PP_HD
#define BMH_RP_SMALL_CAP 24 /* CIGAR slots reserved per task on the first attempt of a try */
/* MD bytes bmh_wanted_cigar_device brings back per region, one 128-byte line each (bmh_reg2cigar_batch keeps its 96: what a 150 bp mate
 * with 12 % substitutions needs is ~55, but a mate that only rescue could place reaches 105 in tests/test_11_wanted_device_sam.py's
 * paired-end input, and every region past the slot is a second trip through the host form).  BMH_WANTED_HOST names the regions past
 * it in both forms. */
#define BMH_RP_MD_SLOT 128

/* the reference sequences as (offset, len) records `stride` bytes apart: bmh_refann_t on the host, bmh_refspan_t on the device */
typedef struct bmh_refspan { int64_t offset; int32_t len, rsv_; } bmh_refspan_t; /* 16 bytes */
typedef struct bmh_rp_refv {
	const void *off0, *len0; /* the first record's int64 offset and int32 len */
	size_t stride;
	int32_t n_seqs;
	int64_t l_pac;
} bmh_rp_refv_t;
BMH_RP_HD static inline int64_t bmh_rp_ref_off(const bmh_rp_refv_t *v, int i) { return *(const int64_t *)((const char *)v->off0 + (size_t)i * v->stride); }
BMH_RP_HD static inline int32_t bmh_rp_ref_len(const bmh_rp_refv_t *v, int i) { return *(const int32_t *)((const char *)v->len0 + (size_t)i * v->stride); }

/* the scoring fields the bands read */
typedef struct bmh_rp_opt { int32_t a, mat0, o_del, e_del, o_ins, e_ins, w; } bmh_rp_opt_t;

/* ---- bntseq.c:316-330; the same result as the reference for every pos_f in [0, l_pac), -1 past it */
BMH_RP_HD static inline int bmh_rp_pos2rid(const bmh_rp_refv_t *v, int64_t pos_f)
{
	int left = 0, mid = 0, right = v->n_seqs;
	if (pos_f >= v->l_pac) return -1;
	while (left < right) {
		mid = (left + right) >> 1;
		if (pos_f >= bmh_rp_ref_off(v, mid)) {
			if (mid == v->n_seqs - 1) break;
			if (pos_f < bmh_rp_ref_off(v, mid + 1)) break;
			left = mid + 1;
		} else right = mid;
	}
	return mid;
}

/* ---- bwa.c:184-197.  -1: the region bridges the strands (the reference gives up on the run, bwamem.c:1183-1186); 0: it lies inside
 * its reference sequence; 1: it hangs over an end and has to be cut to [*cb, *ce), already clamped to the region. */
BMH_RP_HD static inline int bmh_rp_xref_test(const bmh_rp_refv_t *v, int64_t rb, int64_t re, int64_t *cb_, int64_t *ce_)
{
	const int64_t l_pac = v->l_pac;
	int64_t fm, cb, ce;
	int is_rev, rid;
	if (rb < l_pac && re > l_pac) return -1;
	fm = (rb + re) >> 1;
	is_rev = fm >= l_pac; /* bns_depos, bntseq.h:83-86 */
	if (is_rev) fm = (l_pac << 1) - 1 - fm;
	rid = bmh_rp_pos2rid(v, fm);
	if (rid < 0) rid = 0; /* (fm < 0: coordinates the callers refuse before they get here) */
	cb = is_rev ? (l_pac << 1) - (bmh_rp_ref_off(v, rid) + bmh_rp_ref_len(v, rid)) : bmh_rp_ref_off(v, rid); /* its sequence, on the mapping strand */
	ce = cb + bmh_rp_ref_len(v, rid);
	if (!(cb > rb || ce < re)) return 0;
	*cb_ = cb > rb ? cb : rb, *ce_ = ce < re ? ce : re;
	return 1;
}

/* ---- bwa.c:199-218 over the one-try CIGAR of the region, then the verdict of :221: 0, or -2 when nothing is left of it */
BMH_RP_HD static inline int bmh_rp_xref_cut(int n_cigar, const uint32_t *cigar, int64_t cb, int64_t ce, int32_t *qb, int32_t *qe, int64_t *rb,
                                            int64_t *re)
{
	int64_t x = *rb;
	int k, y = *qb;
	for (k = 0; k < n_cigar; ++k) {
		const int op = (int)(cigar[k] & 0xf), len = (int)(cigar[k] >> 4);
		if (op == 0) {
			if (x <= cb && cb < x + len) *qb = y + (int)(cb - x), *rb = cb;
			if (x < ce && ce <= x + len) {
				*qe = y + (int)(ce - x), *re = ce;
				break;
			} else x += len, y += len;
		} else if (op == 1) y += len;
		else if (op == 2) {
			if (x <= cb && cb < x + len) *qb = y, *rb = x + len;
			if (x < ce && ce <= x + len) {
				*qe = y, *re = x;
				break;
			} else x += len;
		}
	}
	return *qb == *qe || *rb == *re ? -2 : 0;
}

BMH_RP_HD static inline int bmh_rp_iabs(int x) { return x < 0 ? -x : x; }

/* ---- bwamem.c:884-891 */
BMH_RP_HD static inline int bmh_rp_infer_bw(int l1, int l2, int score, int a, int q, int r)
{
	BMH_PP_NOCONTRACT
	int w;
	if (l1 == l2 && l1 * a - score < (q + r - a) * 2) return 0;
	w = bmh_pp_d2i((double)((l1 < l2 ? l1 : l2) * a - score - q) / r + 2.);
	if (w < bmh_rp_iabs(l1 - l2)) w = bmh_rp_iabs(l1 - l2);
	return w;
}

/* ---- the band mem_reg2aln starts with (bwamem.c:1187-1191), or reg_w for bwa_fix_xref2's single call (bwa.c:198) */
BMH_RP_HD static inline int bmh_rp_first_band(const bmh_rp_opt_t *o, int ql, int tl, int truesc, int reg_w)
{
	int tmp, w2;
	if (truesc == INT32_MIN) return reg_w;
	tmp = bmh_rp_infer_bw(ql, tl, truesc, o->a, o->o_del, o->e_del);
	w2 = bmh_rp_infer_bw(ql, tl, truesc, o->a, o->o_ins, o->e_ins);
	w2 = w2 > tmp ? w2 : tmp;
	if (w2 > o->w) w2 = w2 < reg_w ? w2 : reg_w;
	return w2;
}

/* ---- band of a try whose inferred band is w2 (bwa.c:116-125) */
BMH_RP_HD static inline int bmh_rp_try_band(const bmh_rp_opt_t *o, int ql, int tl, int w2)
{
	BMH_PP_NOCONTRACT
	const int max_ins = bmh_pp_d2i((double)(((ql + 1) >> 1) * o->mat0 - o->o_ins) / o->e_ins + 1.);
	const int max_del = bmh_pp_d2i((double)(((ql + 1) >> 1) * o->mat0 - o->o_del) / o->e_del + 1.);
	int max_gap = max_ins > max_del ? max_ins : max_del, w, min_w;
	max_gap = max_gap > 1 ? max_gap : 1;
	w = (int)(((int64_t)max_gap + bmh_rp_iabs(tl - ql) + 1) >> 1);
	w = w < w2 ? w : w2;
	min_w = bmh_rp_iabs(tl - ql) + 3;
	return w > min_w ? w : min_w;
}

/* w2 << t as the loop of bwamem.c:1194-1201 widens it, saturating */
BMH_RP_HD static inline int bmh_rp_widen(int w2, int t)
{
	const int64_t x = w2 < 0 ? (int64_t)w2 : (int64_t)w2 << t;
	return x > INT32_MAX ? INT32_MAX : (int)x;
}

/* ---- one region's plan: the band of each try (-1: no such try; band[0] == -1: the no-gap case, ql == tl && w2 == 0, bwa.c:108-114),
 * which of its n_tasks global alignments each try reads (equal bands share one: the band saturates at bwa.c:119-124), and the CIGAR
 * slots of each task */
typedef struct bmh_rp_plan {
	int32_t band[3], slot[3];
	int32_t n_tasks;
	uint32_t cap;
} bmh_rp_plan_t;

BMH_RP_HD static inline void bmh_rp_plan(const bmh_rp_opt_t *o, int ql, int tl, int truesc, int reg_w, bmh_rp_plan_t *pl)
{
	const int single = truesc == INT32_MIN;
	const int w2 = bmh_rp_first_band(o, ql, tl, truesc, reg_w);
	int t, prev_w = -1;
	pl->band[0] = pl->band[1] = pl->band[2] = -1;
	pl->slot[0] = pl->slot[1] = pl->slot[2] = -1;
	pl->n_tasks = 0;
	pl->cap = (uint32_t)(ql + tl + 2 < BMH_RP_SMALL_CAP ? ql + tl + 2 : BMH_RP_SMALL_CAP);
	if (ql == tl && w2 == 0) return;
	for (t = 0; t < (single ? 1 : 3); ++t) {
		const int w = bmh_rp_try_band(o, ql, tl, bmh_rp_widen(w2, t));
		pl->band[t] = w;
		if (w == prev_w) { pl->slot[t] = pl->slot[t - 1]; continue; }
		prev_w = w;
		pl->slot[t] = pl->n_tasks++;
	}
}

/* ... and its record and tasks: the oriented copies at o_off (query, then window), task indices from task0, CIGAR slots from cig0 */
BMH_RP_HD static inline void bmh_rp_emit(const bmh_rp_plan_t *pl, uint64_t q_src, int64_t rb, uint64_t o_off, int ql, int tl, int truesc,
                                         int64_t task0, uint64_t cig0, bmh_region_req_t *q, bmh_glb_task_t *tasks)
{
	int t, made = 0;
	q->q_src = q_src, q->rb = rb, q->o_off = o_off, q->ql = ql, q->tl = tl, q->truesc = truesc;
	for (t = 0; t < 3; ++t) q->task[t] = pl->slot[t] < 0 ? -1 : (int32_t)(task0 + pl->slot[t]);
	for (t = 0; t < 3; ++t) {
		bmh_glb_task_t *x;
		if (pl->slot[t] != made) continue; /* the first try that uses task `made` */
		x = &tasks[made];
		x->q_off = o_off, x->t_off = o_off + (uint64_t)ql, x->qlen = (uint16_t)ql, x->tlen = (uint16_t)tl, x->w = pl->band[t];
		x->cigar_off = (uint32_t)(cig0 + (uint64_t)made * pl->cap), x->cigar_cap = pl->cap;
		++made;
	}
}

#endif
