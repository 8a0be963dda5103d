/*
 * sam_post.c -- region post-processing and SAM text (host side, plain C, above the C-ABI).
 *
 * What mem_process_seqs does with a read's region vector after the extensions:
 *
 *   bmh_sort_and_dedup    mem_sort_and_dedup    reference bwa-0.7.8/bwamem.c:395-436
 *   bmh_mark_primary_se   mem_mark_primary_se   bwamem.c:445-475
 *   bmh_approx_mapq_se    mem_approx_mapq_se    bwamem.c:1023-1047
 *   bmh_pestat            mem_pestat            bwamem_pair.c:46-107   (cal_sub :34-44, mem_infer_dir :25-32)
 *   bmh_sam_batch         worker2 (bwamem.c:1281-1295) for a slice of a chunk: mem_reg2sam_se (:1049-1083) or
 *                         mem_sam_pe (bwamem_pair.c:240-332, without its rescue block) over mem_pair (:177-238),
 *                         mem_reg2aln (bwamem.c:1164-1236), bwa_fix_xref2 (bwa.c:179-222), mem_aln2sam (bwamem.c:904-1017)
 *
 * The reference interleaves decisions, global alignments and text per read.  Here a slice runs in three passes:
 *   A  per read / pair: primary marking, pairing, mapQ -> the exact list of regions that will be printed
 *   B  their global alignments as GPU batches: first the few regions that hang over the end of a reference sequence
 *      (bwa_fix_xref2 needs one bwa_gen_cigar2 each), then all of them through bmh_reg2cigar_batch (band inference and
 *      the <= 3 widening tries of mem_reg2aln)
 *   C  per read / pair: coordinates, clipping, flags, text
 *      (bmh_sam_text_batch over samtext_core.h: sized first, then written into one pool per slice)
 * No per-region mallocs: alignments live in per-slice arrays.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <time.h>

#include "../../include/bwamem_hip.h"
#include "dedup_core.h"
#include "pestat_core.h"
#include "postproc_core.h"
#include "regplan_core.h"
#include "samcut_core.h"
#include "samtext_core.h"
#include "sort_exact.h"

static double now_s(void) /* the clock of the BMH_DRIVER_TRACE lines: wall time, or with BMH_TRACE_CPU this thread's CPU time */
{
	static int cpu = -1;
	struct timespec ts;
	if (cpu < 0) cpu = getenv("BMH_TRACE_CPU") != 0;
	clock_gettime(cpu ? CLOCK_THREAD_CPUTIME_ID : CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

#define MIN_DIR_CNT 10 /* bwamem_pair.c:15-18; MIN_RATIO (:14) is pestat_core.h's */
#define MIN_DIR_RATIO 0.05
#define OUTLIER_BOUND 2.0
#define MAPPING_BOUND 3.0
#define MAX_STDDEV 4.0

/* ---- orders (utils.c:45); those of mem_sort_and_dedup are in dedup_core.h, those of marking and pairing in postproc_core.h */
static int lt_u64(const void *x, const void *y) { return *(const uint64_t *)x < *(const uint64_t *)y; }
static void sort_u64(uint64_t *a, size_t n, uint64_t max) /* insert sizes: 1..max_ins -> a counting sort where that is small */
{
	if (max < (1u << 22) && n > 64) {
		uint32_t *cnt = (uint32_t *)calloc((size_t)max + 2, sizeof(uint32_t));
		size_t i, k = 0;
		uint64_t v;
		if (cnt) {
			for (i = 0; i < n; ++i) ++cnt[a[i] <= max ? a[i] : max + 1];
			for (v = 0; v <= max + 1; ++v)
				for (; cnt[v]; --cnt[v]) a[k++] = v;
			free(cnt);
			return;
		}
	}
	bmh_sort_exact(a, n, 8, lt_u64);
}

/* ---- bwamem.c:395-436: the routine is dedup_core.h's, shared with the device kernel; here only its range stack */
int bmh_sort_and_dedup(int n, bmh_alnreg_t *a, float mask_level_redun)
{
	bmh_sort_stk_t stk[8 * sizeof(size_t) + 2]; /* >= bmh_sort_stack_len(n) for any n */
	return bmh_dedup_core(n, a, mask_level_redun, stk);
}

#define SORT_STK_LEN (8 * sizeof(size_t) + 2) /* >= bmh_sort_stack_len(n) for any n */

/* ---- bwamem.c:445-475: the routine is postproc_core.h's, shared with the device kernel; here its z[] list and range stack */
void bmh_mark_primary_se(const bmh_sam_opt_t *o, int n, bmh_alnreg_t *a, int64_t id)
{
	bmh_sort_stk_t stk[SORT_STK_LEN];
	int zs[64], *z = zs;
	if (n <= 0) return;
	/* (the reference aborts when its z vector cannot grow; a void routine cannot report it, so say it and leave the vector as it
	 * came -- bmh_decide_batch, which bmh_sam_batch uses, answers BMH_E_NOMEM instead) */
	if (n > 64 && !(z = (int *)malloc(sizeof(int) * (size_t)n))) {
		fprintf(stderr, "[bwamem_hip] bmh_mark_primary_se: out of memory, %d regions left unmarked\n", n);
		return;
	}
	bmh_pp_mark(o, n, a, id, z, stk);
	if (z != zs) free(z);
}

/* ---- bwamem.c:1023-1047 */
int bmh_approx_mapq_se(const bmh_sam_opt_t *o, const bmh_alnreg_t *a) { return bmh_pp_mapq(o, a, 0); }

/* ---- bwamem_pair.c:46-107 in two halves.  The pair walk (:56-72) is pestat_core.h's, shared with the device kernel; the
 * statistics below it are host only: they are cheap, and their two sums are added in ascending order in double. */

/* bwamem_pair.c:73-106 over the candidates of each orientation, q[d][0..qn[d]) */
static void pestat_finish(const bmh_sam_opt_t *o, uint64_t *const qv[4], const size_t qnv[4], bmh_pestat_t pes[4], int verbose)
{
	size_t max;
	int d;
	memset(pes, 0, 4 * sizeof(bmh_pestat_t));
	if (verbose >= 3)
		fprintf(stderr, "[M::mem_pestat] # candidate unique pairs for (FF, FR, RF, RR): (%ld, %ld, %ld, %ld)\n", (long)qnv[0], (long)qnv[1], (long)qnv[2],
		        (long)qnv[3]);
	for (d = 0; d < 4; ++d) {
		bmh_pestat_t *r = &pes[d];
		uint64_t *q = qv[d];
		const size_t qn = qnv[d];
		size_t k;
		int p25, p50, p75, x;
		if (qn < MIN_DIR_CNT) {
			if (verbose >= 0) fprintf(stderr, "[M::mem_pestat] skip orientation %c%c as there are not enough pairs\n", "FR"[d >> 1 & 1], "FR"[d & 1]);
			r->failed = 1;
			continue;
		} else if (verbose >= 0) fprintf(stderr, "[M::mem_pestat] analyzing insert size distribution for orientation %c%c...\n", "FR"[d >> 1 & 1], "FR"[d & 1]);
		sort_u64(q, qn, (uint64_t)o->max_ins); /* ks_introsort_64 (:75): equal keys are indistinguishable, any sort gives its array */
		p25 = (int)q[(int)(.25 * qn + .499)];
		p50 = (int)q[(int)(.50 * qn + .499)];
		p75 = (int)q[(int)(.75 * qn + .499)];
		r->low = (int)(p25 - OUTLIER_BOUND * (p75 - p25) + .499);
		if (r->low < 1) r->low = 1;
		r->high = (int)(p75 + OUTLIER_BOUND * (p75 - p25) + .499);
		if (verbose >= 0) {
			fprintf(stderr, "[M::mem_pestat] (25, 50, 75) percentile: (%d, %d, %d)\n", p25, p50, p75);
			fprintf(stderr, "[M::mem_pestat] low and high boundaries for computing mean and std.dev: (%d, %d)\n", r->low, r->high);
		}
		for (k = 0, x = 0, r->avg = 0; k < qn; ++k)
			if (q[k] >= (uint64_t)r->low && q[k] <= (uint64_t)r->high) r->avg += q[k], ++x;
		r->avg /= x;
		for (k = 0, r->std = 0; k < qn; ++k)
			if (q[k] >= (uint64_t)r->low && q[k] <= (uint64_t)r->high) r->std += (q[k] - r->avg) * (q[k] - r->avg);
		r->std = sqrt(r->std / x);
		if (verbose >= 0) fprintf(stderr, "[M::mem_pestat] mean and std.dev: (%.2f, %.2f)\n", r->avg, r->std);
		r->low = (int)(p25 - MAPPING_BOUND * (p75 - p25) + .499);
		r->high = (int)(p75 + MAPPING_BOUND * (p75 - p25) + .499);
		if (r->low > r->avg - MAX_STDDEV * r->std) r->low = (int)(r->avg - MAX_STDDEV * r->std + .499);
		if (r->high < r->avg - MAX_STDDEV * r->std) r->high = (int)(r->avg + MAX_STDDEV * r->std + .499);
		if (r->low < 1) r->low = 1;
		if (verbose >= 0) fprintf(stderr, "[M::mem_pestat] low and high boundaries for proper pairs: (%d, %d)\n", r->low, r->high);
	}
	for (d = 0, max = 0; d < 4; ++d) max = max > qnv[d] ? max : qnv[d];
	for (d = 0; d < 4; ++d)
		if (pes[d].failed == 0 && qnv[d] < max * MIN_DIR_RATIO) {
			pes[d].failed = 1;
			if (verbose >= 0) fprintf(stderr, "[M::mem_pestat] skip orientation %c%c\n", "FR"[d >> 1 & 1], "FR"[d & 1]);
		}
}

/* one array for the four orientations' candidates, cnt[d] of them each; q[d] = where orientation d's start.  0 = out of memory */
static uint64_t *pestat_split(const size_t cnt[4], uint64_t *q[4])
{
	uint64_t *buf = (uint64_t *)malloc(8 * (cnt[0] + cnt[1] + cnt[2] + cnt[3] + 1));
	if (buf) q[0] = buf, q[1] = q[0] + cnt[0], q[2] = q[1] + cnt[1], q[3] = q[2] + cnt[2];
	return buf;
}

/* the pair walk, bwamem_pair.c:56-72, over np pairs: the one loop behind bmh_pestat_candidates (w32: the words) and bmh_pestat (w64:
 * dir << 62 | is, which holds any max_ins).  Exactly one of w32, w64 is given. */
static void pestat_walk(const bmh_sam_opt_t *o, int64_t l_pac, size_t np, const bmh_alnreg_v *regs, uint32_t *w32, uint64_t *w64)
{
	size_t i;
	for (i = 0; i < np; ++i) {
		const bmh_alnreg_v *r0 = &regs[i << 1 | 0], *r1 = &regs[i << 1 | 1];
		int64_t is = 0;
		int dir;
		if (i + 8 < np) /* every read's region vector is an allocation of its own: this serial loop is all cache misses */
			__builtin_prefetch(regs[(i + 8) << 1].a), __builtin_prefetch(regs[(i + 8) << 1 | 1].a);
		dir = bmh_ps_pair(o, l_pac, r0->a, r0->n, r1->a, r1->n, &is);
		if (w32) w32[i] = dir < 0 ? 0 : (uint32_t)dir << 30 | (uint32_t)is; /* == bmh_ps_candidate */
		else w64[i] = dir < 0 ? 0 : (uint64_t)dir << 62 | (uint64_t)is;
	}
}

int bmh_pestat_candidates(const bmh_sam_opt_t *o, int64_t l_pac, int n, const bmh_alnreg_v *regs, uint32_t *cand)
{
	int i;
	if (!o || l_pac < 0 || n < 0 || (n > 0 && !regs) || (n > 1 && !cand)) return BMH_E_ARG;
	if (o->max_ins > BMH_PS_MAX_INS) return BMH_E_RANGE;
	for (i = 0; i < (n & ~1); ++i)
		if (regs[i].n && !regs[i].a) return BMH_E_ARG;
	pestat_walk(o, l_pac, (size_t)(n >> 1), regs, cand, 0);
	return BMH_OK;
}

int bmh_pestat_from_candidates(const bmh_sam_opt_t *o, int64_t n_pairs, const uint32_t *cand, bmh_pestat_t pes[4], int verbose)
{
	size_t cnt[4] = {0, 0, 0, 0}, at[4] = {0, 0, 0, 0};
	uint64_t *q[4], *buf;
	int64_t i;
	if (!o || n_pairs < 0 || (n_pairs > 0 && !cand) || !pes) return BMH_E_ARG;
	if (o->max_ins > BMH_PS_MAX_INS) return BMH_E_RANGE;
	for (i = 0; i < n_pairs; ++i) {
		if (!cand[i]) continue;
		if (BMH_PS_IS(cand[i]) == 0 || BMH_PS_IS(cand[i]) > o->max_ins) return BMH_E_ARG; /* no word of bmh_ps_candidate; pes is as it came */
		++cnt[BMH_PS_DIR(cand[i])];
	}
	if (!(buf = pestat_split(cnt, q))) return BMH_E_NOMEM;
	for (i = 0; i < n_pairs; ++i)
		if (cand[i]) q[BMH_PS_DIR(cand[i])][at[BMH_PS_DIR(cand[i])]++] = (uint64_t)BMH_PS_IS(cand[i]);
	pestat_finish(o, q, cnt, pes, verbose);
	free(buf);
	return BMH_OK;
}

/* candidates, then finish.  The candidates are kept as 64-bit values (dir << 62 | is), so any max_ins is served */
void bmh_pestat(const bmh_sam_opt_t *o, int64_t l_pac, int n, const bmh_alnreg_v *regs, bmh_pestat_t pes[4], int verbose)
{
	const size_t np = n > 0 ? (size_t)(n >> 1) : 0;
	size_t cnt[4] = {0, 0, 0, 0}, at[4] = {0, 0, 0, 0}, i;
	uint64_t *v = (uint64_t *)malloc(8 * (np + 1)), *q[4], *buf = 0;
	if (v) pestat_walk(o, l_pac, np, regs, 0, v);
	for (i = 0; v && i < np; ++i)
		if (v[i]) ++cnt[v[i] >> 62];
	/* Out of memory: the reference aborts when its vectors cannot grow; a void routine can only say it, so it prints a message and
	 * marks all four orientations as failed (pairing then goes without insert-size windows).  No test reaches this branch. */
	if (!v || !(buf = pestat_split(cnt, q))) {
		fprintf(stderr, "[bwamem_hip] bmh_pestat: out of memory, every orientation is marked as failed\n");
		memset(pes, 0, 4 * sizeof(bmh_pestat_t));
		pes[0].failed = pes[1].failed = pes[2].failed = pes[3].failed = 1;
		free(v);
		return;
	}
	for (i = 0; i < np; ++i)
		if (v[i]) q[v[i] >> 62][at[v[i] >> 62]++] = v[i] & ~(3ull << 62);
	free(v);
	pestat_finish(o, q, cnt, pes, verbose);
	free(buf);
}

/* ---- bwamem_pair.c:177-238: the routine is postproc_core.h's; here its key vector and range stack */
int bmh_pair(const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t pes[4], const bmh_alnreg_v a[2], uint64_t id, int *sub, int *n_sub, int z[2])
{
	bmh_sort_stk_t stk[SORT_STK_LEN];
	bmh_pair64_t *v = (bmh_pair64_t *)malloc(sizeof(bmh_pair64_t) * (a[0].n + a[1].n + 1));
	int ret;
	*sub = *n_sub = 0;
	if (!v) return 0;
	ret = bmh_pp_pair(o, l_pac, pes, 0, (int)a[0].n, a[0].a, (int)a[1].n, a[1].a, id, sub, n_sub, z, v, stk);
	free(v);
	return ret;
}

/* ---- pass A of bmh_sam_batch: the decisions, per read or pair, over postproc_core.h (on the device: bmh_decide_device) */
int bmh_decide_batch(const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t *pes, int64_t id0, int n, bmh_alnreg_v *regs, const int64_t *roff,
                     bmh_pairdec_t *pd, int32_t *reg_mapq, int32_t *n_want, int32_t *want_k)
{
	bmh_sort_stk_t stk[SORT_STK_LEN];
	const int pe = o && (o->flag & BMH_MEM_F_PE) != 0;
	size_t zmax = 1, vmax = 1;
	int *z = 0;
	bmh_pair64_t *v = 0;
	int i, rc;
	if ((rc = bmh_pp_check_args(o, pes, n, regs, roff, pd, reg_mapq, n_want, want_k))) return rc;
	if (n == 0) return BMH_OK;
	for (i = 0; i < n; ++i) {
		zmax = regs[i].n > zmax ? regs[i].n : zmax;
		if (pe && (i & 1)) vmax = regs[i - 1].n + regs[i].n > vmax ? regs[i - 1].n + regs[i].n : vmax;
	}
	z = (int *)malloc(sizeof(int) * zmax * 2);
	if (pe) v = (bmh_pair64_t *)malloc(sizeof(bmh_pair64_t) * vmax);
	if (!z || (pe && !v)) {
		free(z), free(v);
		return BMH_E_NOMEM;
	}
	if (!pe) {
		for (i = 0; i < n; ++i) { /* worker2's SE branch, bwamem.c:1285-1289 */
			if (i + 8 < n) __builtin_prefetch(regs[i + 8].a);
			bmh_pp_unit_se(o, 0, id0 + i, (int)regs[i].n, regs[i].a, z, stk, reg_mapq + roff[i], &n_want[i], want_k + roff[i]);
		}
	} else {
		for (i = 0; i < n >> 1; ++i) { /* mem_sam_pe after its rescue block, bwamem_pair.c:264-331 */
			const bmh_alnreg_v *a = &regs[i << 1];
			const uint64_t id = (uint64_t)(id0 >> 1) + (uint64_t)i;
			const int nn[2] = {(int)a[0].n, (int)a[1].n};
			bmh_alnreg_t *const aa[2] = {a[0].a, a[1].a};
			int *const zz[2] = {z, z + zmax};
			int32_t *const mq[2] = {reg_mapq + roff[i << 1], reg_mapq + roff[i << 1 | 1]};
			int32_t *const wk[2] = {want_k + roff[i << 1], want_k + roff[i << 1 | 1]};
			if (i + 6 < n >> 1) __builtin_prefetch(regs[(i + 6) << 1].a), __builtin_prefetch(regs[(i + 6) << 1 | 1].a);
			bmh_pp_unit_pe(o, l_pac, pes, 0, id, nn, aa, zz, v, stk, &pd[i], mq, &n_want[i << 1], wk);
		}
	}
	free(z), free(v);
	return BMH_OK;
}

/* the device call's tables, made HERE so that they come from the compiler and the libm the host routines above use
 * (csrc/api.hip calls these; not part of the interface) */
__attribute__((visibility("hidden"))) void bmh_pp_fill_log_(double *logk, int64_t k0, int64_t k1) { bmh_pp_fill_log(logk, k0, k1); }
__attribute__((visibility("hidden"))) void bmh_pp_fill_term_(const bmh_sam_opt_t *o, const bmh_pestat_t *pes, const int64_t term_off[4], double *term)
{
	bmh_pp_fill_term(o, pes, term_off, term);
}

/* ================================================================================================ alignments and text */

static bmh_rp_refv_t refv_of(const bmh_refidx_t *bns) /* the reference sequences as regplan_core.h walks them */
{
	bmh_rp_refv_t v;
	v.off0 = bns->anns ? &bns->anns[0].offset : 0, v.len0 = bns->anns ? &bns->anns[0].len : 0, v.stride = sizeof(bmh_refann_t);
	v.n_seqs = bns->n_seqs, v.l_pac = bns->l_pac;
	return v;
}

const bmh_params_t *bmh_ctx_params_(const bmh_ctx_t *ctx);

/* ================================================================================================ pass B: the alignments
 * bwa_fix_xref2 (bwa.c:179-222) for the few regions that hang over the end of a reference sequence (one bwa_gen_cigar2 each), then
 * mem_reg2aln's band loop (bwamem.c:1187-1201) for every wanted region, as GPU batches through bmh_reg2cigar_batch.  Everything that
 * needs no sequence byte is regplan_core.h's, shared with the planning kernels of bmh_wanted_cigar_device (csrc/wanted.hip). */

enum { MD_SLOT_ = BMH_RP_MD_SLOT };

/* what both forms refuse before anything runs (host only) */
static int wanted_check_args(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int n, const bmh_read_t *reads, const bmh_alnreg_v *regs,
                             const int64_t *roff, const int32_t *n_want, const int32_t *want_k, int64_t *n_w)
{
	int64_t at = 0, w = 0;
	int i;
	*n_w = 0;
	if (!ctx || !bns || !pac || n < 0 || bns->l_pac <= 0 || bns->n_seqs <= 0 || !bns->anns) return BMH_E_ARG;
	if (n > 0 && (!reads || !regs || !roff || !n_want || !want_k)) return BMH_E_ARG;
	for (i = 0; i < n; ++i) {
		if ((regs[i].n && !regs[i].a) || regs[i].n > 0x7fffffffu || roff[i] != at) return BMH_E_ARG;
		if (n_want[i] < 0 || (size_t)n_want[i] > regs[i].n) return BMH_E_ARG;
		if (reads[i].l_seq < 0 || (reads[i].l_seq > 0 && !reads[i].seq)) return BMH_E_ARG;
		at += (int64_t)regs[i].n, w += n_want[i];
	}
	if (n > 0 && roff[n] != at) return BMH_E_ARG;
	*n_w = w;
	return BMH_OK;
}

/* a wanted region as the planning sees it: BMH_E_ARG / BMH_E_RANGE as the kernel gives them, else 0 */
static int wanted_check_region(int64_t l_pac, int l_seq, const bmh_alnreg_t *a)
{
	if (!(0 <= a->qb && a->qb < a->qe && a->qe <= l_seq)) return BMH_E_ARG;
	if (!(a->rb >= 0 && a->rb < a->re && a->re <= l_pac << 1)) return BMH_E_ARG;
	if (a->rb < l_pac && a->re > l_pac) return BMH_E_ARG; /* bridges the strands: the reference gives up on the run (bwamem.c:1183-1186) */
	if (a->qe - a->qb > 65535 || a->re - a->rb > 65535) return BMH_E_RANGE;
	return 0;
}

/* The host form.  wr[0..n_w) in want order (n_w = sum of n_want); cigar_off / md_off address *cig_ / *md_, malloc'd here (the
 * caller frees them), in bmh_reg2cigar_batch's packing.  bands: fill band[] (the public call; bmh_sam_batch has no use for it). */
__attribute__((visibility("hidden"))) int bmh_wanted_host_(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads,
                                                           const bmh_alnreg_v *regs, const int64_t *roff, const int32_t *n_want, const int32_t *want_k,
                                                           int64_t n_w, int bands, bmh_wanted_res_t *wr, uint32_t **cig_, char **md_, int64_t *n_fixed)
{
	const int64_t l_pac = bns->l_pac;
	const bmh_rp_refv_t rv = refv_of(bns);
	const bmh_params_t *p = bmh_ctx_params_(ctx);
	bmh_cigar_req_t *reqs = 0, *fq = 0;
	bmh_cigar_res_t *res = 0, *fr = 0;
	int64_t *cbe = 0; /* cb, ce of fix f */
	uint32_t *cig = 0, *fc = 0;
	char *md = 0, *fmd = 0;
	size_t j, n_fix = 0, cw = 8, mb = 16, fw = 8, fm_ = 16;
	int i, q, rc = BMH_OK;

	*cig_ = 0, *md_ = 0;
	if (n_fixed) *n_fixed = 0;
	if (!p) return BMH_E_ARG;
	if (n_w == 0) return BMH_OK;
	reqs = (bmh_cigar_req_t *)malloc(sizeof(*reqs) * (size_t)n_w);
	res = (bmh_cigar_res_t *)malloc(sizeof(*res) * (size_t)n_w);
	if (!reqs || !res) { rc = BMH_E_NOMEM; goto done; }
	for (i = 0, j = 0; i < n; ++i) /* the want list as requests; the bwa_fix_xref2 test (bwa.c:184-197) */
		for (q = 0; q < n_want[i]; ++q, ++j) {
			const int k = want_k[roff[i] + q];
			const bmh_alnreg_t *ar;
			bmh_wanted_res_t *x = &wr[j];
			int64_t cb, ce;
			if (k < 0 || (size_t)k >= regs[i].n) { rc = BMH_E_ARG; goto done; }
			ar = &regs[i].a[k];
			if ((rc = wanted_check_region(l_pac, reads[i].l_seq, ar))) goto done;
			memset(x, 0, sizeof(*x));
			x->rb = ar->rb, x->re = ar->re, x->qb = ar->qb, x->qe = ar->qe;
			x->band[0] = x->band[1] = x->band[2] = -1;
			reqs[j].read = i, reqs[j].truesc = ar->truesc, reqs[j].reg_w = ar->w;
			if (bmh_rp_xref_test(&rv, x->rb, x->re, &cb, &ce) > 0) {
				int64_t *t = (int64_t *)realloc(cbe, sizeof(int64_t) * 2 * (n_fix + 1));
				if (!t) { rc = BMH_E_NOMEM; goto done; }
				cbe = t, cbe[2 * n_fix] = cb, cbe[2 * n_fix + 1] = ce;
				x->flags = BMH_WANTED_MOVED, x->rsv_ = (int32_t)n_fix++; /* (rsv_ holds the fix index until the cut) */
				fw += (size_t)(x->qe - x->qb) + (size_t)(x->re - x->rb) + 2, fm_ += 3 * ((size_t)(x->qe - x->qb) + (size_t)(x->re - x->rb)) + 16;
			}
		}
	if (n_fix) { /* one bwa_gen_cigar2(w_ = opt->w) per such region, then walk its CIGAR to the cut points (bwa.c:198-219) */
		size_t f = 0;
		fq = (bmh_cigar_req_t *)malloc(sizeof(*fq) * n_fix), fr = (bmh_cigar_res_t *)malloc(sizeof(*fr) * n_fix);
		fc = (uint32_t *)malloc(4 * fw), fmd = (char *)malloc(fm_);
		if (!fq || !fr || !fc || !fmd) { rc = BMH_E_NOMEM; goto done; }
		for (j = 0; j < (size_t)n_w; ++j) {
			const bmh_wanted_res_t *x = &wr[j];
			if (!(x->flags & BMH_WANTED_MOVED)) continue;
			fq[f].read = reqs[j].read, fq[f].qb = x->qb, fq[f].qe = x->qe, fq[f].rb = x->rb, fq[f].re = x->re, fq[f].truesc = INT32_MIN, fq[f].reg_w = w;
			++f;
		}
		if ((rc = bmh_reg2cigar_batch(ctx, l_pac, pac, reads, (int64_t)n_fix, fq, fr, fc, fw, fmd, fm_))) goto done;
		for (j = 0; j < (size_t)n_w; ++j) {
			bmh_wanted_res_t *x = &wr[j];
			int f_;
			if (!(x->flags & BMH_WANTED_MOVED)) continue;
			f_ = x->rsv_, x->rsv_ = 0;
			if (fr[f_].n_cigar > BMH_RP_SMALL_CAP) x->flags |= BMH_WANTED_HOST;
			if (bmh_rp_xref_cut(fr[f_].n_cigar, fc + fr[f_].cigar_off, cbe[2 * f_], cbe[2 * f_ + 1], &x->qb, &x->qe, &x->rb, &x->re)) {
				rc = BMH_E_ARG; /* bwa_fix_xref2 returns -2: the reference aborts */
				goto done;
			}
		}
	}
	for (j = 0; j < (size_t)n_w; ++j) {
		const bmh_wanted_res_t *x = &wr[j];
		reqs[j].qb = x->qb, reqs[j].qe = x->qe, reqs[j].rb = x->rb, reqs[j].re = x->re;
		cw += (size_t)(x->qe - x->qb) + (size_t)(x->re - x->rb) + 2, mb += 3 * ((size_t)(x->qe - x->qb) + (size_t)(x->re - x->rb)) + 16;
	}
	{ /* pools: a CIGAR may have ql+tl+1 operations and an MD 3 bytes per base, but they almost never have more than a
	   * few -- try with 16 words / 48 bytes per region (plus one region's worst case) and only fall back to the sizes
	   * that always suffice if the driver says BMH_E_CIGAR_CAP (hundreds of megabytes of untouched-but-mapped memory
	   * per slice, mapped and unmapped by every host thread at once, cost more than the alignments) */
		size_t cw2 = 16 * (size_t)n_w + 70000, mb2 = 48 * (size_t)n_w + 3 * 140000 + 64;
		if (cw2 > cw) cw2 = cw;
		if (mb2 > mb) mb2 = mb;
		cig = (uint32_t *)malloc(4 * cw2), md = (char *)malloc(mb2);
		if (!cig || !md) { rc = BMH_E_NOMEM; goto done; }
		rc = bmh_reg2cigar_batch(ctx, l_pac, pac, reads, n_w, reqs, res, cig, cw2, md, mb2);
		if (rc == BMH_E_CIGAR_CAP && (cw2 < cw || mb2 < mb)) {
			free(cig), free(md);
			cig = (uint32_t *)malloc(4 * cw), md = (char *)malloc(mb);
			if (!cig || !md) { rc = BMH_E_NOMEM; goto done; }
			rc = bmh_reg2cigar_batch(ctx, l_pac, pac, reads, n_w, reqs, res, cig, cw, md, mb);
		}
		if (rc) goto done;
	}
	for (j = 0; j < (size_t)n_w; ++j) {
		bmh_wanted_res_t *x = &wr[j];
		x->score = res[j].score, x->n_cigar = res[j].n_cigar, x->NM = res[j].NM, x->tries = res[j].tries;
		x->cigar_off = res[j].cigar_off, x->md_off = res[j].md_off, x->md_len = res[j].md_len;
		if (res[j].n_cigar > BMH_RP_SMALL_CAP || res[j].md_len > MD_SLOT_) x->flags |= BMH_WANTED_HOST;
		if (bands) {
			const bmh_rp_opt_t po = {p->a, p->mat[0], p->o_del, p->e_del, p->o_ins, p->e_ins, p->w};
			bmh_rp_plan_t pl;
			bmh_rp_plan(&po, x->qe - x->qb, (int)(x->re - x->rb), reqs[j].truesc, reqs[j].reg_w, &pl);
			x->band[0] = pl.band[0], x->band[1] = pl.band[1], x->band[2] = pl.band[2];
		}
	}
	if (n_fixed) *n_fixed = (int64_t)n_fix;
	*cig_ = cig, *md_ = md, cig = 0, md = 0;
done:
	free(reqs), free(res), free(fq), free(fr), free(cbe), free(fc), free(fmd), free(cig), free(md);
	return rc;
}

/* the caller's records and pools, in want order, from a form's own: written only here, after everything has succeeded */
__attribute__((visibility("hidden"))) int bmh_wanted_deliver_(int64_t n_w, const bmh_wanted_res_t *wr, const uint32_t *cig, const char *md,
                                                              bmh_wanted_res_t *results, uint32_t *cigar_pool, size_t cigar_words, char *md_pool, size_t md_bytes)
{
	size_t cu = 0, mu = 0;
	int64_t j;
	for (j = 0; j < n_w; ++j) cu += (size_t)wr[j].n_cigar, mu += (size_t)wr[j].md_len + 1;
	if (cu > cigar_words || mu > md_bytes) return BMH_E_CIGAR_CAP;
	for (j = 0, cu = mu = 0; j < n_w; ++j) {
		bmh_wanted_res_t x = wr[j];
		memcpy(cigar_pool + cu, cig + x.cigar_off, 4 * (size_t)x.n_cigar);
		memcpy(md_pool + mu, md + x.md_off, (size_t)x.md_len);
		md_pool[mu + x.md_len] = 0;
		x.cigar_off = (uint32_t)cu, x.md_off = (uint32_t)mu;
		results[j] = x;
		cu += (size_t)x.n_cigar, mu += (size_t)x.md_len + 1;
	}
	return BMH_OK;
}

int bmh_wanted_cigar_batch(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads, const bmh_alnreg_v *regs,
                           const int64_t *roff, const int32_t *n_want, const int32_t *want_k, bmh_wanted_res_t *results, uint32_t *cigar_pool,
                           size_t cigar_words, char *md_pool, size_t md_bytes)
{
	bmh_wanted_res_t *wr = 0;
	uint32_t *cig = 0;
	char *md = 0;
	int64_t n_w;
	int rc = wanted_check_args(ctx, bns, pac, n, reads, regs, roff, n_want, want_k, &n_w);
	if (rc) return rc;
	if (n_w == 0) return BMH_OK;
	if (!results || !cigar_pool || !md_pool) return BMH_E_ARG;
	if (!(wr = (bmh_wanted_res_t *)malloc(sizeof(*wr) * (size_t)n_w))) return BMH_E_NOMEM;
	rc = bmh_wanted_host_(ctx, bns, pac, w, n, reads, regs, roff, n_want, want_k, n_w, 1, wr, &cig, &md, 0);
	if (!rc) rc = bmh_wanted_deliver_(n_w, wr, cig, md, results, cigar_pool, cigar_words, md_pool, md_bytes);
	free(wr), free(cig), free(md);
	return rc;
}

/* the argument check of the two public forms, for csrc/api.hip */
__attribute__((visibility("hidden"))) int bmh_wanted_check_args_(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int n, const bmh_read_t *reads,
                                                                 const bmh_alnreg_v *regs, const int64_t *roff, const int32_t *n_want, const int32_t *want_k,
                                                                 int64_t *n_w)
{
	return wanted_check_args(ctx, bns, pac, n, reads, regs, roff, n_want, want_k, n_w);
}

/* ================================================================================================ pass C: coordinates and text
 * mem_reg2aln's second half (bwamem.c:1203-1235) and mem_reg2sam_se / mem_aln2sam (bwamem.c:904-1083) for a slice, over samtext_core.h,
 * the text the kernels of bmh_sam_text_device (csrc/samtext.hip) run: here only the checks, the arrays and the two passes. */

static int mates_named_alike(int n, const bmh_seq_t *seqs) /* reads 2p, 2p + 1 of an even n, every name there */
{
	int i;
	for (i = 0; i < n; i += 2)
		if (strcmp(seqs[i].name, seqs[i + 1].name) != 0) {
			fprintf(stderr, "[bwamem_hip] paired reads have different names: \"%s\", \"%s\"\n", seqs[i].name, seqs[i + 1].name);
			return BMH_E_ARG;
		}
	return BMH_OK;
}

/* what both forms refuse before anything runs (host only).  first: n + 1 entries, first[i] = wanted regions before read i; *lines = SAM
 * lines of the slice; *cig_words / *md_bytes = how far the records reach into the two pools */
__attribute__((visibility("hidden"))) int bmh_samtext_check_(const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs,
                                                             const bmh_alnreg_v *regs, const int64_t *roff, const bmh_pairdec_t *pd, const int32_t *reg_mapq,
                                                             const int32_t *n_want, const int32_t *want_k, const bmh_wanted_res_t *wr, const uint32_t *cig,
                                                             const char *md, char **text, int64_t *text_off, int64_t *first, int64_t *lines, size_t *cig_words,
                                                             size_t *md_bytes)
{
	const int pe = o && (o->flag & BMH_MEM_F_PE) != 0;
	int64_t at = 0, w = 0, j, nl = 0;
	size_t cw = 0, mb = 0;
	int i, q;
	*lines = 0, *cig_words = 0, *md_bytes = 0;
	if (!o || !bns || !text || !text_off || n < 0 || (pe && ((n & 1) || !pes))) return BMH_E_ARG;
	if (n == 0) return BMH_OK;
	if (!first || !seqs || !regs || !roff || !reg_mapq || !n_want || !want_k || (pe && !pd)) return BMH_E_ARG;
	if (bns->l_pac <= 0 || bns->n_seqs <= 0 || !bns->anns) return BMH_E_ARG;
	for (i = 0; i < bns->n_seqs; ++i)
		if (!bns->anns[i].name) return BMH_E_ARG;
	for (i = 0; i < n; ++i) {
		if ((regs[i].n && !regs[i].a) || regs[i].n > 0x7fffffffu || roff[i] != at) return BMH_E_ARG;
		if (n_want[i] < 0 || (size_t)n_want[i] > regs[i].n) return BMH_E_ARG;
		if (!seqs[i].name || seqs[i].l_seq < 0 || (seqs[i].l_seq > 0 && !seqs[i].seq)) return BMH_E_ARG;
		for (q = 0; q < n_want[i]; ++q)
			if (want_k[at + q] < 0 || (size_t)want_k[at + q] >= regs[i].n) return BMH_E_ARG;
		first[i] = w;
		at += (int64_t)regs[i].n, w += n_want[i];
		nl += pe && pd[i >> 1].paired ? 1 : n_want[i] ? n_want[i] : 1;
	}
	first[n] = w;
	if (roff[n] != at || (w > 0 && (!wr || !cig || !md))) return BMH_E_ARG;
	for (j = 0; j < w; ++j) {
		if (wr[j].n_cigar < 0) return BMH_E_ARG;
		if ((size_t)wr[j].cigar_off + (size_t)wr[j].n_cigar > cw) cw = (size_t)wr[j].cigar_off + (size_t)wr[j].n_cigar;
		if ((size_t)wr[j].md_off + (size_t)wr[j].md_len > mb) mb = (size_t)wr[j].md_off + (size_t)wr[j].md_len;
	}
	if (pe && (i = mates_named_alike(n, seqs))) return i;
	*lines = nl, *cig_words = cw, *md_bytes = mb;
	return BMH_OK;
}

/* what bmh_samtext_check_ refuses of the arguments, the reads and the names alone: a slice whose regions are on the device already
 * (bmh_reads_sam_device, csrc/api.hip) */
__attribute__((visibility("hidden"))) int bmh_samtext_check_reads_(const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n,
                                                                   const bmh_seq_t *seqs, char **text, int64_t *text_off)
{
	const int pe = o && (o->flag & BMH_MEM_F_PE) != 0;
	int i;
	if (!o || !bns || !text || !text_off || n < 0 || (pe && ((n & 1) || !pes))) return BMH_E_ARG;
	if (n == 0) return BMH_OK;
	if (!seqs || bns->l_pac <= 0 || bns->n_seqs <= 0 || !bns->anns) return BMH_E_ARG;
	for (i = 0; i < bns->n_seqs; ++i)
		if (!bns->anns[i].name) return BMH_E_ARG;
	for (i = 0; i < n; ++i)
		if (!seqs[i].name || seqs[i].l_seq < 0 || (seqs[i].l_seq > 0 && !seqs[i].seq)) return BMH_E_ARG;
	return pe ? mates_named_alike(n, seqs) : BMH_OK;
}

/* what bmh_samtext_check_ refuses of a slice whose pass A and pass B outputs stay on the device (bmh_phase2_text_device, csrc/api.hip):
 * the arguments, the reads and the names.  The vectors and offsets are bmh_pp_check_args's there. */
__attribute__((visibility("hidden"))) int bmh_samtext_check_seqs_(const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n,
                                                                  const bmh_seq_t *seqs, const bmh_alnreg_v *regs, char **text, int64_t *text_off)
{
	if (n > 0 && !regs) return BMH_E_ARG;
	return bmh_samtext_check_reads_(o, bns, pes, n, seqs, text, text_off);
}

int bmh_sam_text_batch(const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs, const bmh_alnreg_v *regs,
                       const int64_t *roff, const bmh_pairdec_t *pd, const int32_t *reg_mapq, const int32_t *n_want, const int32_t *want_k,
                       const bmh_wanted_res_t *results, const uint32_t *cigar_pool, const char *md_pool, const char *rg_id, char **text, int64_t *text_off)
{
	const int pe = o && (o->flag & BMH_MEM_F_PE) != 0, nr = pe ? 2 : 1;
	bmh_rp_refv_t rv;
	bmh_st_env_t E;
	bmh_st_read_t *rd = 0;
	bmh_st_aln_t *alns = 0;
	bmh_st_plan_t *plan = 0;
	int64_t *first = 0, *off = 0, lines, j;
	uint64_t *noff = 0;
	char *npool = 0, *buf = 0;
	size_t cw, mb, nb = 0;
	int i, r, rc;

	if (n > 0 && !(first = (int64_t *)malloc(sizeof(int64_t) * ((size_t)n + 1)))) return BMH_E_NOMEM;
	if ((rc = bmh_samtext_check_(o, bns, pes, n, seqs, regs, roff, pd, reg_mapq, n_want, want_k, results, cigar_pool, md_pool, text, text_off, first, &lines,
	                             &cw, &mb)))
		goto done;
	if (n == 0) {
		if (!(buf = (char *)malloc(1))) return BMH_E_NOMEM;
		*text = buf, text_off[0] = 0;
		return BMH_OK;
	}
	rv = refv_of(bns);
	for (i = 0; i < bns->n_seqs; ++i) nb += strlen(bns->anns[i].name);
	noff = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)bns->n_seqs + 1)), npool = (char *)malloc(nb + 1);
	rd = (bmh_st_read_t *)malloc(sizeof(*rd) * (size_t)n);
	alns = (bmh_st_aln_t *)malloc(sizeof(*alns) * ((size_t)first[n] + 1));
	plan = (bmh_st_plan_t *)malloc(sizeof(*plan) * (size_t)n);
	off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)n + 1));
	if (!noff || !npool || !rd || !alns || !plan || !off) { rc = BMH_E_NOMEM; goto done; }
	for (i = 0, nb = 0; i < bns->n_seqs; ++i) {
		const size_t l = strlen(bns->anns[i].name);
		noff[i] = nb, memcpy(npool + nb, bns->anns[i].name, l), nb += l;
	}
	noff[bns->n_seqs] = nb;
	E.names.pool = npool, E.names.off = noff, E.names.n_seqs = bns->n_seqs, E.names.rsv_ = 0;
	E.cig = cigar_pool, E.md = md_pool, E.rg_id = rg_id, E.l_rg = rg_id ? (int32_t)strlen(rg_id) : 0, E.rsv_ = 0;
	for (i = 0; i < n; ++i) { /* the records, in want order */
		const bmh_seq_t *s = &seqs[i];
		bmh_st_read_t *v = &rd[i];
		v->name = s->name, v->l_name = (int32_t)strlen(s->name), v->comment = s->comment, v->l_comment = s->comment ? (int32_t)strlen(s->comment) : 0;
		v->qual = s->qual, v->seq = (const uint8_t *)s->seq, v->l_seq = s->l_seq, v->rsv_ = 0;
		for (j = first[i]; j < first[i + 1]; ++j) {
			const int k = want_k[roff[i] + (j - first[i])];
			if ((rc = bmh_st_record(&rv, &results[j], &regs[i].a[k], reg_mapq[roff[i] + k], s->l_seq, cigar_pool, &alns[j]))) goto done;
		}
	}
	for (i = 0; i < n; i += nr) { /* the per-unit rule */
		const int32_t *const wk[2] = {want_k + roff[i], pe ? want_k + roff[i + 1] : 0};
		const bmh_alnreg_t *const ra[2] = {regs[i].a, pe ? regs[i + 1].a : 0};
		bmh_st_unit(o->flag, bns->l_pac, pes, pe, pe ? &pd[i >> 1] : 0, first + i, wk, ra, alns, plan + i);
	}
	for (i = 0, off[0] = 0; i < n; ++i) { /* the size of every read's lines, then the same composer into slices of exactly that size */
		bmh_st_sink_t t = {0, 0, 0, 0, 0};
		bmh_st_read_text(&E, &t, &rd[i], &plan[i], (int)(first[i + 1] - first[i]), alns + first[i]);
		if (t.err) { rc = BMH_E_ARG; goto done; }
		off[i + 1] = off[i] + t.l;
	}
	if (!(buf = (char *)malloc((size_t)off[n] + 1))) { rc = BMH_E_NOMEM; goto done; }
	for (i = 0, r = 0; i < n; ++i) {
		bmh_st_sink_t t = {buf + off[i], 0, off[i + 1] - off[i], 0, 0};
		r += bmh_st_read_text(&E, &t, &rd[i], &plan[i], (int)(first[i + 1] - first[i]), alns + first[i]);
		if (t.err || t.l != t.cap) { rc = BMH_E_ARG; goto done; } /* (cannot happen: the same records, the same composer) */
	}
	if (r != lines) { rc = BMH_E_ARG; goto done; } /* (cannot happen) */
	memcpy(text_off, off, sizeof(int64_t) * ((size_t)n + 1));
	*text = buf, buf = 0;
done:
	free(first), free(off), free(noff), free(npool), free(rd), free(alns), free(plan), free(buf);
	return rc;
}

/* pass A behind the context's switch (csrc/api.hip): bmh_decide_device while bmh_ctx_set_decide_device is on, falling back to
 * bmh_decide_batch where that answers BMH_E_RANGE; bmh_decide_batch otherwise */
void bmh_decide_stats_reset_(bmh_ctx_t *ctx);
int bmh_decide_routed_(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t *pes, int64_t id0, int n, bmh_alnreg_v *regs,
                       const int64_t *roff, bmh_pairdec_t *pd, int32_t *reg_mapq, int32_t *n_want, int32_t *want_k);
/* pass B behind the context's switch (csrc/api.hip): bmh_wanted_cigar_device's work while bmh_ctx_set_wanted_device is on, else
 * bmh_wanted_host_ above; *cig / *md are malloc'd */
int bmh_wanted_routed_(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads, const bmh_alnreg_v *regs,
                       const int64_t *roff, const int32_t *n_want, const int32_t *want_k, int64_t n_w, bmh_wanted_res_t *wr, uint32_t **cig, char **md);

/* pass A and pass B as one device session behind the context's switch (csrc/api.hip): with bmh_ctx_set_phase2_device on, *done = 1 and
 * bmh_phase2_device's outputs, *wr / *cig / *md malloc'd; *done = 0 with the switch off, and for a slice whose tables the call refuses
 * before its upload (BMH_E_RANGE), which then goes through the two hooks above */
int bmh_phase2_routed_(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes, int64_t id0, int n,
                       const bmh_read_t *reads, bmh_alnreg_v *regs, const int64_t *roff, bmh_pairdec_t *pd, int32_t *reg_mapq, int32_t *n_want,
                       int32_t *want_k, int64_t *n_w, bmh_wanted_res_t **wr, uint32_t **cig, char **md, int *done);
/* pass C behind the context's switch (csrc/api.hip): bmh_sam_text_device while bmh_ctx_set_samtext_device is on, else
 * bmh_sam_text_batch above; *text is malloc'd */
int bmh_samtext_routed_(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs,
                        const bmh_alnreg_v *regs, const int64_t *roff, const bmh_pairdec_t *pd, const int32_t *reg_mapq, const int32_t *n_want,
                        const int32_t *want_k, const bmh_wanted_res_t *wr, const uint32_t *cig, const char *md, const char *rg_id, char **text,
                        int64_t *text_off);

/* all three passes as one device session behind the context's switch (csrc/api.hip): with bmh_ctx_set_phase2_text_device on, *done = 1
 * and bmh_phase2_text_device's text, *text malloc'd, the vectors untouched; *done = 0 with the switch off, and for a slice the call
 * refuses before its upload (BMH_E_RANGE), which then goes through the hooks above whatever the other switches say */
int bmh_phase2_text_routed_(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes, int64_t id0, int n,
                            const bmh_seq_t *seqs, const bmh_alnreg_v *regs, const char *rg_id, char **text, int64_t *text_off, int *done);

int bmh_sam_batch(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes,
                  int64_t id0, int n, bmh_seq_t *seqs, bmh_alnreg_v *regs, const char *rg_id)
{
	const int pe = (o->flag & BMH_MEM_F_PE) != 0;
	const int64_t l_pac = bns ? bns->l_pac : 0;
	bmh_wanted_res_t *wr = 0; /* the wanted regions, in want order: final coordinates and alignments */
	int64_t n_w = 0;
	bmh_pairdec_t *pd = 0;
	int64_t *roff = 0, *text_off = 0;
	int32_t *reg_mapq = 0, *n_want = 0, *want_k = 0;
	bmh_read_t *reads = 0;
	uint32_t *cig = 0;
	char *md = 0, *text = 0;
	int i, rc = BMH_OK, fused = 0, texted = 0;
	const int trace = getenv("BMH_DRIVER_TRACE") != 0;
	double tt[4] = {0, 0, 0, 0};

	bmh_decide_stats_reset_(ctx);
	if (!ctx || !o || !bns || !pac || n < 0 || (n > 0 && (!seqs || !regs)) || (pe && ((n & 1) || !pes))) return BMH_E_ARG;
	if (n == 0) return BMH_OK;
	reads = (bmh_read_t *)malloc(sizeof(bmh_read_t) * (size_t)n);
	roff = (int64_t *)malloc(sizeof(int64_t) * ((size_t)n + 1));
	n_want = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
	if (pe) pd = (bmh_pairdec_t *)calloc((size_t)(n >> 1), sizeof(bmh_pairdec_t));
	if (!reads || !roff || !n_want || (pe && !pd)) { rc = BMH_E_NOMEM; goto done; }
	for (i = 0; i < n; ++i) reads[i].l_seq = seqs[i].l_seq, reads[i].seq = (const uint8_t *)seqs[i].seq;
	for (i = 0, roff[0] = 0; i < n; ++i) {
		if (regs[i].n && !regs[i].a) { rc = BMH_E_ARG; goto done; }
		roff[i + 1] = roff[i] + (int64_t)regs[i].n;
	}
	text_off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)n + 1));
	if (!text_off) { rc = BMH_E_NOMEM; goto done; }

	if (trace) tt[0] = now_s();
	/* ---- all three passes as one device session (bmh_phase2_text_device behind the context's switch): only the text comes back, and the
	 * vectors stay as they came */
	if ((rc = bmh_phase2_text_routed_(ctx, o, bns, pac, pes, id0, n, seqs, regs, rg_id, &text, text_off, &texted))) goto done;
	if (texted) {
		if (trace) tt[1] = tt[2] = now_s();
		goto strings;
	}
	reg_mapq = (int32_t *)malloc(sizeof(int32_t) * ((size_t)roff[n] + 1));
	want_k = (int32_t *)malloc(sizeof(int32_t) * ((size_t)roff[n] + 1));
	if (!reg_mapq || !want_k) { rc = BMH_E_NOMEM; goto done; }
	/* ---- pass A and pass B as one device session (bmh_phase2_device behind the context's switch): its want list and records go to
	 * pass C as they are */
	if ((rc = bmh_phase2_routed_(ctx, o, bns, pac, pes, id0, n, reads, regs, roff, pd, reg_mapq, n_want, want_k, &n_w, &wr, &cig, &md, &fused))) goto done;
	/* ---- pass A: decisions (bmh_decide_batch, or bmh_decide_device behind the context's switch) */
	if (!fused) {
		if ((rc = bmh_decide_routed_(ctx, o, l_pac, pes, id0, n, regs, roff, pd, reg_mapq, n_want, want_k))) goto done;
		for (i = 0; i < n; ++i) n_w += n_want[i];
	}

	if (trace) tt[1] = now_s();
	/* ---- pass B: bwa_fix_xref2 (bwa.c:179-222), then the alignments: bmh_wanted_cigar_batch's work, or with
	 * bmh_ctx_set_wanted_device on bmh_wanted_cigar_device's (the same records either way) */
	if (n_w && !fused) {
		wr = (bmh_wanted_res_t *)malloc(sizeof(*wr) * (size_t)n_w);
		if (!wr) { rc = BMH_E_NOMEM; goto done; }
		if ((rc = bmh_wanted_routed_(ctx, bns, pac, o->w, n, reads, regs, roff, n_want, want_k, n_w, wr, &cig, &md))) goto done;
	}

	if (trace) tt[2] = now_s();
	/* ---- pass C: mem_reg2aln's second half (bwamem.c:1203-1235) for every wanted region, then the text: bmh_sam_text_batch, or with
	 * bmh_ctx_set_samtext_device on bmh_sam_text_device (the same bytes either way); then one string per read */
	if ((rc = bmh_samtext_routed_(ctx, o, bns, pes, n, seqs, regs, roff, pd, reg_mapq, n_want, want_k, wr, cig, md, rg_id, &text, text_off))) goto done;
strings:
	if ((rc = bmh_sam_cut(n, seqs, text, text_off))) goto done; /* host/samcut_core.h: all or nothing */
	if (trace)
		fprintf(stderr, "[bwamem_hip] bmh_sam_batch %d reads, %zu alignments: marking + pairing %.1f ms, global alignments (bmh_reg2cigar_batch) %.1f ms, coordinates + text %.1f ms\n",
		        n, (size_t)n_w, (tt[1] - tt[0]) * 1e3, (tt[2] - tt[1]) * 1e3, (now_s() - tt[2]) * 1e3);
	if (trace) { /* what this slice's device sessions of phase 2 moved (each switch's statistics are this call's while it is on, -1 otherwise) */
		bmh_phase2_stats_t p2;
		bmh_samtext_stats_t sx;
		bmh_phase2_text_stats_t pt;
		long long up = 0, down = 0, waits = 0;
		if (bmh_last_phase2_stats(ctx, &p2) == BMH_OK && p2.h2d_bytes > 0) up += p2.h2d_bytes, down += p2.d2h_bytes, waits += p2.waits;
		if (bmh_last_samtext_stats(ctx, &sx) == BMH_OK && sx.h2d_bytes > 0) up += sx.h2d_bytes, down += sx.d2h_bytes, waits += sx.waits;
		if (bmh_last_phase2_text_stats(ctx, &pt) == BMH_OK && pt.h2d_bytes > 0) up += pt.h2d_bytes, down += pt.d2h_bytes, waits += pt.waits;
		if (waits) fprintf(stderr, "[bwamem_hip] bmh_sam_batch %d reads: phase 2 device sessions moved %lld bytes up, %lld bytes down, %lld waits\n", n, up, down, waits);
	}
done:
	free(wr), free(pd), free(reads), free(cig), free(md), free(roff), free(reg_mapq), free(n_want), free(want_k), free(text), free(text_off);
	return rc;
}
