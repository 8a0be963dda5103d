/*
 * matesw_batch.c -- batched mate rescue: the loop of mem_sam_pe (reference bwa-0.7.8/bwamem_pair.c:251-263) over
 * mem_matesw (bwamem_pair.c:109-175) for a whole chunk of read pairs, its ksw_align2 calls run as GPU batches.
 *
 * What is sequential in the reference stays sequential here: every mem_matesw invocation first tests the four
 * orientations against the CURRENT content of the mate's region vector (:112-121), which earlier invocations of the
 * same pair may have changed.  So each pair is a small resumable machine {end i, hit j}; a ROUND plans, per unfinished
 * pair, its next few invocations that need Smith-Waterman (up to four ksw_align2 calls each: skip[] is fixed at
 * :112-121), runs all of them in one bmh_sw_batch, and folds the results in the reference's order (:150-166 insert,
 * :168 mem_sort_and_dedup after every orientation), re-deriving skip[] from the then-current vector before each
 * invocation.  The first planned invocation of a pair is never speculative; the ones planned ahead may turn out to be
 * skipped (their ksw_align2 results are then simply not used) -- the outcome is exactly the reference's.
 *
 * Sequences: the pool holds the reads of the pairs that need rescue, once each.  A reverse-complemented mate (:130-133) is BMH_F_QREV|BMH_F_QCOMP; with
 * the reference resident on the device the window bns_get_seq would return (:143) is a BMH_F_TPAC task, otherwise it
 * is decoded on the host into the round's pool.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/bwamem_hip.h"

const bmh_params_t *bmh_ctx_params_(const bmh_ctx_t *ctx);
int bmh_ctx_has_pac_(const bmh_ctx_t *ctx, const uint8_t *pac, int64_t l_pac);
void bmh_ctx_set_driver_stats_(bmh_ctx_t *ctx, const bmh_driver_stats_t *st);

#include "matesw_core.h" /* the rules both drivers share: skip test, windows, tasks, regions, planning, folding */

typedef struct {
	bmh_alnreg_t *b[2]; /* hits of each end within pen_unpaired of its best, the first max_matesw of them, copied up front (bwamem_pair.c:252-259) */
	int nb[2];
	bmh_msw_pair_t s;
} pair_t;

static void fetch_window(int64_t l_pac, const uint8_t *pac, int64_t beg, int64_t end, uint8_t *dst) /* bntseq.c:355-376 */
{
	int64_t k, l = 0;
	if (beg >= l_pac) {
		const int64_t lo = (l_pac << 1) - 1 - end, hi = (l_pac << 1) - 1 - beg;
		for (k = hi; k > lo; --k) dst[l++] = (uint8_t)(3 - (pac[k >> 2] >> ((~k & 3) << 1) & 3));
	} else
		for (k = beg; k < end; ++k) dst[l++] = (uint8_t)(pac[k >> 2] >> ((~k & 3) << 1) & 3);
}

/* pair q as matesw_core.h sees it, over the caller's vectors as they are now */
static void view(const pair_t *ps, const bmh_read_t *reads, bmh_alnreg_v *regs, bmh_msw_io_t *io)
{
	int i;
	for (i = 0; i < 2; ++i) {
		io->b[i] = ps->b[i], io->nb[i] = ps->nb[i];
		io->a[i] = regs[i].a, io->n[i] = (int32_t)regs[i].n, io->cap[i] = (int32_t)regs[i].m;
		io->l_seq[i] = reads[i].l_seq;
	}
}

int bmh_matesw_batch(bmh_ctx_t *ctx, int64_t l_pac, const uint8_t *pac, int n_pairs, const bmh_read_t *reads,
                     bmh_alnreg_v *regs, const bmh_pestat_t pes[4], const bmh_matesw_opt_t *o, bmh_dedup_fn dedup,
                     void *dedup_user, int *n_sw)
{
	const bmh_params_t *P;
	pair_t *ps = 0;
	uint64_t *read_off = 0; /* pool offsets of the two reads of each ACTIVE pair */
	int *act = 0, n_act = 0, q;
	uint8_t *pool = 0;
	bmh_sw_task_t *tasks = 0;
	bmh_sw_result_t *res = 0;
	size_t reads_bytes = 0, pool_cap = 0, task_cap = 0;
	int p, r, rc = BMH_OK, tpac, first_round = 1;
	bmh_driver_stats_t st;
	memset(&st, 0, sizeof(st));

	if (!ctx || !pac || !reads || !regs || !pes || !o || !dedup || n_pairs < 0 || l_pac <= 0) return BMH_E_ARG;
	if (!(P = bmh_ctx_params_(ctx))) return BMH_E_ARG;
	if (n_pairs == 0) return BMH_OK;
	tpac = bmh_ctx_has_pac_(ctx, pac, l_pac);
	/* Most pairs need no rescue at all: every candidate hit already has a properly placed mate, so each of its
	 * mem_matesw calls returns at bwamem_pair.c:122 and nothing ever changes.  Whether that is so can be read off the
	 * vectors as phase 1 left them (the first call that does NOT return there is the first that could change anything),
	 * so only the other pairs -- a few per cent -- get a machine, copies of their candidate hits, and room in the pool. */
	act = (int *)malloc(sizeof(int) * (size_t)n_pairs);
	if (!act) { rc = BMH_E_NOMEM; goto done; }
	for (p = 0; p < n_pairs; ++p) {
		int i, busy = 0;
		for (i = 0; i < 2 && !busy; ++i) {
			const bmh_alnreg_v *a = &regs[2 * p + i], *ma = &regs[2 * p + !i];
			size_t j;
			int nb = 0;
			for (j = 0; j < a->n && !busy; ++j) { /* the hits copied to b[i] (:252-257), the first max_matesw of them (:258-259) */
				int skip[4];
				if (a->a[j].score < a->a[0].score - o->pen_unpaired) continue;
				if (nb++ >= o->max_matesw) break;
				if (bmh_msw_skip(l_pac, pes, a->a[j].rb, ma->a, (int32_t)ma->n, skip) != 4) busy = 1;
			}
		}
		if (busy) act[n_act++] = p;
	}
	if (n_sw) memset(n_sw, 0, sizeof(int) * (size_t)n_pairs);
	if (n_act == 0) goto done;
	ps = (pair_t *)calloc((size_t)n_act, sizeof(pair_t));
	read_off = (uint64_t *)malloc(sizeof(uint64_t) * 2 * (size_t)n_act);
	if (!ps || !read_off) { rc = BMH_E_NOMEM; goto done; }
	for (q = 0; q < n_act; ++q) {
		int i;
		size_t j;
		p = act[q];
		for (i = 0; i < 2; ++i) {
			const bmh_alnreg_v *a = &regs[2 * p + i];
			if (reads[2 * p + i].l_seq < 1 || reads[2 * p + i].l_seq > 65535) { rc = BMH_E_RANGE; goto done; }
			read_off[2 * q + i] = reads_bytes, reads_bytes += (size_t)reads[2 * p + i].l_seq;
			if (a->n && o->max_matesw > 0 && !(ps[q].b[i] = (bmh_alnreg_t *)malloc(sizeof(bmh_alnreg_t) * (a->n < (size_t)o->max_matesw ? a->n : (size_t)o->max_matesw)))) {
				rc = BMH_E_NOMEM;
				goto done;
			}
			for (j = 0; j < a->n && ps[q].nb[i] < o->max_matesw; ++j) /* bwamem_pair.c:252-259 */
				if (a->a[j].score >= a->a[0].score - o->pen_unpaired) ps[q].b[i][ps[q].nb[i]++] = a->a[j];
		}
	}

	for (;;) {
		size_t n_tasks = 0, win_bytes = 0, used, want_tasks = 0;
		int active = 0;
		/* ---- plan (bmh_msw_plan): from each unfinished pair's cursor on, the next invocations that (as things stand) need
		 * ksw_align2, the later ones planned ahead.  Without this, a pair with h candidate hits would cost h GPU round trips. */
		for (q = 0; q < n_act; ++q) {
			bmh_msw_io_t io;
			uint64_t wb;
			p = act[q];
			if (ps[q].s.done) continue;
			view(&ps[q], reads + 2 * p, regs + 2 * p, &io);
			want_tasks += (size_t)bmh_msw_plan(l_pac, pes, &io, &ps[q].s, &wb);
			win_bytes += (size_t)wb;
			++active;
		}
		if (!active) break;

		/* ---- build the round's tasks (and, without a resident reference, its windows) */
		if (want_tasks > task_cap) {
			task_cap = want_tasks + want_tasks / 2 + 64;
			free(tasks), free(res);
			tasks = (bmh_sw_task_t *)malloc(sizeof(bmh_sw_task_t) * task_cap);
			res = (bmh_sw_result_t *)malloc(sizeof(bmh_sw_result_t) * task_cap);
			if (!tasks || !res) { rc = BMH_E_NOMEM; goto done; }
		}
		used = reads_bytes;
		if (first_round || !tpac) {
			const size_t need_bytes = reads_bytes + (tpac ? 0 : win_bytes) + 16;
			if (need_bytes > pool_cap) {
				pool_cap = need_bytes + need_bytes / 2;
				free(pool);
				if (!(pool = (uint8_t *)malloc(pool_cap))) { rc = BMH_E_NOMEM; goto done; }
				first_round = 1;
			}
			if (first_round)
				for (q = 0; q < n_act; ++q) {
					memcpy(pool + read_off[2 * q], reads[2 * act[q]].seq, (size_t)reads[2 * act[q]].l_seq);
					memcpy(pool + read_off[2 * q + 1], reads[2 * act[q] + 1].seq, (size_t)reads[2 * act[q] + 1].l_seq);
				}
		}
		for (q = 0; q < n_act; ++q) {
			bmh_msw_pair_t *s = &ps[q].s;
			int v;
			p = act[q];
			if (s->done) continue;
			for (v = 0; v < s->n_inv; ++v) {
				bmh_msw_inv_t *e = &s->inv[v];
				const int mate = 2 * q + !e->i, l_ms = reads[2 * p + !e->i].l_seq; /* `mate` indexes read_off */
				for (r = 0; r < 4; ++r) {
					bmh_sw_task_t *t;
					if (e->plan[r] != BMH_MSW_CALL) continue;
					t = &tasks[n_tasks];
					bmh_msw_task(P->a, o->min_seed_len, l_ms, r, read_off[mate], e->rb[r], e->re[r], t);
					if (!tpac) { /* the window decoded on the host, behind the reads */
						fetch_window(l_pac, pac, e->rb[r], e->re[r], pool + used);
						t->t_off = used, used += (size_t)(e->re[r] - e->rb[r]), t->flags &= (uint16_t)~BMH_F_TPAC;
					}
					e->plan[r] = (int32_t)n_tasks + 1; /* 1-based index of its result */
					++n_tasks;
				}
			}
		}
		if (n_tasks) {
			++st.rounds, st.ext_tasks += (int64_t)n_tasks; /* here: GPU rounds and ksw_align2 calls */
			memset(pool + used, 0, 16);
			if (first_round || !tpac) {
				st.pool_bytes += (int64_t)used + 16;
				if ((rc = bmh_upload_pool(ctx, pool, used + 16))) goto done;
				first_round = 0;
			}
			if ((rc = bmh_sw_batch(ctx, 0, 0, tasks, (int64_t)n_tasks, res))) goto done;
		}

		/* ---- fold (bmh_msw_fold_step), invocation by invocation in the reference's order, as far as the planned results reach */
		for (q = 0; q < n_act; ++q) {
			const bmh_msw_dedup_t dd = {dedup, dedup_user, 0.f, 0};
			p = act[q];
			if (ps[q].s.done) continue;
			for (;;) {
				bmh_msw_io_t io;
				int c;
				view(&ps[q], reads + 2 * p, regs + 2 * p, &io);
				c = bmh_msw_fold_step(l_pac, pes, o->min_seed_len, &io, &ps[q].s, res, (uint32_t)n_tasks, &dd);
				regs[2 * p].n = (size_t)io.n[0], regs[2 * p + 1].n = (size_t)io.n[1];
				if (c == BMH_MSW_FULL) { /* kv_push's growth (kvec.h:68-74) until the invocation's regions fit */
					bmh_alnreg_v *ma = &regs[2 * p + !ps[q].s.i];
					bmh_alnreg_t *na;
					size_t m = ma->m;
					while (m < ma->n + 4) m = m ? m << 1 : 2;
					if (!(na = (bmh_alnreg_t *)realloc(ma->a, sizeof(bmh_alnreg_t) * m))) { rc = BMH_E_NOMEM; goto done; }
					ma->a = na, ma->m = m;
				} else if (c == BMH_MSW_BAD) {
					rc = BMH_E_ARG;
					goto done;
				} else if (c != BMH_MSW_FOLDED) break;
			}
		}
	}
	if (n_sw)
		for (q = 0; q < n_act; ++q) n_sw[act[q]] = ps[q].s.n;
done:
	bmh_ctx_set_driver_stats_(ctx, &st);
	if (ps)
		for (q = 0; q < n_act; ++q) free(ps[q].b[0]), free(ps[q].b[1]);
	free(ps), free(read_off), free(pool), free(tasks), free(res), free(act);
	return rc;
}
