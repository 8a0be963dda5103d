/*
 * matesw_core_main.c -- stand-alone check of host/matesw_core.h (over host/dedup_core.h) for a plain and a sanitizer build:
 * tests/test_matesw_core_cpu.py compiles it with gcc, links the oracle (liborc.so) and runs it as a child process.
 *
 * It drives the shared routines exactly as the device loop of csrc/matesw.hip does -- per round and unfinished pair FOLD as far as
 * the previous round's results reach, then PLAN and append the tasks; then the round's ksw_align2 calls, for which the oracle's
 * orc_sw_batch stands in for launch_sw (BMH_F_TPAC tasks, given the pac) -- until no pair is unfinished.
 * Every vector lives in a heap block of exactly its slice capacity (n + 4 * candidate hits of the other end) and every range
 * stack in a heap block of exactly bmh_sort_stack_len(n) entries, so an access past either is the sanitizer's to report.
 *
 * Input file (little endian, written by the test):
 *   int32 n_cases
 *   per case: bmh_params_t, bmh_matesw_opt_t, bmh_pestat_t[4], float mask_level_redun, int32 mode, int64 l_pac, int32 pac_bytes, pac,
 *             int32 n_pairs, per read (2 per pair) int32 l_seq and its base codes, per vector int32 n and its records
 *     mode 0: per vector int32 n and the expected records, per pair int32 n_sw (a recorded fixture)
 *     mode 1: nothing more: the expectation is orc_matesw_pair's, given bmh_dedup_core as its mem_sort_and_dedup
 * Output: per case one line "case C: P pairs, A active, R rounds, T tasks, E empty-window plans, N no-call plans, S needed-after-all
 * stops, D differ".  Exit status 0: every case reproduced its expectation record for record.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/matesw_core.h"
#include "../bwa-mem-quickassist_amd/host/dedup_core.h"
#include "../oracle/matesw_oracle.h"
#include "../oracle/sw_oracle.h"

static int rd(void *p, size_t sz, size_t n, FILE *f) { return n == 0 || fread(p, sz, n, f) == n; }

static int dedup_exact(void *user, int n, bmh_alnreg_t *a) /* bmh_dedup_core over a range stack of exactly the stated length */
{
	bmh_sort_stk_t *stk = (bmh_sort_stk_t *)malloc(sizeof(*stk) * bmh_sort_stack_len((size_t)n));
	int m;
	if (!stk) exit(2);
	m = bmh_dedup_core(n, a, *(const float *)user, stk);
	free(stk);
	return m;
}

typedef struct {
	bmh_alnreg_t *b[2], *a[2];
	int nb[2], n[2], cap[2];
	uint64_t read_off[2];
	bmh_msw_pair_t s;
} pair_t;

static int n_hits(const bmh_alnreg_v *v, const bmh_matesw_opt_t *o) /* |b[i]| of bwamem_pair.c:252-259 */
{
	size_t j;
	int nb = 0;
	for (j = 0; j < v->n && nb < o->max_matesw; ++j) nb += v->a[j].score >= v->a[0].score - o->pen_unpaired;
	return nb;
}

static void view(const pair_t *ps, const bmh_read_t *reads, bmh_msw_io_t *io)
{
	int i;
	for (i = 0; i < 2; ++i) {
		io->b[i] = ps->b[i], io->nb[i] = ps->nb[i];
		io->a[i] = ps->a[i], io->n[i] = ps->n[i], io->cap[i] = ps->cap[i];
		io->l_seq[i] = reads[i].l_seq;
	}
}

int main(int argc, char **argv)
{
	FILE *f;
	int32_t n_cases, c;
	int bad_total = 0;
	if (argc != 2 || !(f = fopen(argv[1], "rb"))) {
		fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
		return 2;
	}
	if (!rd(&n_cases, 4, 1, f)) return 2;
	for (c = 0; c < n_cases; ++c) {
		bmh_params_t P;
		bmh_matesw_opt_t o;
		bmh_pestat_t pes[4];
		float level;
		int32_t mode, pac_bytes, n_pairs, k, p, q, n_act = 0;
		int64_t l_pac;
		uint8_t *pac, *pool;
		bmh_read_t *reads;
		bmh_alnreg_v *regs, *want;
		int32_t *want_n, *act;
		pair_t *ps;
		bmh_sw_task_t *tasks;
		bmh_sw_result_t *res;
		size_t bytes = 0;
		uint32_t n_res = 0;
		long rounds = 0, n_tasks = 0, n_empty = 0, n_nocall = 0, n_needed = 0, launches = 0;
		int bad = 0;
		const bmh_msw_dedup_t dd = {dedup_exact, &level, 0.f, 0};
		if (!rd(&P, sizeof(P), 1, f) || !rd(&o, sizeof(o), 1, f) || !rd(pes, sizeof(pes), 1, f) || !rd(&level, 4, 1, f) || !rd(&mode, 4, 1, f) ||
		    !rd(&l_pac, 8, 1, f) || !rd(&pac_bytes, 4, 1, f) || pac_bytes < 0)
			return 2;
		pac = (uint8_t *)malloc((size_t)pac_bytes + 1);
		if (!pac || !rd(pac, 1, (size_t)pac_bytes, f) || !rd(&n_pairs, 4, 1, f) || n_pairs < 0) return 2;
		reads = (bmh_read_t *)calloc((size_t)2 * n_pairs + 1, sizeof(*reads));
		regs = (bmh_alnreg_v *)calloc((size_t)2 * n_pairs + 1, sizeof(*regs));
		want = (bmh_alnreg_v *)calloc((size_t)2 * n_pairs + 1, sizeof(*want));
		want_n = (int32_t *)calloc((size_t)n_pairs + 1, sizeof(*want_n));
		act = (int32_t *)calloc((size_t)n_pairs + 1, sizeof(*act));
		if (!reads || !regs || !want || !want_n || !act) return 2;
		for (k = 0; k < 2 * n_pairs; ++k) {
			if (!rd(&reads[k].l_seq, 4, 1, f) || reads[k].l_seq < 0) return 2;
			reads[k].seq = (uint8_t *)malloc((size_t)reads[k].l_seq + 1);
			if (!reads[k].seq || !rd((void *)reads[k].seq, 1, (size_t)reads[k].l_seq, f)) return 2;
		}
		for (k = 0; k < 2 * n_pairs; ++k) {
			int32_t n;
			if (!rd(&n, 4, 1, f) || n < 0) return 2;
			regs[k].n = regs[k].m = (size_t)n;
			regs[k].a = (bmh_alnreg_t *)malloc(sizeof(bmh_alnreg_t) * (size_t)n + 1);
			if (!regs[k].a || !rd(regs[k].a, sizeof(bmh_alnreg_t), (size_t)n, f)) return 2;
		}
		if (mode == 0) {
			for (k = 0; k < 2 * n_pairs; ++k) {
				int32_t n;
				if (!rd(&n, 4, 1, f) || n < 0) return 2;
				want[k].n = want[k].m = (size_t)n;
				want[k].a = (bmh_alnreg_t *)malloc(sizeof(bmh_alnreg_t) * (size_t)n + 1);
				if (!want[k].a || !rd(want[k].a, sizeof(bmh_alnreg_t), (size_t)n, f)) return 2;
			}
			if (!rd(want_n, 4, (size_t)n_pairs, f)) return 2;
		} else
			for (p = 0; p < n_pairs; ++p) { /* the oracle, on copies the oracle may realloc */
				for (k = 2 * p; k < 2 * p + 2; ++k) {
					want[k].n = want[k].m = regs[k].n;
					want[k].a = (bmh_alnreg_t *)malloc(sizeof(bmh_alnreg_t) * regs[k].n + 1);
					if (!want[k].a) return 2;
					memcpy(want[k].a, regs[k].a, sizeof(bmh_alnreg_t) * regs[k].n);
				}
				want_n[p] = orc_matesw_pair(&P, &o, l_pac, pac, pes, reads + 2 * p, want + 2 * p, dedup_exact, &level);
			}

		/* ---- the drivers' pre-filter: pairs with a candidate hit whose mem_matesw would not return at bwamem_pair.c:122 */
		for (p = 0; p < n_pairs; ++p) {
			int i, busy = 0;
			for (i = 0; i < 2 && !busy; ++i) {
				const bmh_alnreg_v *a = &regs[2 * p + i], *ma = &regs[2 * p + !i];
				size_t j;
				int nb = 0, skip[4];
				for (j = 0; j < a->n && !busy; ++j) {
					if (a->a[j].score < a->a[0].score - o.pen_unpaired) continue;
					if (nb++ >= o.max_matesw) break;
					if (bmh_msw_skip(l_pac, pes, a->a[j].rb, ma->a, (int32_t)ma->n, skip) != 4) busy = 1;
				}
			}
			if (busy) act[n_act++] = p;
		}
		/* ---- what the device driver uploads: slices of exactly their capacity, the candidate hits, the reads as the pool */
		ps = (pair_t *)calloc((size_t)n_act + 1, sizeof(*ps));
		if (!ps) return 2;
		for (q = 0; q < n_act; ++q) {
			int i;
			p = act[q];
			for (i = 0; i < 2; ++i) {
				const bmh_alnreg_v *v = &regs[2 * p + i];
				pair_t *s = &ps[q];
				size_t j;
				s->cap[i] = (int)v->n + 4 * n_hits(&regs[2 * p + !i], &o), s->n[i] = (int)v->n;
				s->a[i] = (bmh_alnreg_t *)malloc(sizeof(bmh_alnreg_t) * (size_t)s->cap[i]); /* (malloc(0) may be NULL: nothing is ever written then) */
				s->b[i] = (bmh_alnreg_t *)malloc(sizeof(bmh_alnreg_t) * (size_t)n_hits(v, &o));
				if ((s->cap[i] && !s->a[i]) || (n_hits(v, &o) && !s->b[i])) return 2;
				if (v->n) memcpy(s->a[i], v->a, sizeof(bmh_alnreg_t) * v->n);
				for (j = 0; j < v->n && s->nb[i] < o.max_matesw; ++j)
					if (v->a[j].score >= v->a[0].score - o.pen_unpaired) s->b[i][s->nb[i]++] = v->a[j];
				s->read_off[i] = bytes, bytes += (size_t)reads[2 * p + i].l_seq;
			}
		}
		pool = (uint8_t *)calloc(bytes + 16, 1);
		tasks = (bmh_sw_task_t *)malloc(sizeof(*tasks) * ((size_t)n_act * 4 * BMH_MSW_LOOKAHEAD + 1));
		res = (bmh_sw_result_t *)malloc(sizeof(*res) * ((size_t)n_act * 4 * BMH_MSW_LOOKAHEAD + 1));
		if (!pool || !tasks || !res) return 2;
		for (q = 0; q < n_act; ++q)
			for (k = 0; k < 2; ++k) memcpy(pool + ps[q].read_off[k], reads[2 * act[q] + k].seq, (size_t)reads[2 * act[q] + k].l_seq);
		/* ---- the device loop */
		for (;; ++launches) {
			uint32_t appended = 0;
			int unfinished = 0;
			if (launches > 4L * (o.max_matesw > 0 ? o.max_matesw : 0) + 4) {
				fprintf(stderr, "case %d: no end after %ld launches\n", c, launches);
				return 1;
			}
			for (q = 0; q < n_act; ++q) { /* msw_round_kernel, lane q */
				pair_t *s = &ps[q];
				bmh_msw_io_t io;
				int code, v, r;
				if (s->s.done) continue;
				view(s, reads + 2 * act[q], &io);
				do code = bmh_msw_fold_step(l_pac, pes, o.min_seed_len, &io, &s->s, res, n_res, &dd);
				while (code == BMH_MSW_FOLDED);
				s->n[0] = io.n[0], s->n[1] = io.n[1];
				if (code == BMH_MSW_FULL || code == BMH_MSW_BAD) {
					fprintf(stderr, "case %d pair %d: fold answers %d (a slice too small, or a plan past the results)\n", c, act[q], code);
					return 1;
				}
				if (code == BMH_MSW_DONE) continue;
				n_needed += code == BMH_MSW_STOP_NEEDED;
				bmh_msw_plan(l_pac, pes, &io, &s->s, 0);
				for (v = 0; v < s->s.n_inv; ++v) {
					bmh_msw_inv_t *e = &s->s.inv[v];
					for (r = 0; r < 4; ++r) {
						n_empty += e->plan[r] == BMH_MSW_EMPTY, n_nocall += e->plan[r] == BMH_MSW_NOCALL;
						if (e->plan[r] != BMH_MSW_CALL) continue;
						bmh_msw_task(P.a, o.min_seed_len, reads[2 * act[q] + !e->i].l_seq, r, s->read_off[!e->i], e->rb[r], e->re[r], &tasks[appended]);
						e->plan[r] = (int32_t)++appended;
					}
				}
				++unfinished;
			}
			n_res = appended;
			if (!unfinished) break;
			if (appended) {
				int64_t cells;
				++rounds, n_tasks += appended;
				if (orc_sw_batch(&P, pool, pac, l_pac, tasks, (int)appended, res, &cells, 1)) {
					fprintf(stderr, "case %d: the oracle refuses the round's tasks\n", c);
					return 1;
				}
			}
		}
		/* ---- record for record */
		for (p = 0, q = 0; p < n_pairs; ++p) {
			const int active = q < n_act && act[q] == p;
			for (k = 0; k < 2; ++k) {
				const bmh_alnreg_t *got = active ? ps[q].a[k] : regs[2 * p + k].a;
				const size_t n = active ? (size_t)ps[q].n[k] : regs[2 * p + k].n;
				if (n != want[2 * p + k].n || (n && memcmp(got, want[2 * p + k].a, sizeof(bmh_alnreg_t) * n))) {
					if (bad++ < 5) fprintf(stderr, "case %d pair %d end %d: %zu regions, expected %zu, or other records\n", c, p, k, n, want[2 * p + k].n);
				}
			}
			if ((active ? ps[q].s.n : 0) != want_n[p]) {
				if (bad++ < 5) fprintf(stderr, "case %d pair %d: n_sw %d, expected %d\n", c, p, active ? ps[q].s.n : 0, want_n[p]);
			}
			q += active;
		}
		printf("case %d: %d pairs, %d active, %ld rounds, %ld tasks, %ld empty-window plans, %ld no-call plans, %ld needed-after-all stops, %d differ\n", c,
		       n_pairs, n_act, rounds, n_tasks, n_empty, n_nocall, n_needed, bad);
		bad_total += bad;
		for (q = 0; q < n_act; ++q) free(ps[q].a[0]), free(ps[q].a[1]), free(ps[q].b[0]), free(ps[q].b[1]);
		for (k = 0; k < 2 * n_pairs; ++k) free((void *)reads[k].seq), free(regs[k].a), free(want[k].a);
		free(ps), free(pool), free(tasks), free(res), free(reads), free(regs), free(want), free(want_n), free(act), free(pac);
	}
	fclose(f);
	return bad_total ? 1 : 0;
}
