// matesw.hip -- mate rescue on the device: the driver of bmh_matesw_batch (host/matesw_batch.c), i.e. the block of mem_sam_pe at
// reference bwa-0.7.8/bwamem_pair.c:251-263 over mem_matesw (:109-175), with the planning, the folding and mem_sort_and_dedup (:168)
// as a kernel, one lane per active pair.  The rules both drivers must agree on are one text, host/matesw_core.h.
//
//   host, before anything is enqueued   the pre-filter of the host driver (only pairs with a candidate hit whose mem_matesw would not
//                       return at :122 are active), and every refusal: a refused call uploads nothing
//   one upload          per active vector its count and its arena slice (capacity n + 4 * candidate hits of the other end: an
//                       invocation inserts at most four regions and de-duplication only shrinks), the pair records, the candidate
//                       hits b[i] of :252-259, the active pairs' reads as the pool
//   msw_round_kernel    per unfinished pair: FOLD as far as the previous round's results reach (bmh_msw_fold_step, bmh_dedup_core over the
//                       lane's own range stack), then PLAN (bmh_msw_plan) into the pair's machine and append the tasks with an atomic
//                       counter: results are addressed through the index kept in the plan, so append order never reaches the output
//   launch_sw           the round's ksw_align2 calls
//   host loop           launch the kernel, read back {tasks appended, pairs unfinished, error flag, -}: 16 bytes per round trip
//   one download        the counts, n per pair and the slices
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bmh_ctx.h"
#include "bmh_device.h"
#include "../host/matesw_core.h"

namespace bmh {

// status words (uint32 index); 0..3 are what the host reads in the loop
enum { MSW_N_TASKS = 0, MSW_N_UNFINISHED = 1, MSW_ERR = 2, MSW_STATUS_BYTES = 64 };
constexpr int kMswTasksPerPair = 4 * BMH_MSW_LOOKAHEAD; // a round's tasks of one pair at most
constexpr int kMswStk = 34;                             // bmh_sort_stack_len(n) <= 33 entries for n < 2^31, as region_dedup_kernel

struct MswPair { // one active pair, 64 bytes
	uint64_t read_off[2]; // its reads in the pool
	uint32_t slice[2];    // where its vectors' slices start in the arena ...
	int32_t cap[2];       // ... and the records they hold
	uint32_t hit[2];      // where its candidate hits start ...
	int32_t nb[2];        // ... and how many
	int32_t l_seq[2];
	int32_t rsv[2];
};
static_assert(sizeof(MswPair) == 64, "pair record");

struct MswPes {
	bmh_pestat_t r[4];
};

struct MswWs {
	uint32_t *status;
	int32_t *cnt;            // 2 per pair: the vectors' lengths, in and out
	int32_t *nsw;            // per pair: the sum of mem_matesw's return values, written when the pair is done
	bmh_alnreg_t *arena;
	const MswPair *pair;
	const bmh_alnreg_t *hits;
	bmh_msw_pair_t *state;   // the machines between launches
	bmh_sw_task_t *tasks;    // kMswTasksPerPair per pair
	bmh_sw_result_t *res;
};

__device__ __forceinline__ void msw_fail(uint32_t *status, int code) { atomicCAS((int *)&status[MSW_ERR], 0, code); }

// n_res: the tasks of the previous round, whose results lie in ws.res; sw_err: the Smith-Waterman kernels' error flag, moved into
// the status words so that one read-back carries everything
__global__ __launch_bounds__(64) void msw_round_kernel(int a, int min_seed_len, int64_t l_pac, MswPes pes, MswWs ws, int n_act, uint32_t n_res,
                                                       uint32_t task_cap, uint32_t arena_cap, uint32_t hits_cap, float mask_level_redun, int *sw_err)
{
	const int q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q == 0) {
		const int e = *sw_err;
		if (e) msw_fail(ws.status, e), *sw_err = 0;
	}
	if (q >= n_act) return;
	bmh_msw_pair_t *s = &ws.state[q];
	if (s->done) return;
	const MswPair pr = ws.pair[q];
	bmh_msw_io_t io;
	for (int i = 0; i < 2; ++i) {
		io.b[i] = ws.hits + pr.hit[i], io.nb[i] = pr.nb[i];
		io.a[i] = ws.arena + pr.slice[i], io.n[i] = ws.cnt[2 * q + i], io.cap[i] = pr.cap[i];
		io.l_seq[i] = pr.l_seq[i];
		// every access below stays inside the slice and the hits, or nothing is touched
		if (pr.cap[i] < 0 || pr.nb[i] < 0 || io.n[i] < 0 || io.n[i] > pr.cap[i] || (uint64_t)pr.slice[i] + (uint64_t)pr.cap[i] > arena_cap ||
		    (uint64_t)pr.hit[i] + (uint64_t)pr.nb[i] > hits_cap) {
			msw_fail(ws.status, BMH_E_ARG);
			s->done = 1;
			return;
		}
	}
	bmh_sort_stk_t stk[kMswStk];
	const bmh_msw_dedup_t dd = {nullptr, nullptr, mask_level_redun, stk};
	int c;
	do c = bmh_msw_fold_step(l_pac, pes.r, min_seed_len, &io, s, ws.res, n_res, &dd);
	while (c == BMH_MSW_FOLDED);
	ws.cnt[2 * q] = io.n[0], ws.cnt[2 * q + 1] = io.n[1];
	if (c == BMH_MSW_FULL || c == BMH_MSW_BAD) { // cannot happen: the slice holds four regions per invocation
		msw_fail(ws.status, BMH_E_ARG);
		s->done = 1;
		return;
	}
	if (c == BMH_MSW_DONE) {
		ws.nsw[q] = s->n;
		return;
	}
	const int want = bmh_msw_plan(l_pac, pes.r, &io, s, nullptr);
	if (want > 0) {
		const uint32_t base = atomicAdd(&ws.status[MSW_N_TASKS], (uint32_t)want);
		if ((uint64_t)base + (uint64_t)want > task_cap) { // cannot happen: kMswTasksPerPair per pair
			msw_fail(ws.status, BMH_E_ARG);
			s->done = 1;
			return;
		}
		uint32_t at = base;
		for (int v = 0; v < s->n_inv; ++v) {
			bmh_msw_inv_t *e = &s->inv[v];
			const int m = !e->i;
			for (int r = 0; r < 4; ++r) {
				if (e->plan[r] != BMH_MSW_CALL) continue;
				bmh_sw_task_t t;
				bmh_msw_task(a, min_seed_len, pr.l_seq[m], r, pr.read_off[m], e->rb[r], e->re[r], &t);
				ws.tasks[at] = t;
				e->plan[r] = (int32_t)++at; // index + 1 of its result
			}
		}
	}
	atomicAdd(&ws.status[MSW_N_UNFINISHED], 1u);
}

} // namespace bmh

using namespace bmh;

namespace {

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct MswLayout { // [status | counts, n per pair | arena | pair records | hits | pool] is what goes up, [counts .. arena] what comes down
	size_t status, out, arena, pair, hits, pool, state, tasks, res, total;
	MswLayout(size_t n_act, size_t arena_n, size_t hits_n, size_t pool_bytes)
	{
		size_t o = 0;
		auto take = [&](size_t bytes) {
			const size_t at = o;
			o += al256(bytes);
			return at;
		};
		status = take(MSW_STATUS_BYTES), out = take(n_act * 12), arena = take(arena_n * sizeof(bmh_alnreg_t)), pair = take(n_act * sizeof(MswPair));
		hits = take(hits_n * sizeof(bmh_alnreg_t)), pool = take(pool_bytes), state = take(n_act * sizeof(bmh_msw_pair_t));
		tasks = take(n_act * kMswTasksPerPair * sizeof(bmh_sw_task_t)), res = take(n_act * kMswTasksPerPair * sizeof(bmh_sw_result_t)), total = o;
	}
};

// after an error inside the enqueued section: nothing of this call is left running, and the Smith-Waterman kernels' error flag is
// clean for the next call; the error stays the answer
int msw_abandon(bmh_ctx *ctx, int rc)
{
	std::string why = std::move(ctx->last_error);
	int e = 0;
	(void)stream_wait(ctx, ctx->stream);
	if (hipMemcpyAsync(ctx->h_err, ctx->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess && stream_wait(ctx, ctx->stream) == hipSuccess)
		e = *ctx->h_err;
	if (e) {
		(void)hipMemsetAsync(ctx->d_err, 0, sizeof(int), ctx->stream);
		(void)stream_wait(ctx, ctx->stream);
	}
	ctx->last_error = std::move(why);
	return rc;
}

} // namespace

extern "C" int bmh_matesw_device(bmh_ctx_t *ctx, int64_t l_pac, int n_pairs, const bmh_read_t *reads, bmh_alnreg_v *regs, const bmh_pestat_t pes[4],
                                 const bmh_matesw_opt_t *o, float mask_level_redun, int *n_sw)
{
	if (!ctx || !reads || !regs || !pes || !o || n_pairs < 0 || l_pac <= 0) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	if (!ctx->dev.pac || ctx->dev.l_pac != l_pac) {
		ctx->last_error = "bmh_matesw_device: needs the 2-bit reference of this l_pac resident on the device (bmh_ctx_set_pac)";
		return BMH_E_ARG;
	}
	for (int k = 0; k < 2 * n_pairs; ++k)
		if (regs[k].n && !regs[k].a) return BMH_E_ARG;
	bmh_driver_stats_t st{};
	ctx->dstats = st;
	if (n_sw && n_pairs) memset(n_sw, 0, sizeof(int) * (size_t)n_pairs);
	if (n_pairs == 0) return BMH_OK;
	// ---- the host driver's pre-filter: most pairs need no rescue at all (every mem_matesw call of theirs returns at bwamem_pair.c:122)
	const int maxm = std::max(o->max_matesw, 0);
	auto n_hits = [&](const bmh_alnreg_v &v) { // |b[i]| of :252-259
		int nb = 0;
		for (size_t j = 0; j < v.n && nb < maxm; ++j) nb += v.a[j].score >= v.a[0].score - o->pen_unpaired;
		return nb;
	};
	std::vector<int> act;
	for (int p = 0; p < n_pairs; ++p) {
		bool busy = false;
		for (int i = 0; i < 2 && !busy; ++i) {
			const bmh_alnreg_v &v = regs[2 * p + i], &ma = regs[2 * p + !i];
			int nb = 0, skip[4];
			for (size_t j = 0; j < v.n && !busy; ++j) {
				if (v.a[j].score < v.a[0].score - o->pen_unpaired) continue;
				if (nb++ >= o->max_matesw) break;
				busy = bmh_msw_skip(l_pac, pes, v.a[j].rb, ma.a, (int32_t)ma.n, skip) != 4;
			}
		}
		if (busy) act.push_back(p);
	}
	const size_t n_act = act.size();
	if (n_act == 0) return BMH_OK;
	// ---- every refusal, before anything is enqueued
	const bmh_params_t &P = ctx->params;
	size_t bytes = 0, arena_n = 0, hits_n = 0;
	int lmax = 1, lmin = 65535;
	for (size_t q = 0; q < n_act; ++q)
		for (int i = 0; i < 2; ++i) {
			const int k = 2 * act[q] + i, l = reads[k].l_seq;
			if (l < 1 || l > 65535) {
				ctx->last_error = "bmh_matesw_device: read " + std::to_string(k) + " of a pair that needs rescue has " + std::to_string(l) + " bases (1..65535)";
				return BMH_E_RANGE;
			}
			if (!reads[k].seq) return BMH_E_ARG;
			// what validate_sw (api.hip) checks per task: it depends on the mate's length and the parameters only
			const bool xbyte = l * P.a < 250;
			if (!(ctx->wide_sw && !xbyte) && (int64_t)l * ctx->dev.max_mat >= kScoreLimit) {
				ctx->last_error = "bmh_matesw_device: read " + std::to_string(k) + ": l_seq*max(mat) reaches the 16-bit score range (bmh_ctx_set_wide_sw)";
				return BMH_E_RANGE;
			}
			if (xbyte && sw_byte_gaps_wrap(P)) {
				ctx->last_error = "bmh_matesw_device: byte mode needs o_del+e_del and o_ins+e_ins below 256";
				return BMH_E_RANGE;
			}
			if (regs[k].n > 0x7fffffffu) return BMH_E_ARG;
			bytes += (size_t)l, lmax = std::max(lmax, l), lmin = std::min(lmin, l);
			arena_n += regs[k].n + 4 * (size_t)n_hits(regs[k ^ 1]), hits_n += (size_t)n_hits(regs[k]);
		}
	if (arena_n > 0x7fffffffu || hits_n > 0x7fffffffu || n_act * kMswTasksPerPair > 0x7fffffffu) {
		ctx->last_error = "bmh_matesw_device: more than 2^31-1 regions in the batch";
		return BMH_E_ARG;
	}
	long long span = 0; // the widest window less the mate: high - low of an open orientation
	for (int r = 0; r < 4; ++r)
		if (!pes[r].failed) span = std::max(span, (long long)pes[r].high - pes[r].low);
	const int tcap = (int)std::min<long long>(std::min<long long>(span + lmax, l_pac << 1), 0x7fffffff);

	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	const MswLayout L(n_act, arena_n, hits_n, bytes + 16);
	const size_t b_up = L.state - L.out, b_down = L.pair - L.out;
	int rc;
	if ((rc = ensure(ctx, ctx->d_msw, L.total)) || (rc = ensure_host(ctx, ctx->h_up, b_up)) || (rc = ensure_host(ctx, ctx->h_down, b_down + 256))) return rc;
	uint8_t *d = (uint8_t *)ctx->d_msw.p, *hb = (uint8_t *)ctx->h_up.p;
	const auto up = [&](size_t x) { return hb + (x - L.out); }; // the staging buffer mirrors the device layout from `out` on
	memset(hb, 0, b_up);
	{
		int32_t *cnt = (int32_t *)up(L.out);
		bmh_alnreg_t *arena = (bmh_alnreg_t *)up(L.arena), *hits = (bmh_alnreg_t *)up(L.hits);
		MswPair *pair = (MswPair *)up(L.pair);
		uint8_t *pool = up(L.pool);
		size_t at = 0, a_at = 0, h_at = 0;
		for (size_t q = 0; q < n_act; ++q)
			for (int i = 0; i < 2; ++i) {
				const int k = 2 * act[q] + i;
				const bmh_alnreg_v &v = regs[k];
				MswPair &pr = pair[q];
				pr.read_off[i] = at, pr.l_seq[i] = reads[k].l_seq;
				memcpy(pool + at, reads[k].seq, (size_t)reads[k].l_seq), at += (size_t)reads[k].l_seq;
				pr.slice[i] = (uint32_t)a_at, pr.cap[i] = (int32_t)(v.n + 4 * (size_t)n_hits(regs[k ^ 1]));
				if (v.n) memcpy(arena + a_at, v.a, v.n * sizeof(bmh_alnreg_t));
				cnt[2 * q + i] = (int32_t)v.n, a_at += (size_t)pr.cap[i];
				pr.hit[i] = (uint32_t)h_at;
				for (size_t j = 0; j < v.n && pr.nb[i] < maxm; ++j)
					if (v.a[j].score >= v.a[0].score - o->pen_unpaired) hits[h_at + (size_t)pr.nb[i]++] = v.a[j];
				h_at += (size_t)pr.nb[i];
			}
	}
	const MswWs ws{(uint32_t *)(d + L.status), (int32_t *)(d + L.out), (int32_t *)(d + L.out) + 2 * n_act, (bmh_alnreg_t *)(d + L.arena),
	               (const MswPair *)(d + L.pair), (const bmh_alnreg_t *)(d + L.hits), (bmh_msw_pair_t *)(d + L.state), (bmh_sw_task_t *)(d + L.tasks),
	               (bmh_sw_result_t *)(d + L.res)};
	MswPes dpes;
	memcpy(dpes.r, pes, sizeof(dpes.r));
	const uint32_t task_cap = (uint32_t)(n_act * kMswTasksPerPair);
	const int max_rounds = 4 * maxm + 4;
	uint32_t *hs = (uint32_t *)ctx->h_down.p;
	hipStream_t s = ctx->stream;
	rc = [&]() -> int {
		BMH_HIP(ctx, hipMemsetAsync(ws.status, 0, MSW_STATUS_BYTES, s)); // the status words start clean on every call
		BMH_HIP(ctx, hipMemsetAsync(ws.state, 0, n_act * sizeof(bmh_msw_pair_t), s));
		BMH_HIP(ctx, hipMemcpyAsync(d + L.out, hb, b_up, hipMemcpyHostToDevice, s));
		uint32_t n_res = 0;
		for (int round = 0;; ++round) {
			if (round) BMH_HIP(ctx, hipMemsetAsync(ws.status, 0, 8, s)); // the round's tasks and unfinished pairs
			hipLaunchKernelGGL(msw_round_kernel, dim3((unsigned)((n_act + 63) / 64)), dim3(64), 0, s, P.a, o->min_seed_len, l_pac, dpes, ws, (int)n_act,
			                   n_res, task_cap, (uint32_t)arena_n, (uint32_t)hits_n, mask_level_redun, ctx->d_err);
			BMH_HIP(ctx, hipGetLastError());
			BMH_HIP(ctx, hipMemcpyAsync(hs, ws.status, 16, hipMemcpyDeviceToHost, s));
			BMH_HIP(ctx, stream_wait(ctx, s));
			if ((int)hs[MSW_ERR]) {
				ctx->last_error = (int)hs[MSW_ERR] == BMH_E_RANGE ? "mate rescue on the device: a Smith-Waterman task was outside the supported range (see bwamem_hip.h)"
				                                                  : "mate rescue on the device: a pair's regions do not fit its arena slice, or its records are inconsistent";
				return (int)hs[MSW_ERR];
			}
			n_res = hs[MSW_N_TASKS];
			if (hs[MSW_N_UNFINISHED] == 0) break;
			if (n_res > task_cap) return BMH_E_ARG;
			if (round >= max_rounds) { // cannot happen: the first planned invocation of a pair always folds
				ctx->last_error = "mate rescue on the device: no end after " + std::to_string(max_rounds) + " rounds";
				return BMH_E_ARG;
			}
			if (n_res) { // (a round without tasks is legal: empty or uncallable windows only)
				++st.rounds, st.ext_tasks += (int64_t)n_res;
				// the caps are given: the longest and shortest active read, the widest window any open orientation can ask for
				int e;
				if ((e = launch_sw(ctx, d + L.pool, ws.tasks, (int64_t)n_res, ws.res, lmax, std::max(tcap, 1), lmin))) return e;
			}
		}
		BMH_HIP(ctx, hipMemcpyAsync(ctx->h_down.p, d + L.out, b_down, hipMemcpyDeviceToHost, s));
		BMH_HIP(ctx, stream_wait(ctx, s));
		return BMH_OK;
	}();
	if (st.rounds) st.pool_bytes = (int64_t)bytes + 16; // as the host driver counts its pool: shipped for the first round that runs Smith-Waterman
	ctx->dstats = st;
	if (rc) return msw_abandon(ctx, rc);
	// ---- the vectors of the active pairs: grown first, so that a failure leaves every vector as it was
	const uint8_t *hd = (const uint8_t *)ctx->h_down.p;
	const int32_t *cnt = (const int32_t *)hd, *nsw = cnt + 2 * n_act;
	const bmh_alnreg_t *arena = (const bmh_alnreg_t *)(hd + (L.arena - L.out));
	const MswPair *pair = (const MswPair *)up(L.pair);
	for (size_t q = 0; q < n_act; ++q)
		for (int i = 0; i < 2; ++i) {
			bmh_alnreg_v &v = regs[2 * act[q] + i];
			const int32_t k = cnt[2 * q + i];
			if (k < 0 || k > pair[q].cap[i]) { // cannot happen
				ctx->last_error = "mate rescue on the device: the device's counts are inconsistent";
				return BMH_E_ARG;
			}
			if ((size_t)k > v.m) {
				bmh_alnreg_t *na = (bmh_alnreg_t *)realloc(v.a, (size_t)k * sizeof(bmh_alnreg_t));
				if (!na) {
					ctx->last_error = "mate rescue on the device: out of host memory for the regions";
					return BMH_E_NOMEM;
				}
				v.a = na, v.m = (size_t)k;
			}
		}
	for (size_t q = 0; q < n_act; ++q) {
		for (int i = 0; i < 2; ++i) {
			bmh_alnreg_v &v = regs[2 * act[q] + i];
			const size_t k = (size_t)cnt[2 * q + i];
			if (k) memcpy(v.a, arena + pair[q].slice[i], k * sizeof(bmh_alnreg_t));
			v.n = k;
		}
		if (n_sw) n_sw[act[q]] = nsw[q];
	}
	return BMH_OK;
}
