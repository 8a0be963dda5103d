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
// The same rescue over a flat region table that stays on the device (matesw_resident, bmh_matesw_table_device) is further down: the
// host's steps above as kernels around the same rounds.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bmh_ctx.h"
#include "bmh_device.h"
#include "wave_ticket.h"
#include "../host/matesw_core.h"
#include "../host/matesw_table_core.h"

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

// ---- the same rescue over a flat region table (matesw_resident): what the host driver does around the rounds, as kernels
//   mt_filter_kernel   one lane per pair: the candidate counts, the busy test, the capacities and the refusals of host/matesw_table_core.h
//                      into the pair's MtPair; the batch's plan -- active pairs, arena records, hits, longest and shortest active read,
//                      first refusal -- folded per wave, one ticket per wave, the last wave folds the parts into the MtPlan record
//   mt_sum_kernel / mt_scan_kernel   block sums of 256 positions and their exclusive scan, the form of region_long.hip
//   mt_pack_kernel     one lane per pair: its active index q (pair order, as the host's list), slice and hit starts from the scan; the
//                      MswPair record, the two counts, act[q]
//   mt_slices_kernel   one wave per active vector: its regions into the arena slice and its candidate hits into the hits, a lane per
//                      16 bytes: a wave instruction moves 1 KiB of consecutive bytes
//   (the rounds)
//   mt_count_kernel    per vector its final n (an active one's count, else its input length) into block sums
//   mt_place_kernel    roff_out from the scan, n_sw per pair, the 16-byte total record
//   mt_copy_kernel     one wave per vector: from the arena slice or from the input table into reg_out, a lane per 16 bytes
constexpr int kMtScanThreads = 256;
constexpr unsigned long long kMtNoRefusal = ~0ull;
enum { MT_R_ARG = 4 }; // beside BMH_MT_R_*: the table itself is inconsistent (offsets, a vector or a slice past 2^31 - 1 records)

struct MtSum {
	unsigned long long a, b, c;
};
__device__ __forceinline__ MtSum operator+(MtSum x, MtSum y) { return MtSum{x.a + y.a, x.b + y.b, x.c + y.c}; }

struct MtPair { // 32 bytes
	int32_t nb[2], cap[2];
	int32_t q;            // -1: needs no rescue; else its index among the active pairs (0 until mt_pack_kernel)
	uint32_t slice, hit;  // of end 0; end 1's follow at slice + cap[0], hit + nb[0]
	int32_t rsv;
};
static_assert(sizeof(MtPair) == 32, "pair record of the table form");

struct MtPlan { // 64 bytes: what comes down before the first round; a wave's part has the same form
	long long arena_n, hits_n;
	unsigned long long refusal; // read index << 8 | code of the smallest read index that raised one, kMtNoRefusal: none
	long long refusal_len;      // that read's length
	long long n_act;
	int32_t lmax, lmin;
	uint32_t ticket, rsv[3];
};
static_assert(sizeof(MtPlan) == 64, "plan record");
constexpr int kMtPartWords = sizeof(MtPlan) / 8; // a wave's part: the stride of MtStage's parts, six words of it used

struct MtTotal { // 16 bytes: what comes down behind the merge
	unsigned long long total;
	int32_t err, rsv;
};

struct MtIn {
	int n_pairs;
	const unsigned long long *soff, *roff;
	const bmh_alnreg_t *reg;
	unsigned long long total;
};

__device__ __forceinline__ void mt_merge(MtPlan &x, const MtPlan &y)
{
	x.arena_n += y.arena_n, x.hits_n += y.hits_n, x.n_act += y.n_act;
	x.lmax = max(x.lmax, y.lmax), x.lmin = min(x.lmin, y.lmin);
	if (y.refusal < x.refusal) x.refusal = y.refusal, x.refusal_len = y.refusal_len;
}

__device__ __forceinline__ void mt_wave_fold(MtPlan &x)
{
	for (int d = 32; d >= 1; d >>= 1) {
		MtPlan y;
		y.arena_n = __shfl_xor(x.arena_n, d), y.hits_n = __shfl_xor(x.hits_n, d), y.n_act = __shfl_xor(x.n_act, d);
		y.refusal = (unsigned long long)__shfl_xor((long long)x.refusal, d), y.refusal_len = __shfl_xor(x.refusal_len, d);
		y.lmax = __shfl_xor(x.lmax, d), y.lmin = __shfl_xor(x.lmin, d);
		mt_merge(x, y);
	}
}

__global__ __launch_bounds__(64) void mt_filter_kernel(MtIn in, bmh_matesw_opt_t o, MswPes pes, bmh_mt_rule_t rule, int64_t l_pac, MtPair *__restrict__ pair,
                                                       long long *part, MtPlan *plan)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x;
	MtPlan x = {0, 0, kMtNoRefusal, 0, 0, 1, 65535, 0, {0, 0, 0}};
	if (p < in.n_pairs) {
		MtPair rec = {{0, 0}, {0, 0}, -1, 0, 0, 0};
		const unsigned long long r0 = in.roff[2 * p], r1 = in.roff[2 * p + 1], r2 = in.roff[2 * p + 2];
		if (r0 > r1 || r1 > r2 || r2 > in.total || r1 - r0 > 0x7fffffffull || r2 - r1 > 0x7fffffffull) {
			x.refusal = (unsigned long long)(2 * (long long)p) << 8 | MT_R_ARG; // (nothing of the pair is read)
		} else {
			const long long l0 = (long long)(in.soff[2 * p + 1] - in.soff[2 * p]), l1 = (long long)(in.soff[2 * p + 2] - in.soff[2 * p + 1]);
			bmh_mt_pair_t m;
			bmh_mt_pair(l_pac, pes.r, &o, &rule, in.reg + r0, (int64_t)(r1 - r0), in.reg + r1, (int64_t)(r2 - r1), l0, l1, &m);
			rec.nb[0] = m.nb[0], rec.nb[1] = m.nb[1];
			if (m.busy) {
				int why[2] = {m.refuse[0], m.refuse[1]};
				for (int i = 0; i < 2; ++i)
					if (!why[i] && m.cap[i] > 0x7fffffffll) why[i] = MT_R_ARG;
				const int bad = why[0] ? 0 : why[1] ? 1 : -1;
				if (bad >= 0) {
					x.refusal = (unsigned long long)(2 * (long long)p + bad) << 8 | (unsigned)why[bad], x.refusal_len = bad ? l1 : l0;
				} else {
					rec.cap[0] = (int32_t)m.cap[0], rec.cap[1] = (int32_t)m.cap[1], rec.q = 0;
					x.n_act = 1, x.arena_n = m.cap[0] + m.cap[1], x.hits_n = (long long)m.nb[0] + m.nb[1];
					x.lmax = (int32_t)max(l0, l1), x.lmin = (int32_t)min(l0, l1);
				}
			}
		}
		pair[p] = rec;
	}
	mt_wave_fold(x);
	// the wave's part, a ticket, and on the last wave to arrive every wave's part (wave_ticket.h)
	const long long w[6] = {x.arena_n, x.hits_n, (long long)x.refusal, x.refusal_len, x.n_act, (long long)(uint32_t)x.lmax | (long long)x.lmin << 32};
	if (!wave_ticket_publish<6, kMtPartWords>(part, w, &plan->ticket)) return;
	MtPlan t = {0, 0, kMtNoRefusal, 0, 0, 1, 65535, 0, {0, 0, 0}};
	for (unsigned b = (unsigned)lane; b < gridDim.x; b += 64) {
		MtPlan y;
		y.arena_n = wave_ticket_word<kMtPartWords>(part, b, 0), y.hits_n = wave_ticket_word<kMtPartWords>(part, b, 1);
		y.refusal = (unsigned long long)wave_ticket_word<kMtPartWords>(part, b, 2);
		y.refusal_len = wave_ticket_word<kMtPartWords>(part, b, 3), y.n_act = wave_ticket_word<kMtPartWords>(part, b, 4);
		const long long ll = wave_ticket_word<kMtPartWords>(part, b, 5);
		y.lmax = (int32_t)(ll & 0xffffffffll), y.lmin = (int32_t)(ll >> 32);
		mt_merge(t, y);
	}
	mt_wave_fold(t);
	if (lane == 0) {
		plan->arena_n = t.arena_n, plan->hits_n = t.hits_n, plan->refusal = t.refusal, plan->refusal_len = t.refusal_len;
		plan->n_act = t.n_act, plan->lmax = t.lmax, plan->lmin = t.lmin;
	}
}

// exclusive prefix of v over the block's 256 threads, and the block's total; every thread of the block calls it
__device__ __forceinline__ MtSum mt_block_excl_scan(MtSum v, MtSum *total)
{
	__shared__ MtSum wsum[kMtScanThreads / 64];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	MtSum inc = v;
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long a = __shfl_up(inc.a, d), b = __shfl_up(inc.b, d), c = __shfl_up(inc.c, d);
		if (lane >= d) inc.a += a, inc.b += b, inc.c += c;
	}
	__syncthreads(); // (a second call in the same kernel: the first one's readers are done)
	if (lane == 63) wsum[wv] = inc;
	__syncthreads();
	MtSum base{0, 0, 0}, tot{0, 0, 0};
	for (int k = 0; k < kMtScanThreads / 64; ++k) {
		if (k < wv) base = base + wsum[k];
		tot = tot + wsum[k];
	}
	*total = tot;
	return MtSum{base.a + inc.a - v.a, base.b + inc.b - v.b, base.c + inc.c - v.c};
}

// what a position adds.  PAIRS: over the pairs, {1, its slices' records, its hits} for an active one.  VECS: over the vectors, a = its
// final n -- an active vector's count as the rounds left it, else its length in the input table
struct MtMerge {
	const MtPair *pair;
	const MswPair *mpair;
	const int32_t *cnt, *nsw;
	long long n_act;
	uint32_t *status;
};
enum { kMtPairs = 0, kMtVecs = 1 };
template <int WHAT>
__device__ __forceinline__ MtSum mt_value(const MtIn &in, const MtMerge &mg, long long k)
{
	if (WHAT == kMtPairs) {
		if (k >= in.n_pairs || mg.pair[k].q < 0) return MtSum{0, 0, 0};
		const MtPair r = mg.pair[k];
		return MtSum{1, (unsigned long long)r.cap[0] + (unsigned long long)r.cap[1], (unsigned long long)r.nb[0] + (unsigned long long)r.nb[1]};
	}
	if (k >= 2 * (long long)in.n_pairs) return MtSum{0, 0, 0};
	const MtPair r = mg.pair[k >> 1];
	if (r.q < 0) return MtSum{in.roff[k + 1] - in.roff[k], 0, 0}; // (mt_filter_kernel has seen the offsets in order)
	if (r.q >= mg.n_act) return MtSum{0, 0, 0};                    // (cannot happen: mt_pack_kernel has said so)
	const int32_t n = mg.cnt[2 * (size_t)r.q + (k & 1)];
	if (n < 0 || n > r.cap[k & 1]) { // cannot happen: the round kernel keeps a count inside its slice
		msw_fail(mg.status, BMH_E_ARG);
		return MtSum{0, 0, 0};
	}
	return MtSum{(unsigned long long)n, 0, 0};
}

template <int WHAT>
__global__ __launch_bounds__(kMtScanThreads) void mt_sum_kernel(MtIn in, MtMerge mg, MtSum *__restrict__ bsum)
{
	MtSum tot;
	(void)mt_block_excl_scan(mt_value<WHAT>(in, mg, (long long)blockIdx.x * kMtScanThreads + threadIdx.x), &tot);
	if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one block: bsum[0, nb) becomes its exclusive prefix, bsum[nb] the total
__global__ __launch_bounds__(kMtScanThreads) void mt_scan_kernel(MtSum *__restrict__ bsum, long long nb)
{
	MtSum carry{0, 0, 0};
	for (long long base = 0; base < nb; base += kMtScanThreads) { // (uniform bounds: every thread takes every round)
		const long long k = base + threadIdx.x;
		const MtSum v = k < nb ? bsum[k] : MtSum{0, 0, 0};
		MtSum tot;
		const MtSum ex = mt_block_excl_scan(v, &tot);
		if (k < nb) bsum[k] = carry + ex;
		carry = carry + tot;
	}
	if (threadIdx.x == 0) bsum[nb] = carry;
}

// pair and act start as 0xff bytes: a record this kernel does not reach has cap < 0, which the round kernel refuses and mt_slices_kernel
// passes over
__global__ __launch_bounds__(kMtScanThreads) void mt_pack_kernel(MtIn in, MtPair *__restrict__ pair, const MtSum *__restrict__ bsum, MswPair *__restrict__ mpair,
                                                                 int32_t *__restrict__ cnt, int32_t *__restrict__ nsw, int32_t *__restrict__ act, long long n_act,
                                                                 unsigned long long arena_n, unsigned long long hits_n, uint32_t *status)
{
	const long long p = (long long)blockIdx.x * kMtScanThreads + threadIdx.x;
	MtMerge mg = {pair, nullptr, nullptr, nullptr, n_act, status};
	MtSum tot;
	const MtSum v = mt_value<kMtPairs>(in, mg, p);
	const MtSum at = bsum[blockIdx.x] + mt_block_excl_scan(v, &tot);
	if (!v.a) return;
	MtPair r = pair[p];
	if (at.a >= (unsigned long long)n_act || at.b + v.b > arena_n || at.c + v.c > hits_n) { // the plan summed the same records: cannot happen
		msw_fail(status, BMH_E_ARG);
		r.q = -1, pair[p] = r;
		return;
	}
	r.q = (int32_t)at.a, r.slice = (uint32_t)at.b, r.hit = (uint32_t)at.c;
	pair[p] = r;
	MswPair pr;
	for (int i = 0; i < 2; ++i) {
		pr.read_off[i] = in.soff[2 * p + i], pr.l_seq[i] = (int32_t)(in.soff[2 * p + i + 1] - in.soff[2 * p + i]);
		pr.slice[i] = r.slice + (i ? (uint32_t)r.cap[0] : 0u), pr.cap[i] = r.cap[i];
		pr.hit[i] = r.hit + (i ? (uint32_t)r.nb[0] : 0u), pr.nb[i] = r.nb[i];
		pr.rsv[i] = 0;
		cnt[2 * at.a + i] = (int32_t)(in.roff[2 * p + i + 1] - in.roff[2 * p + i]);
	}
	mpair[at.a] = pr;
	nsw[at.a] = 0, act[at.a] = (int32_t)p;
}

static_assert(sizeof(bmh_alnreg_t) == 64, "the table kernels move a region as four uint4");
__global__ __launch_bounds__(kMtScanThreads) void mt_slices_kernel(MtIn in, const MswPair *__restrict__ mpair, const int32_t *__restrict__ act, long long n_act,
                                                                   int pen_unpaired, bmh_alnreg_t *__restrict__ arena, bmh_alnreg_t *__restrict__ hits,
                                                                   unsigned long long arena_n, unsigned long long hits_n)
{
	const long long v = (long long)blockIdx.x * (kMtScanThreads / 64) + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63, i = (int)(v & 1);
	if (v >= 2 * n_act) return;
	const MswPair pr = mpair[v >> 1];
	const long long p = act[v >> 1];
	if (pr.cap[i] < 0 || pr.nb[i] < 0 || p < 0 || p >= in.n_pairs) return;
	const unsigned long long r0 = in.roff[2 * p + i], n = in.roff[2 * p + i + 1] - r0;
	// every access below stays inside the table, the slice and the hits, or nothing is touched
	if (r0 > in.total || n > in.total - r0 || n > (unsigned long long)pr.cap[i] || (unsigned long long)pr.slice[i] + (unsigned long long)pr.cap[i] > arena_n ||
	    (unsigned long long)pr.hit[i] + (unsigned long long)pr.nb[i] > hits_n)
		return;
	if (n == 0) return;
	const bmh_alnreg_t *src = in.reg + r0;
	const uint4 *src4 = (const uint4 *)src;
	uint4 *dst4 = (uint4 *)(arena + pr.slice[i]), *hit4 = (uint4 *)(hits + pr.hit[i]);
	const int thr = src[0].score - pen_unpaired;
	long long seen = 0; // candidates before this chunk
	for (unsigned long long base = 0; base < n; base += 64) { // 64 records a chunk: one ballot, four 1-KiB moves
		const unsigned long long j = base + (unsigned)lane;
		const unsigned long long mask = __ballot(j < n && src[j].score >= thr);
		for (int s = 0; s < 4; ++s) {
			const unsigned x = (unsigned)(s * 64 + lane), rec = x >> 2; // the chunk's uint4 x belongs to its record rec
			if (base + rec >= n) continue;
			const uint4 d = src4[base * 4 + x];
			dst4[base * 4 + x] = d;
			if (mask >> rec & 1) {
				const long long rank = seen + __popcll(mask & ((1ull << rec) - 1));
				if (rank < pr.nb[i]) hit4[rank * 4 + (x & 3)] = d;
			}
		}
		seen += __popcll(mask);
	}
}

__global__ __launch_bounds__(kMtScanThreads) void mt_place_kernel(MtIn in, MtMerge mg, const MtSum *__restrict__ bsum, long long nb, unsigned long long *__restrict__ roff_out,
                                                                  int32_t *__restrict__ nsw_out, MtTotal *__restrict__ tot_out)
{
	const long long k = (long long)blockIdx.x * kMtScanThreads + threadIdx.x, nv = 2 * (long long)in.n_pairs;
	MtSum tot;
	const MtSum ex = mt_block_excl_scan(mt_value<kMtVecs>(in, mg, k), &tot);
	if (k == 0) {
		roff_out[nv] = bsum[nb].a;
		tot_out->total = bsum[nb].a, tot_out->err = (int32_t)mg.status[MSW_ERR], tot_out->rsv = 0;
	}
	if (k >= nv) return;
	roff_out[k] = bsum[blockIdx.x].a + ex.a;
	if (!(k & 1)) {
		const int32_t q = mg.pair[k >> 1].q;
		nsw_out[k >> 1] = q >= 0 && q < mg.n_act ? mg.nsw[q] : 0;
	}
}

__global__ __launch_bounds__(kMtScanThreads) void mt_copy_kernel(MtIn in, MtMerge mg, const bmh_alnreg_t *__restrict__ arena, unsigned long long arena_n,
                                                                 const unsigned long long *__restrict__ roff_out, bmh_alnreg_t *__restrict__ reg_out,
                                                                 unsigned long long out_cap)
{
	const long long k = (long long)blockIdx.x * (kMtScanThreads / 64) + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63, i = (int)(k & 1);
	if (k >= 2 * (long long)in.n_pairs) return;
	const unsigned long long o0 = roff_out[k], n = roff_out[k + 1] - o0;
	if (o0 > out_cap || n > out_cap - o0 || n == 0) return; // (the total record tells the host if the table outgrew its room)
	const MtPair r = mg.pair[k >> 1];
	const bmh_alnreg_t *src;
	if (r.q < 0) {
		const unsigned long long r0 = in.roff[k];
		if (r0 > in.total || n > in.total - r0) return;
		src = in.reg + r0;
	} else {
		if (r.q >= mg.n_act) return;
		const MswPair pr = mg.mpair[r.q];
		if (pr.cap[i] < 0 || n > (unsigned long long)pr.cap[i] || (unsigned long long)pr.slice[i] + (unsigned long long)pr.cap[i] > arena_n) return;
		src = arena + pr.slice[i];
	}
	const uint4 *src4 = (const uint4 *)src;
	uint4 *dst4 = (uint4 *)(reg_out + o0);
	for (unsigned long long x = (unsigned)lane; x < n * 4; x += 64) dst4[x] = src4[x];
}

// (bmh_ctx.h) waits for what was enqueued, then reads the kernels' error flag and clears it if set; the error stays the answer
int abandon_call(bmh_ctx *ctx, int rc)
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

} // namespace bmh

using namespace bmh;

namespace {

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

bmh_mt_rule_t mt_rule(const bmh_ctx *ctx)
{
	return bmh_mt_rule_t{ctx->params.a, ctx->dev.max_mat, kScoreLimit, ctx->wide_sw ? 1 : 0, sw_byte_gaps_wrap(ctx->params) ? 1 : 0, 0};
}

// the text of a read's refusal (host/matesw_table_core.h's codes); the table call names the read in all three
std::string mt_refusal_text(const char *who, int why, long long k, long long l, bool name_read = false)
{
	const std::string w = std::string(who) + ": ";
	if (why == BMH_MT_R_LEN) return w + "read " + std::to_string(k) + " of a pair that needs rescue has " + std::to_string(l) + " bases (1..65535)";
	if (why == BMH_MT_R_SCORE) return w + "read " + std::to_string(k) + ": l_seq*max(mat) reaches the 16-bit score range (bmh_ctx_set_wide_sw)";
	return w + (name_read ? "read " + std::to_string(k) + ": " : std::string()) + "byte mode needs o_del+e_del and o_ins+e_ins below 256";
}

// the target cap of the rounds' Smith-Waterman launches: the widest window any open orientation can ask for
int msw_tcap(const bmh_pestat_t pes[4], int64_t l_pac, int lmax)
{
	long long span = 0; // the widest window less the mate: high - low of an open orientation
	for (int r = 0; r < 4; ++r)
		if (!pes[r].failed) span = std::max(span, (long long)pes[r].high - pes[r].low);
	return (int)std::min<long long>(std::min<long long>(span + lmax, l_pac << 1), 0x7fffffff);
}

// The rounds of one call, for both drivers: the pair records, hits, slices and counts lie in ws and the status words are clean.  Per round
// the kernel, the 16-byte read-back (counted in *readbacks) and the round's ksw_align2 calls against d_pool; st gets the rounds and tasks.
int msw_run_rounds(bmh_ctx *ctx, int64_t l_pac, const bmh_matesw_opt_t *o, const bmh_pestat_t pes[4], const MswWs &ws, size_t n_act, size_t arena_n,
                   size_t hits_n, const uint8_t *d_pool, int lmax, int lmin, float mask_level_redun, bmh_driver_stats_t &st, int *readbacks)
{
	const bmh_params_t &P = ctx->params;
	MswPes dpes;
	memcpy(dpes.r, pes, sizeof(dpes.r));
	const int tcap = msw_tcap(pes, l_pac, lmax);
	const uint32_t task_cap = (uint32_t)(n_act * kMswTasksPerPair);
	const int max_rounds = 4 * std::max(o->max_matesw, 0) + 4;
	uint32_t *hs = (uint32_t *)ctx->h_down.p;
	hipStream_t s = ctx->stream;
	BMH_HIP(ctx, hipMemsetAsync(ws.state, 0, n_act * sizeof(bmh_msw_pair_t), s));
	uint32_t n_res = 0;
	for (int round = 0;; ++round) {
		if (round) BMH_HIP(ctx, hipMemsetAsync(ws.status, 0, 8, s)); // the round's tasks and unfinished pairs
		hipLaunchKernelGGL(msw_round_kernel, dim3((unsigned)((n_act + 63) / 64)), dim3(64), 0, s, P.a, o->min_seed_len, l_pac, dpes, ws, (int)n_act,
		                   n_res, task_cap, (uint32_t)arena_n, (uint32_t)hits_n, mask_level_redun, ctx->d_err);
		BMH_HIP(ctx, hipGetLastError());
		BMH_HIP(ctx, hipMemcpyAsync(hs, ws.status, 16, hipMemcpyDeviceToHost, s));
		BMH_HIP(ctx, stream_wait(ctx, s));
		++*readbacks;
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
			if ((e = launch_sw(ctx, d_pool, ws.tasks, (int64_t)n_res, ws.res, lmax, std::max(tcap, 1), lmin))) return e;
		}
	}
	return BMH_OK;
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
	// ---- the host driver's pre-filter: most pairs need no rescue at all (every mem_matesw call of theirs returns at bwamem_pair.c:122).
	// The rules are host/matesw_table_core.h's, which mt_filter_kernel runs over a table
	auto n_hits = [&](const bmh_alnreg_v &v) { return (size_t)bmh_mt_nb(v.a, (int64_t)v.n, o->pen_unpaired, o->max_matesw); }; // |b[i]| of :252-259
	const int maxm = std::max(o->max_matesw, 0);
	std::vector<int> act;
	for (int p = 0; p < n_pairs; ++p) {
		const bmh_alnreg_v &v0 = regs[2 * p], &v1 = regs[2 * p + 1];
		if (bmh_mt_busy(l_pac, pes, v0.a, (int64_t)v0.n, v1.a, (int64_t)v1.n, o->pen_unpaired, o->max_matesw)) act.push_back(p);
	}
	const size_t n_act = act.size();
	if (n_act == 0) return BMH_OK;
	// ---- every refusal, before anything is enqueued
	const bmh_mt_rule_t rule = mt_rule(ctx);
	size_t bytes = 0, arena_n = 0, hits_n = 0;
	int lmax = 1, lmin = 65535;
	for (size_t q = 0; q < n_act; ++q)
		for (int i = 0; i < 2; ++i) {
			const int k = 2 * act[q] + i, l = reads[k].l_seq;
			const int why = bmh_mt_refuse(&rule, (int64_t)l);
			if (why == BMH_MT_R_LEN || (why && reads[k].seq)) {
				ctx->last_error = mt_refusal_text("bmh_matesw_device", why, k, (long long)l);
				return BMH_E_RANGE;
			}
			if (!reads[k].seq) return BMH_E_ARG;
			if (regs[k].n > 0x7fffffffu) return BMH_E_ARG;
			bytes += (size_t)l, lmax = std::max(lmax, l), lmin = std::min(lmin, l);
			arena_n += (size_t)bmh_mt_cap((int64_t)regs[k].n, (int32_t)n_hits(regs[k ^ 1])), hits_n += n_hits(regs[k]);
		}
	if (arena_n > 0x7fffffffu || hits_n > 0x7fffffffu || n_act * kMswTasksPerPair > 0x7fffffffu) {
		ctx->last_error = "bmh_matesw_device: more than 2^31-1 regions in the batch";
		return BMH_E_ARG;
	}

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
	hipStream_t s = ctx->stream;
	rc = [&]() -> int {
		BMH_HIP(ctx, hipMemsetAsync(ws.status, 0, MSW_STATUS_BYTES, s)); // the status words start clean on every call
		BMH_HIP(ctx, hipMemcpyAsync(d + L.out, hb, b_up, hipMemcpyHostToDevice, s));
		int readbacks = 0, e;
		if ((e = msw_run_rounds(ctx, l_pac, o, pes, ws, n_act, arena_n, hits_n, d + L.pool, lmax, lmin, mask_level_redun, st, &readbacks))) return e;
		BMH_HIP(ctx, hipMemcpyAsync(ctx->h_down.p, d + L.out, b_down, hipMemcpyDeviceToHost, s));
		BMH_HIP(ctx, stream_wait(ctx, s));
		return BMH_OK;
	}();
	if (st.rounds) st.pool_bytes = (int64_t)bytes + 16; // as the host driver counts its pool: shipped for the first round that runs Smith-Waterman
	ctx->dstats = st;
	if (rc) return abandon_call(ctx, rc);
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

// ---- the table form

namespace {

struct MtStage { // ctx->d_mswt: what the filter needs, sized from n_pairs alone
	size_t plan, part, pair, bsum, total;
	size_t waves, blocks_p, blocks_v;
	explicit MtStage(size_t n_pairs)
	{
		waves = std::max<size_t>((n_pairs + 63) / 64, 1);
		blocks_p = std::max<size_t>((n_pairs + kMtScanThreads - 1) / kMtScanThreads, 1);
		blocks_v = std::max<size_t>((2 * n_pairs + kMtScanThreads - 1) / kMtScanThreads, 1);
		plan = 0, part = al256(sizeof(MtPlan)), pair = part + al256(waves * 64), bsum = pair + al256(n_pairs * sizeof(MtPair));
		total = bsum + al256((blocks_v + 1) * sizeof(MtSum)); // (the pairs' sums and later the vectors' take turns in it)
	}
};

struct MtEvents { // the three kernel groups' brackets in timing mode
	bmh_ctx *ctx;
	int begin(int g)
	{
		if (!ctx->timing) return BMH_OK;
		for (hipEvent_t &e : ctx->ev_mswt)
			if (!e) BMH_HIP(ctx, hipEventCreate(&e));
		BMH_HIP(ctx, hipEventRecord(ctx->ev_mswt[2 * g], ctx->stream));
		return BMH_OK;
	}
	int end(int g)
	{
		if (ctx->timing) BMH_HIP(ctx, hipEventRecord(ctx->ev_mswt[2 * g + 1], ctx->stream));
		return BMH_OK;
	}
	int ms(int g, float *out)
	{
		if (ctx->timing) BMH_HIP(ctx, hipEventElapsedTime(out, ctx->ev_mswt[2 * g], ctx->ev_mswt[2 * g + 1]));
		return BMH_OK;
	}
};

} // namespace

int bmh::matesw_resident(bmh_ctx *ctx, int64_t l_pac, int n_pairs, const uint8_t *d_pool, const unsigned long long *d_soff, const ResidentRegs &in,
                         const bmh_pestat_t pes[4], const bmh_matesw_opt_t *o, float mask_level_redun, ResidentRegs *out, int **d_n_sw,
                         const bmh_sam_opt_t *plan_opt, long long *n_sw_sum)
{
	static const char *who = "bmh_matesw_table_device";
	bmh_driver_stats_t st{};
	ctx->dstats = st;
	bmh_matesw_table_stats_t &mt = ctx->mt;
	mt = bmh_matesw_table_stats_t{in.total, 0, 0, 0, 0, n_pairs, 0, 0, -1.f, -1.f, -1.f};
	const size_t np = (size_t)n_pairs;
	const MtStage S(np);
	int rc;
	if ((rc = ensure(ctx, ctx->d_mswt, S.total)) || (rc = ensure_host(ctx, ctx->h_down, 256))) return rc;
	uint8_t *ds = (uint8_t *)ctx->d_mswt.p;
	MtPlan *d_plan = (MtPlan *)(ds + S.plan);
	MtPair *d_pair = (MtPair *)(ds + S.pair);
	MtSum *d_bsum = (MtSum *)(ds + S.bsum);
	const MtIn tin{n_pairs, d_soff, in.roff, in.reg, (unsigned long long)in.total};
	MswPes dpes;
	memcpy(dpes.r, pes, sizeof(dpes.r));
	hipStream_t s = ctx->stream;
	MtEvents ev{ctx};
	// ---- the filter, the sums of its records and their scan; the plan record comes down: the first wait
	MtMerge mg{d_pair, nullptr, nullptr, nullptr, 0, nullptr};
	BMH_HIP(ctx, hipMemsetAsync(d_plan, 0, sizeof(MtPlan), s));
	if ((rc = ev.begin(0))) return rc;
	hipLaunchKernelGGL(mt_filter_kernel, dim3((unsigned)S.waves), dim3(64), 0, s, tin, *o, dpes, mt_rule(ctx), l_pac, d_pair, (long long *)(ds + S.part), d_plan);
	hipLaunchKernelGGL(mt_sum_kernel<kMtPairs>, dim3((unsigned)S.blocks_p), dim3(kMtScanThreads), 0, s, tin, mg, d_bsum);
	hipLaunchKernelGGL(mt_scan_kernel, dim3(1), dim3(kMtScanThreads), 0, s, d_bsum, (long long)S.blocks_p);
	BMH_HIP(ctx, hipGetLastError());
	if ((rc = ev.end(0))) return rc;
	BMH_HIP(ctx, hipMemcpyAsync(ctx->h_down.p, d_plan, sizeof(MtPlan), hipMemcpyDeviceToHost, s));
	BMH_HIP(ctx, stream_wait(ctx, s));
	mt.mid_bytes += (int64_t)sizeof(MtPlan), ++mt.waits;
	const MtPlan plan = *(const MtPlan *)ctx->h_down.p;
	if ((rc = ev.ms(0, &mt.filter_ms))) return rc;
	if (plan.refusal != kMtNoRefusal) {
		const int why = (int)(plan.refusal & 0xff);
		const long long k = (long long)(plan.refusal >> 8);
		if (why == MT_R_ARG) {
			ctx->last_error = std::string(who) + ": read " + std::to_string(k) + ": its regions' offsets run backwards or past the table, or a vector or slice exceeds 2^31-1 regions";
			return BMH_E_ARG;
		}
		ctx->last_error = mt_refusal_text(who, why, k, plan.refusal_len, true);
		return BMH_E_RANGE;
	}
	if (plan.n_act < 0 || plan.n_act > n_pairs || plan.arena_n < 0 || plan.hits_n < 0) { // cannot happen
		ctx->last_error = std::string(who) + ": the plan record is inconsistent";
		return BMH_E_ARG;
	}
	const size_t n_act = (size_t)plan.n_act, arena_n = (size_t)plan.arena_n, hits_n = (size_t)plan.hits_n;
	if (arena_n > 0x7fffffffu || hits_n > 0x7fffffffu || n_act * kMswTasksPerPair > 0x7fffffffu) {
		ctx->last_error = std::string(who) + ": more than 2^31-1 regions in the batch";
		return BMH_E_ARG;
	}
	mt.active = (int32_t)n_act, mt.arena_records = (int64_t)arena_n, mt.hits = (int64_t)hits_n;
	// ---- the rounds' block as bmh_matesw_device lays it out, without a pool; behind it the active list, the output table and n_sw
	const MswLayout L(n_act, arena_n, hits_n, 0);
	const size_t out_cap = (size_t)in.total + 4 * hits_n; // an invocation inserts at most four regions
	size_t at = L.total;
	auto take = [&](size_t bytes) {
		const size_t x = at;
		at += al256(bytes);
		return x;
	};
	// (the plan record of a caller with plan_opt lies right behind the total: one copy brings both)
	const size_t b_tot = sizeof(MtTotal) + (plan_opt ? kTablePlanRecBytes : 0);
	const size_t o_act = take(n_act * 4), o_roff = take((2 * np + 1) * 8), o_nsw = take(np * 4), o_tot = take(b_tot), o_reg = take(out_cap * sizeof(bmh_alnreg_t));
	const size_t o_ppart = take(plan_opt ? table_plan_part_bytes(2 * n_pairs) : 0);
	if ((rc = ensure(ctx, ctx->d_msw, at))) return rc;
	uint8_t *d = (uint8_t *)ctx->d_msw.p;
	if ((const uint8_t *)in.reg >= d && (const uint8_t *)in.reg < d + ctx->d_msw.cap) return BMH_E_ARG; // the input must not lie in the output's buffer
	const MswWs ws{(uint32_t *)(d + L.status), (int32_t *)(d + L.out), (int32_t *)(d + L.out) + 2 * n_act, (bmh_alnreg_t *)(d + L.arena),
	               (const MswPair *)(d + L.pair), (const bmh_alnreg_t *)(d + L.hits), (bmh_msw_pair_t *)(d + L.state), (bmh_sw_task_t *)(d + L.tasks),
	               (bmh_sw_result_t *)(d + L.res)};
	int32_t *d_act = (int32_t *)(d + o_act), *d_nsw_out = (int32_t *)(d + o_nsw);
	unsigned long long *d_roff_out = (unsigned long long *)(d + o_roff);
	MtTotal *d_tot = (MtTotal *)(d + o_tot);
	bmh_alnreg_t *d_reg_out = (bmh_alnreg_t *)(d + o_reg);
	mg = MtMerge{d_pair, ws.pair, ws.cnt, ws.nsw, (long long)n_act, ws.status};
	int readbacks = 0;
	rc = [&]() -> int {
		int e;
		BMH_HIP(ctx, hipMemsetAsync(ws.status, 0, MSW_STATUS_BYTES, s)); // the status words start clean on every call
		if (n_act) {
			if ((e = ev.begin(1))) return e;
			BMH_HIP(ctx, hipMemsetAsync(d + L.pair, 0xff, n_act * sizeof(MswPair), s));
			BMH_HIP(ctx, hipMemsetAsync(d_act, 0xff, n_act * 4, s));
			hipLaunchKernelGGL(mt_pack_kernel, dim3((unsigned)S.blocks_p), dim3(kMtScanThreads), 0, s, tin, d_pair, (const MtSum *)d_bsum, (MswPair *)(d + L.pair),
			                   ws.cnt, ws.nsw, d_act, (long long)n_act, (unsigned long long)arena_n, (unsigned long long)hits_n, ws.status);
			hipLaunchKernelGGL(mt_slices_kernel, dim3((unsigned)((2 * n_act + 3) / 4)), dim3(kMtScanThreads), 0, s, tin, ws.pair, (const int32_t *)d_act,
			                   (long long)n_act, o->pen_unpaired, ws.arena, (bmh_alnreg_t *)(d + L.hits), (unsigned long long)arena_n, (unsigned long long)hits_n);
			BMH_HIP(ctx, hipGetLastError());
			if ((e = ev.end(1))) return e;
			if ((e = msw_run_rounds(ctx, l_pac, o, pes, ws, n_act, arena_n, hits_n, d_pool, plan.lmax, plan.lmin, mask_level_redun, st, &readbacks))) return e;
		}
		// ---- the merge: the final lengths, their scan, the offsets and n_sw, the regions; the total comes down: the last wait
		if ((e = ev.begin(2))) return e;
		hipLaunchKernelGGL(mt_sum_kernel<kMtVecs>, dim3((unsigned)S.blocks_v), dim3(kMtScanThreads), 0, s, tin, mg, d_bsum);
		hipLaunchKernelGGL(mt_scan_kernel, dim3(1), dim3(kMtScanThreads), 0, s, d_bsum, (long long)S.blocks_v);
		hipLaunchKernelGGL(mt_place_kernel, dim3((unsigned)S.blocks_v), dim3(kMtScanThreads), 0, s, tin, mg, (const MtSum *)d_bsum, (long long)S.blocks_v, d_roff_out,
		                   d_nsw_out, d_tot);
		hipLaunchKernelGGL(mt_copy_kernel, dim3((unsigned)std::max<size_t>((2 * np + 3) / 4, 1)), dim3(kMtScanThreads), 0, s, tin, mg, (const bmh_alnreg_t *)ws.arena,
		                   (unsigned long long)arena_n, (const unsigned long long *)d_roff_out, d_reg_out, (unsigned long long)out_cap);
		BMH_HIP(ctx, hipGetLastError());
		if ((e = ev.end(2))) return e;
		// what phase 2 must know of the table just made (table_plan_kernel, chain2reg.hip); an offset past the table's room is the total's error
		if (plan_opt) BMH_HIP(ctx, hipMemsetAsync(d_tot + 1, 0, kTablePlanRecBytes, s)); // its ticket starts at 0
		if (plan_opt && (e = launch_table_plan(ctx, *plan_opt, 2 * n_pairs, d_roff_out, d_reg_out, (unsigned long long)out_cap, d_nsw_out, d + o_ppart, d_tot + 1, &d_tot->err)))
			return e;
		BMH_HIP(ctx, hipMemcpyAsync(ctx->h_down.p, d_tot, b_tot, hipMemcpyDeviceToHost, s));
		BMH_HIP(ctx, stream_wait(ctx, s));
		return BMH_OK;
	}();
	mt.mid_bytes += 16 * (int64_t)readbacks, mt.waits += readbacks;
	ctx->dstats = st;
	if (rc) return abandon_call(ctx, rc);
	mt.mid_bytes += (int64_t)b_tot, ++mt.waits; // (with the plan record behind the total where the caller asked for one)
	const MtTotal tot = *(const MtTotal *)ctx->h_down.p;
	if (tot.err || tot.total > out_cap) { // cannot happen
		ctx->last_error = "mate rescue on the device: the device's counts are inconsistent";
		return abandon_call(ctx, BMH_E_ARG);
	}
	if (n_act && (rc = ev.ms(1, &mt.pack_ms))) return rc;
	if ((rc = ev.ms(2, &mt.merge_ms))) return rc;
	mt.regions_out = (int64_t)tot.total;
	*out = ResidentRegs{};
	if (plan_opt && (!table_plan_read((const uint8_t *)ctx->h_down.p + sizeof(MtTotal), 2 * n_pairs, out, n_sw_sum) || out->total != (long long)tot.total)) { // cannot happen
		ctx->last_error = "mate rescue on the device: the plan over its table is inconsistent";
		return BMH_E_ARG;
	}
	out->roff = d_roff_out, out->reg = d_reg_out, out->total = (long long)tot.total;
	*d_n_sw = d_nsw_out;
	return BMH_OK;
}

static_assert(sizeof(bmh_matesw_table_stats_t) == 64, "bmh_matesw_table_stats_t is part of the interface");

extern "C" int bmh_matesw_table_device(bmh_ctx_t *ctx, int64_t l_pac, int n_pairs, const bmh_read_t *reads, const uint64_t *roff, const bmh_alnreg_t *reg,
                                       const bmh_pestat_t pes[4], const bmh_matesw_opt_t *o, float mask_level_redun, uint64_t *roff_out,
                                       bmh_alnreg_t **reg_out, int *n_sw)
{
	if (!ctx || !roff || !pes || !o || !roff_out || !reg_out || n_pairs < 0 || l_pac <= 0 || (n_pairs > 0 && !reads)) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	if (!ctx->dev.pac || ctx->dev.l_pac != l_pac) {
		ctx->last_error = "bmh_matesw_table_device: needs the 2-bit reference of this l_pac resident on the device (bmh_ctx_set_pac)";
		return BMH_E_ARG;
	}
	const size_t nv = 2 * (size_t)n_pairs;
	if (roff[0] != 0) return BMH_E_ARG;
	size_t bytes = 0;
	for (size_t k = 0; k < nv; ++k) {
		if (roff[k + 1] < roff[k] || roff[k + 1] - roff[k] > 0x7fffffffu) {
			ctx->last_error = "bmh_matesw_table_device: roff must not decrease, and a vector holds at most 2^31-1 regions (read " + std::to_string(k) + ")";
			return BMH_E_ARG;
		}
		if (reads[k].l_seq < 0 || (reads[k].l_seq > 0 && !reads[k].seq)) return BMH_E_ARG;
		bytes += (size_t)reads[k].l_seq;
	}
	const size_t total = (size_t)roff[nv];
	if (total && !reg) return BMH_E_ARG;
	ctx->dstats = bmh_driver_stats_t{};

	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	// ---- one upload: [read offsets | region offsets | regions | reads, 16 bytes of padding behind them]
	const size_t u_soff = 0, u_roff = al256((nv + 1) * 8), u_reg = u_roff + al256((nv + 1) * 8), u_pool = u_reg + al256(total * sizeof(bmh_alnreg_t));
	const size_t b_up = u_pool + al256(bytes + 16);
	int rc;
	if ((rc = ensure(ctx, ctx->d_mswin, b_up)) || (rc = ensure_host(ctx, ctx->h_up, b_up))) return rc;
	uint8_t *hb = (uint8_t *)ctx->h_up.p, *du = (uint8_t *)ctx->d_mswin.p;
	{
		unsigned long long *soff = (unsigned long long *)(hb + u_soff);
		uint8_t *pool = hb + u_pool;
		size_t at = 0;
		for (size_t k = 0; k < nv; ++k) {
			soff[k] = at;
			if (reads[k].l_seq) memcpy(pool + at, reads[k].seq, (size_t)reads[k].l_seq);
			at += (size_t)reads[k].l_seq;
		}
		soff[nv] = at;
		memset(pool + at, 0, 16);
		memcpy(hb + u_roff, roff, (nv + 1) * 8);
		if (total) memcpy(hb + u_reg, reg, total * sizeof(bmh_alnreg_t));
	}
	BMH_HIP(ctx, hipMemcpyAsync(du, hb, b_up, hipMemcpyHostToDevice, ctx->stream));
	ResidentRegs in, out;
	in.roff = (const unsigned long long *)(du + u_roff), in.reg = (const bmh_alnreg_t *)(du + u_reg), in.total = (long long)total;
	int *d_nsw = nullptr;
	if ((rc = matesw_resident(ctx, l_pac, n_pairs, du + u_pool, (const unsigned long long *)(du + u_soff), in, pes, o, mask_level_redun, &out, &d_nsw))) return rc;
	if (ctx->dstats.rounds) ctx->dstats.pool_bytes = (int64_t)bytes + 16; // the pool as it went up: every read
	// ---- one download: the offsets, n_sw, the regions; the caller's memory is written once everything is there
	const size_t otot = (size_t)out.total, d_roff = 0, d_nsw_at = al256((nv + 1) * 8), d_reg = d_nsw_at + al256((size_t)n_pairs * 4);
	const size_t b_down = d_reg + otot * sizeof(bmh_alnreg_t);
	if ((rc = ensure_host(ctx, ctx->h_down, b_down + 256))) return rc;
	uint8_t *hd = (uint8_t *)ctx->h_down.p;
	BMH_HIP(ctx, hipMemcpyAsync(hd + d_roff, out.roff, (nv + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (n_pairs) BMH_HIP(ctx, hipMemcpyAsync(hd + d_nsw_at, d_nsw, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
	if (otot) BMH_HIP(ctx, hipMemcpyAsync(hd + d_reg, out.reg, otot * sizeof(bmh_alnreg_t), hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	bmh_alnreg_t *ro = (bmh_alnreg_t *)malloc(std::max<size_t>(otot, 1) * sizeof(bmh_alnreg_t));
	if (!ro) {
		ctx->last_error = "bmh_matesw_table_device: out of host memory for the regions";
		return BMH_E_NOMEM;
	}
	if (otot) memcpy(ro, hd + d_reg, otot * sizeof(bmh_alnreg_t));
	memcpy(roff_out, hd + d_roff, (nv + 1) * 8);
	if (n_sw && n_pairs) memcpy(n_sw, hd + d_nsw_at, (size_t)n_pairs * 4);
	*reg_out = ro;
	return BMH_OK;
}

extern "C" int bmh_last_matesw_table_stats(const bmh_ctx_t *ctx, bmh_matesw_table_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->mt;
	return BMH_OK;
}
