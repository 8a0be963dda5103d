// chain2reg.hip -- chains to regions on the device: the per-read driver of mem_chain2aln (reference bwa-0.7.8/bwamem.c:730-878) and
// mem_chain2aln_short (:495-542), i.e. everything chains2regs() of host/chain2aln_batch.c does, without the chains, tasks, results or
// regions ever visiting the host.  The arithmetic both drivers must agree on is one text, host/chain2aln_core.h.
//
// Input: the device chainer's compact output where chain_place_kernel leaves it (DevChains: per read coff / soff, per chain its seed
// count, the seeds) and the reads as a pool with per-read offsets and lengths.  One lane per read throughout, like chain_kernel.
//
//   c2r_window_kernel   per chain: the window [rmax0, rmax1) (bwamem.c:740-755), the short-chain qualifying test and the bmh_sw_task_t
//                       of its ksw_align2 (appended with an atomic counter: results are addressed through the index kept in the
//                       chain's record, so append order never reaches the output), the chain's (len, index) keys in ascending order,
//                       and the round-1 bmh_seed_task_t of the seed the reference extends first -- the task of flat chain c at
//                       index c, so round 1 has exactly tc tasks, which the host knows
//   launch_sw           the short chains' Smith-Watermans
//   loop                launch_seedext on the new tail of the task array, then c2r_replay_kernel: run_read()'s state machine
//                       {st, ci, k} kept in device memory between launches.  A read that needs a result that is not there stops and
//                       appends what the host driver requests (the seed it stopped at, the rest of its chain, the later chains, all
//                       but the provably skipped seeds) behind the earlier rounds' tasks: ONE task array and ONE result array of ts
//                       entries (every kept seed is requested at most once), so "the result is there" is index < tasks finished so far.
//                       A per-seed word (task index + 1, 0 = never requested) is the host driver's have[].
//                       The host reads back {tasks appended, reads stopped, error flag, short-chain tasks}: 16 bytes per round trip.
//   region_dedup_kernel with bmh_ctx_set_regs_dedup on: mem_sort_and_dedup (bwamem.c:395-436, the text of host/dedup_core.h) in place on
//                       every read's arena slice, so that the gather below moves the survivors only.  Also what bmh_sort_dedup_batch
//                       (api.hip) runs on a caller's vectors.
//   gather              count -> scan -> place of the regions (each read wrote into its slice of the region arena, the soff prefix
//                       sums: a read yields at most as many regions as it has kept seeds), then the counts and the compact records down.
//   table_plan_kernel   resident mode (bmh_reads_sam_device) instead of the download: the compact records and their offsets stay where
//                       c2r_place_kernel left them, and one lane per read folds its vector into what phase 2 must know before its first
//                       launch (host/handoff_core.h).  One 128-byte record -- the status words and the plan -- comes down: one wait.
//                       The same kernel runs over the table mate rescue leaves (matesw.hip).
// Behind c2r_place_kernel the driver has three tails, each chosen by its caller: vectors for the host, resident regions with the plan,
// resident regions with the total and the insert-size words.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "bmh_ctx.h"
#include "bmh_device.h"
#include "wave_ticket.h"
#include "../host/chain2aln_core.h"
#include "../host/dedup_core.h"
#include "../host/handoff_core.h"
#include "../host/pestat_core.h"

namespace bmh {

enum { C2R_NEXT_CHAIN = 0, C2R_NEXT_SEED = 1, C2R_DONE = 2 };
// status words (uint32 index).  0..3 are what the host reads in the loop
enum { C2R_N_TASKS = 0, C2R_N_STOPPED = 1, C2R_ERR = 2, C2R_N_SHORT = 3, C2R_EXT_TASKS = 4, C2R_EXTENDED = 6, C2R_SKIPPED = 8, C2R_CHAINS_IN = 10, C2R_DEDUP_REMOVED = 12, C2R_DROP_REMOVED = 14, C2R_STATUS_BYTES = 64 };

struct C2rPlan { // table_plan_kernel's record; the single-end hand-off keeps it right behind the status words: one copy brings both
	bmh_ho_plan_t plan;
	uint32_t ticket; // waves that have written their part
	uint32_t rsv0;
	int64_t pair_kmax; // bmh_ho_pairs over the table's mates
	int64_t n_sw;      // the sum of the per-pair counts the kernel was given, else 0
	uint32_t rsv[2];
};
static_assert(sizeof(C2rPlan) == 64 && sizeof(bmh_ho_plan_t) == 32 && sizeof(C2rPlan) == kTablePlanRecBytes, "plan record");
constexpr int kPlanPartWords = 8; // a wave's part: kmax, opool_cap, total, neg | pair_kmax << 32, n_sw, three spare words

struct C2rChain { // one chain's record, 64 bytes
	int64_t rmax0, rmax1;
	uint64_t seed_base; // flat index of its seed 0 (into seeds, keys and task words)
	int64_t srb, sre;   // mem_chain2aln_short's reference interval ...
	int32_t n;
	int32_t sw_idx;     // ... and the index of its ksw_align2 in the short-chain tasks, -1 = it returns without one
	int32_t sqb, sqe, seedcov, rsv;
};
static_assert(sizeof(C2rChain) == 64, "chain record");

struct C2rState { // run_read()'s state between launches
	int st, ci, k, rsv;
};

struct C2rIn {
	int n_reads;
	const uint64_t *read_off; // q_off of read r in the pool the extension kernels are given
	const int *len;
	const unsigned long long *coff, *soff; // n_reads + 1 each
	const uint32_t *cn;
	const bmh_seed_t *seeds;
	unsigned long long tc, ts;
	const uint32_t *n_keys; // per read its chains before the filter, summed for bmh_chain_stats; null: chains from the host
};

struct C2rWs {
	uint32_t *status;
	C2rChain *chn;           // tc
	C2rState *state;         // n_reads
	uint64_t *srt;           // ts: per chain its keys, 0 where the replay skipped a seed
	uint32_t *slot;          // ts: task index + 1 of the seed's extension, 0 = not requested
	bmh_seed_task_t *tasks;  // ts
	bmh_seed_result_t *res;  // ts
	bmh_sw_task_t *swt;      // tc
	bmh_sw_result_t *swr;    // tc
	bmh_alnreg_t *reg;       // ts: the region arena, read r's slice at soff[r]
	unsigned long long *nreg, *roff; // n_reads + 1: regions per read, their exclusive sums
	uint32_t *cand;          // n_reads / 2 + 1: mem_pestat's word per pair (pestat_collect_kernel), right behind roff: one copy brings both
	bmh_alnreg_t *out;       // ts: the compact regions
	long long *part;         // (n_reads / 64 + 1) x kPlanPartWords: table_plan_kernel's per-wave parts
};

struct C2rSwRule { // what validate_sw (api.hip) checks per task of a host-fed batch
	int msl;       // opt->min_seed_len, 0 = no short-chain pre-step
	int max_mat;
	int wide_sw, wraps;
};

__device__ __forceinline__ void c2r_fail(uint32_t *status, int code) { atomicCAS((int *)&status[C2R_ERR], 0, code); }

// keys are unique, so any sort gives the reference's order: heapsort in place, no stack
__device__ __forceinline__ void c2r_sort(uint64_t *a, int n)
{
	for (int start = n / 2 - 1, end = n; end > 1;) {
		uint64_t v;
		int root;
		if (start >= 0) v = a[start], root = start--;
		else v = a[--end], a[end] = a[0], root = 0;
		for (;;) {
			int ch = 2 * root + 1;
			if (ch >= end) break;
			if (ch + 1 < end && a[ch + 1] > a[ch]) ++ch;
			if (a[ch] <= v) break;
			a[root] = a[ch], root = ch;
		}
		a[root] = v;
	}
}

// request() of the host driver without its bookkeeping: the fused record of seed s of chain c.  BMH_E_RANGE as there, BMH_E_ARG for a
// seed that does not lie inside its read (what validate_seeds answers the host driver)
__device__ __forceinline__ int c2r_task(const C2rChain &c, const bmh_seed_t &s, uint64_t q_off, int l_query, bmh_seed_task_t *t)
{
	if (l_query < 1 || s.qbeg < 0 || s.len < 1 || s.qbeg + s.len > l_query) return BMH_E_ARG; // (validate_seeds of the host-fed call)
	if (s.rbeg < c.rmax0 || s.rbeg + s.len > c.rmax1 || c.rmax1 - c.rmax0 > 0x7fffffff) return BMH_E_RANGE;
	t->q_off = q_off, t->t_off = (uint64_t)c.rmax0; // rseq[0], bwamem.c:757: the window is read from the resident reference
	t->l_query = l_query, t->qbeg = s.qbeg, t->len = s.len;
	t->rbeg = (int32_t)(s.rbeg - c.rmax0), t->wlen = (int32_t)(c.rmax1 - c.rmax0);
	t->flags = BMH_F_TPAC, t->rsv_ = 0;
	return 0;
}

__global__ __launch_bounds__(64) void c2r_window_kernel(bmh_params_t p, int64_t l_pac, C2rIn in, C2rWs ws, C2rSwRule sw)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r == 0) ws.status[C2R_N_TASKS] = (uint32_t)in.tc; // later rounds append behind round 1
	if (r >= in.n_reads) return;
	const C2rState st0 = {C2R_NEXT_CHAIN, -1, 0, 0};
	ws.state[r] = st0, ws.nreg[r] = 0;
	if (in.n_keys && in.n_keys[r]) atomicAdd((unsigned long long *)&ws.status[C2R_CHAINS_IN], (unsigned long long)in.n_keys[r]);
	const int l_query = in.len[r];
	const uint64_t q_off = in.read_off[r];
	const unsigned long long c0 = in.coff[r], c1 = in.coff[r + 1], s1 = in.soff[r + 1];
	unsigned long long sb = in.soff[r];
	if (c1 > in.tc || s1 > in.ts || c0 > c1 || sb > s1) { c2r_fail(ws.status, BMH_E_ARG); ws.state[r].st = C2R_DONE; return; }
	for (unsigned long long c = c0; c < c1; ++c) {
		const int n = (int)in.cn[c];
		C2rChain w = {0, 0, sb, 0, 0, n, -1, 0, 0, 0, 0};
		if (n < 1 || sb + (unsigned long long)n > s1) { // (the compact form holds no empty chain)
			c2r_fail(ws.status, BMH_E_ARG);
			w.n = 0, ws.chn[c] = w;
			continue;
		}
		const bmh_seed_t *sd = in.seeds + sb;
		if (bmh_c2a_window(&p, l_pac, l_query, n, sd, &w.rmax0, &w.rmax1)) c2r_fail(ws.status, BMH_E_ARG);
		bmh_c2a_short_t sc;
		if (sw.msl > 0 && bmh_c2a_short_candidate(&p, l_pac, l_query, n, sd, &sc)) {
			const uint32_t idx = atomicAdd(&ws.status[C2R_N_SHORT], 1u);
			const int qlen = sc.sqe - sc.sqb;
			const bool xbyte = qlen * p.a < 250;
			w.sw_idx = (int32_t)idx, w.sqb = sc.sqb, w.sqe = sc.sqe, w.srb = sc.srb, w.sre = sc.sre, w.seedcov = sc.seedcov;
			if ((!(sw.wide_sw && !xbyte) && (long long)qlen * sw.max_mat >= kScoreLimit) || (sw.wraps && xbyte)) c2r_fail(ws.status, BMH_E_RANGE);
			if (idx < in.tc) { // bwamem.c:529-531
				bmh_sw_task_t t;
				t.q_off = q_off + (uint64_t)sc.sqb, t.t_off = (uint64_t)sc.srb;
				t.tlen = (uint32_t)(sc.sre - sc.srb), t.qlen = (uint16_t)qlen, t.flags = BMH_F_TPAC;
				t.xtra = BMH_SW_XSUBO | BMH_SW_XSTART | (xbyte ? BMH_SW_XBYTE : 0) | (uint32_t)(sw.msl * p.a);
				t.rsv = 0;
				ws.swt[idx] = t;
			} else c2r_fail(ws.status, BMH_E_ARG);
		}
		ws.chn[c] = w;
		// the (len, index) keys in the reference's order, bwamem.c:760-763; the last one is the seed it extends first
		uint64_t *srt = ws.srt + sb;
		for (int i = 0; i < n; ++i) srt[i] = (uint64_t)sd[i].len << 32 | (uint32_t)i, ws.slot[sb + i] = 0;
		c2r_sort(srt, n);
		const uint32_t top = (uint32_t)srt[n - 1];
		bmh_seed_task_t t;
		if (const int e = c2r_task(w, sd[top], q_off, l_query, &t)) {
			c2r_fail(ws.status, e);
			memset(&t, 0, sizeof(t));
		}
		ws.tasks[c] = t, ws.slot[sb + top] = (uint32_t)c + 1;
		sb += (unsigned long long)n;
	}
}

// appends the extension of seed si of chain c unless it was requested before
__device__ __forceinline__ void c2r_request(const C2rIn &in, const C2rWs &ws, const C2rChain &c, int si, uint64_t q_off, int l_query)
{
	uint32_t *slot = &ws.slot[c.seed_base + (uint64_t)si];
	if (*slot) return;
	bmh_seed_task_t t;
	if (const int e = c2r_task(c, in.seeds[c.seed_base + (uint64_t)si], q_off, l_query, &t)) { c2r_fail(ws.status, e); return; }
	const uint32_t idx = atomicAdd(&ws.status[C2R_N_TASKS], 1u);
	if (idx >= in.ts) { c2r_fail(ws.status, BMH_E_ARG); return; } // cannot happen: every seed is requested at most once
	ws.tasks[idx] = t, *slot = idx + 1;
}

// run_read() of the host driver for every unfinished read, with the results of tasks [0, n_done).  ext_cnt: the four list lengths
// of the launch_seedext just finished (null: none), added up for the statistics; ext_err: the extension kernels' error flag, moved
// into the status words so that one read-back carries everything.
__global__ __launch_bounds__(64) void c2r_replay_kernel(bmh_params_t p, C2rIn in, C2rWs ws, uint32_t n_done, const uint32_t *ext_cnt, int *ext_err)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r == 0) {
		if (ext_cnt) *(unsigned long long *)&ws.status[C2R_EXT_TASKS] += (unsigned long long)ext_cnt[0] + ext_cnt[1] + ext_cnt[2] + ext_cnt[3];
		const int e = *ext_err;
		if (e) c2r_fail(ws.status, e), *ext_err = 0;
	}
	if (r >= in.n_reads) return;
	C2rState s = ws.state[r];
	if (s.st == C2R_DONE) return;
	const unsigned long long c0 = in.coff[r], s0 = in.soff[r];
	const int nc = (int)(in.coff[r + 1] - c0);
	const size_t cap = (size_t)(in.soff[r + 1] - s0);
	bmh_alnreg_t *av = ws.reg + s0;
	size_t nav = (size_t)ws.nreg[r];
	const int l_query = in.len[r];
	const uint64_t q_off = in.read_off[r];
	unsigned long long n_ext = 0, n_skip = 0;
	bool stopped = false;
	C2rChain c = ws.chn[c0 + (unsigned long long)(s.ci < 0 ? 0 : s.ci)]; // (a read without chains is done before it is looked at)
	for (;;) {
		if (s.st == C2R_NEXT_CHAIN) {
			if (++s.ci >= nc) { s.st = C2R_DONE; break; }
			c = ws.chn[c0 + (unsigned long long)s.ci];
			if (c.sw_idx >= 0) { // the second half of mem_chain2aln_short, bwamem.c:533-541
				const bmh_sw_result_t x = ws.swr[c.sw_idx];
				if (!(x.tb < BMH_MEM_SHORT_EXT >> 1 || x.te > c.sre - c.srb - (BMH_MEM_SHORT_EXT >> 1))) {
					if (nav >= cap) { c2r_fail(ws.status, BMH_E_ARG); s.st = C2R_DONE; break; }
					bmh_alnreg_t a = {};
					a.rb = c.srb + x.tb, a.re = c.srb + x.te + 1;
					a.qb = c.sqb + x.qb, a.qe = c.sqb + x.qe + 1;
					a.score = x.score, a.csub = x.score2, a.seedcov = c.seedcov;
					av[nav++] = a;
					continue; // the chain is settled
				}
			}
			if (c.n == 0) continue; // bwamem.c:738
			s.k = c.n - 1, s.st = C2R_NEXT_SEED;
		} else {
			if (s.k < 0) { s.st = C2R_NEXT_CHAIN; continue; }
			uint64_t *srt = ws.srt + c.seed_base;
			const bmh_seed_t *sd = in.seeds + c.seed_base;
			const uint32_t si = (uint32_t)srt[s.k];
			const bmh_seed_t sdk = sd[si];
			if (bmh_c2a_seed_near_region(&p, &sdk, av, nav) && !bmh_c2a_has_conflicting_seed(sd, c.n, srt, s.k, &sdk)) {
				srt[s.k] = 0; // bwamem.c:796-799
				--s.k, ++n_skip;
				continue;
			}
			const uint32_t tix = ws.slot[c.seed_base + si];
			if (tix == 0 || tix - 1 >= n_done) { stopped = true; break; } // the device has not extended this seed yet
			if (nav >= cap) { c2r_fail(ws.status, BMH_E_ARG); s.st = C2R_DONE; break; }
			const bmh_seed_result_t x = ws.res[tix - 1];
			bmh_alnreg_t a = {}; // bwamem.c:804-807
			a.qb = x.qb, a.qe = x.qe, a.rb = c.rmax0 + x.rb, a.re = c.rmax0 + x.re; // bwamem.c:831-866
			a.score = x.score, a.truesc = x.truesc, a.w = x.w;                      // ... and :875
			a.seedcov = bmh_c2a_seedcov(sd, c.n, &a);
			av[nav++] = a;
			--s.k, ++n_ext;
		}
	}
	if (stopped) { // what this read may still need: the seed it stopped at, the rest of its chain, the later chains
		const uint64_t *srt = ws.srt + c.seed_base;
		const bmh_seed_t *sd = in.seeds + c.seed_base;
		c2r_request(in, ws, c, (int)(uint32_t)srt[s.k], q_off, l_query);
		for (int kk = s.k - 1; kk >= 0; --kk) {
			const int si = (int)(uint32_t)srt[kk];
			if (bmh_c2a_seed_near_region(&p, &sd[si], av, nav) && !bmh_c2a_may_conflict(sd, c.n, si)) continue; // provably skipped
			c2r_request(in, ws, c, si, q_off, l_query);
		}
		for (int ci = s.ci + 1; ci < nc; ++ci) {
			const C2rChain c2 = ws.chn[c0 + (unsigned long long)ci];
			const bmh_seed_t *sd2 = in.seeds + c2.seed_base;
			for (int si = 0; si < c2.n; ++si) {
				if (bmh_c2a_seed_near_region(&p, &sd2[si], av, nav) && !bmh_c2a_may_conflict(sd2, c2.n, si)) continue;
				c2r_request(in, ws, c2, si, q_off, l_query);
			}
		}
		atomicAdd(&ws.status[C2R_N_STOPPED], 1u);
	}
	ws.state[r] = s, ws.nreg[r] = nav;
	if (n_ext) atomicAdd((unsigned long long *)&ws.status[C2R_EXTENDED], n_ext);
	if (n_skip) atomicAdd((unsigned long long *)&ws.status[C2R_SKIPPED], n_skip);
}

// exclusive sums of one count array, n + 1 outputs (the last one is the total); one block of 1024 threads
__global__ __launch_bounds__(1024) void c2r_scan(const unsigned long long *__restrict__ a, int n, unsigned long long *__restrict__ pa)
{
	__shared__ unsigned long long sa[1024];
	const int t = threadIdx.x, per = (n + 1023) / 1024, lo = min(t * per, n), hi = min(lo + per, n);
	unsigned long long xa = 0;
	for (int k = lo; k < hi; ++k) xa += a[k];
	sa[t] = xa;
	__syncthreads();
	for (int d = 1; d < 1024; d <<= 1) {
		const unsigned long long ya = t >= d ? sa[t - d] : 0;
		__syncthreads();
		sa[t] += ya;
		__syncthreads();
	}
	unsigned long long ca = sa[t] - xa;
	for (int k = lo; k < hi; ++k) {
		pa[k] = ca;
		ca += a[k];
	}
	if (t == 1023) pa[n] = sa[1023];
}

// one lane per read copies its regions from its arena slice to the compact output
static_assert(sizeof(bmh_alnreg_t) == 64, "c2r_place_kernel copies a region as four uint4");
__global__ __launch_bounds__(64) void c2r_place_kernel(C2rIn in, C2rWs ws)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= in.n_reads) return;
	const unsigned long long n = ws.nreg[r], o = ws.roff[r], s0 = in.soff[r];
	if (o + n > in.ts || n > in.soff[r + 1] - s0) { c2r_fail(ws.status, BMH_E_ARG); return; }
	const uint4 *src = (const uint4 *)(ws.reg + s0);
	uint4 *dst = (uint4 *)(ws.out + o);
	for (unsigned long long k = 0; k < n * 4; ++k) dst[k] = src[k];
}

// What phase 2 learns from a walk over the host's vectors, from the compact records instead (host/handoff_core.h): one lane per read
// folds its vector, the wave folds its lanes with shuffles and writes its part, and one atomic per wave -- the ticket -- tells the last
// wave to arrive that every part is there; it folds them into the record.  Blocks are one wave.  The part and the ticket are
// wave_ticket.h's protocol, which mt_filter_kernel (matesw.hip) ends in as well.
struct HoFold {
	bmh_ho_plan_t p;
	int64_t pk;    // bmh_ho_pair's fold
	long long nsw; // a plain sum beside it
};

__device__ __forceinline__ void ho_fold_merge(HoFold &x, const HoFold &q)
{
	bmh_ho_merge(&x.p, &q.p), bmh_ho_pairs_merge(&x.pk, q.pk), x.nsw += q.nsw;
}

__device__ __forceinline__ void ho_wave_fold(HoFold &x)
{
	for (int d = 32; d >= 1; d >>= 1) {
		HoFold q;
		q.p.kmax = __shfl_xor((long long)x.p.kmax, d), q.p.opool_cap = __shfl_xor((long long)x.p.opool_cap, d);
		q.p.total = __shfl_xor((long long)x.p.total, d), q.p.neg = __shfl_xor(x.p.neg, d), q.p.rsv = 0;
		q.pk = __shfl_xor((long long)x.pk, d), q.nsw = __shfl_xor(x.nsw, d);
		ho_fold_merge(x, q);
	}
}

// every lane of the block's one wave arrives here with its own fold; part: the launch's parts, rec: its record with the ticket at 0
__device__ __forceinline__ void ho_plan_finish(HoFold x, long long *part, C2rPlan *rec)
{
	const int lane = threadIdx.x;
	ho_wave_fold(x);
	const long long w[5] = {(long long)x.p.kmax, (long long)x.p.opool_cap, (long long)x.p.total, (long long)(uint32_t)x.p.neg | (long long)x.pk << 32, x.nsw}; // (pk has 21 bits)
	if (!wave_ticket_publish<5, kPlanPartWords>(part, w, &rec->ticket)) return;
	HoFold t = {BMH_HO_PLAN_INIT, BMH_HO_PAIRS_INIT, 0};
	for (unsigned b = (unsigned)lane; b < gridDim.x; b += 64) {
		HoFold q;
		q.p.kmax = wave_ticket_word<kPlanPartWords>(part, b, 0), q.p.opool_cap = wave_ticket_word<kPlanPartWords>(part, b, 1);
		q.p.total = wave_ticket_word<kPlanPartWords>(part, b, 2);
		const long long w3 = wave_ticket_word<kPlanPartWords>(part, b, 3);
		q.p.neg = (int32_t)(w3 & 0xffffffffll), q.p.rsv = 0, q.pk = w3 >> 32;
		q.nsw = wave_ticket_word<kPlanPartWords>(part, b, 4);
		ho_fold_merge(t, q);
	}
	ho_wave_fold(t);
	if (lane == 0) rec->plan = t.p, rec->pair_kmax = t.pk, rec->n_sw = t.nsw;
}

// Over any table in c2r_place_kernel's form -- read r's regions at reg[roff[r] .. roff[r + 1]), cap records of room: phase 1's workspace
// behind c2r_scan, or what mate rescue leaves -- with the paired-end clause: a first mate (bmh_ho_first_mate) learns its mate's count
// from the lane beside it and folds the pair, and adds its pair's n_sw where the caller has such counts.  A single-end caller ignores
// the pairs' fold.  A read whose offsets leave the table sets *err and is not looked at.
__global__ __launch_bounds__(64) void table_plan_kernel(bmh_sam_opt_t o, int n_reads, const unsigned long long *__restrict__ roff, const bmh_alnreg_t *__restrict__ reg,
                                                        unsigned long long cap, const int *__restrict__ n_sw, long long *part, C2rPlan *rec, int *err)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	HoFold x = {BMH_HO_PLAN_INIT, BMH_HO_PAIRS_INIT, 0};
	long long n = 0;
	if (r < n_reads) {
		const unsigned long long at = roff[r], end = roff[r + 1];
		if (at > end || end > cap) atomicCAS(err, 0, BMH_E_ARG);
		else n = (long long)(end - at), bmh_ho_read(&o, reg + at, (int64_t)n, &x.p);
	}
	const long long mate = __shfl_xor(n, 1); // (64 is even: mates share a wave, and every lane of it is here)
	if (bmh_ho_first_mate(r, n_reads)) {
		bmh_ho_pair((int64_t)n, (int64_t)mate, &x.pk);
		if (n_sw) x.nsw = n_sw[r >> 1];
	}
	ho_plan_finish(x, part, rec);
}

size_t table_plan_part_bytes(int n_reads) { return ((size_t)n_reads / 64 + 1) * kPlanPartWords * sizeof(long long); }

int launch_table_plan(bmh_ctx *ctx, const bmh_sam_opt_t &o, int n_reads, const unsigned long long *d_roff, const bmh_alnreg_t *d_reg, unsigned long long cap,
                      const int *d_n_sw, void *d_part, void *d_rec, int *d_err)
{
	hipStream_t s = ctx->stream;
	if (ctx->timing) {
		for (hipEvent_t &e : ctx->ev_plan)
			if (!e) BMH_HIP(ctx, hipEventCreate(&e));
		BMH_HIP(ctx, hipEventRecord(ctx->ev_plan[0], s));
	}
	hipLaunchKernelGGL(table_plan_kernel, dim3((unsigned)std::max((n_reads + 63) / 64, 1)), dim3(64), 0, s, o, n_reads, d_roff, d_reg, cap, d_n_sw, (long long *)d_part,
	                   (C2rPlan *)d_rec, d_err);
	BMH_HIP(ctx, hipGetLastError());
	if (ctx->timing) BMH_HIP(ctx, hipEventRecord(ctx->ev_plan[1], s));
	return BMH_OK;
}

bool table_plan_read(const void *h_rec, int n_reads, ResidentRegs *out, long long *n_sw_sum)
{
	C2rPlan plan;
	memcpy(&plan, h_rec, sizeof(plan));
	if (plan.ticket != (uint32_t)std::max((n_reads + 63) / 64, 1) || plan.plan.total < 0 || plan.plan.opool_cap < 0 || plan.pair_kmax < 0 || plan.n_sw < 0) return false;
	out->total = (long long)plan.plan.total, out->kmax = (long long)plan.plan.kmax, out->opool_cap = (long long)plan.plan.opool_cap;
	out->neg = plan.plan.neg != 0, out->pair_kmax = (long long)plan.pair_kmax;
	if (n_sw_sum) *n_sw_sum = (long long)plan.n_sw;
	return true;
}

// mem_sort_and_dedup (host/dedup_core.h, the text bmh_sort_and_dedup runs) on read r's slice of a region array, one lane per read.
// The range stack of the two introsorts is the lane's own: bmh_sort_stack_len(n) <= 33 entries for n < 2^31.
constexpr int kDedupStk = 34;
__global__ __launch_bounds__(64) void region_dedup_kernel(bmh_alnreg_t *reg, const unsigned long long *__restrict__ off, unsigned long long *cnt, int n_reads,
                                                          unsigned long long total, float mask_level_redun, unsigned long long *removed, int *err)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads) return;
	const unsigned long long n = cnt[r], o = off[r];
	if (n <= 1) return;
	if (n > 0x7fffffffull || o > total || n > total - o) { atomicCAS(err, 0, BMH_E_ARG); return; }
	bmh_sort_stk_t stk[kDedupStk];
	const unsigned long long m = (unsigned long long)bmh_dedup_core((int)n, reg + o, mask_level_redun, stk);
	if (m != n) cnt[r] = m, atomicAdd(removed, n - m);
}

int launch_region_dedup(bmh_ctx *ctx, bmh_alnreg_t *d_reg, const unsigned long long *d_off, unsigned long long *d_cnt, int n_reads,
                        unsigned long long total, float mask_level_redun, unsigned long long *d_removed, int *d_err)
{
	if (n_reads <= 0) return BMH_OK;
	if (ctx->timing) {
		if (!ctx->ev_dedup[0]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_dedup[0]));
		if (!ctx->ev_dedup[1]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_dedup[1]));
		BMH_HIP(ctx, hipEventRecord(ctx->ev_dedup[0], ctx->stream));
	}
	hipLaunchKernelGGL(region_dedup_kernel, dim3((unsigned)((n_reads + 63) / 64)), dim3(64), 0, ctx->stream, d_reg, d_off, d_cnt, n_reads, total,
	                   mask_level_redun, d_removed, d_err);
	BMH_HIP(ctx, hipGetLastError());
	if (ctx->timing) BMH_HIP(ctx, hipEventRecord(ctx->ev_dedup[1], ctx->stream));
	return BMH_OK;
}

} // namespace bmh

using namespace bmh;

namespace {

struct C2rLayout {
	size_t status, chn, state, srt, slot, tasks, res, swt, swr, reg, nreg, roff, cand, out, part, total;
	C2rLayout(size_t n, size_t tc, size_t ts)
	{
		size_t o = 0;
		auto take = [&](size_t bytes) {
			const size_t at = o;
			o += al256(bytes);
			return at;
		};
		status = take(C2R_STATUS_BYTES + sizeof(C2rPlan)), chn = take((tc + 1) * sizeof(C2rChain)), state = take(n * sizeof(C2rState)), srt = take(ts * 8);
		slot = take(ts * 4), tasks = take(ts * sizeof(bmh_seed_task_t)), res = take(ts * sizeof(bmh_seed_result_t));
		swt = take(tc * sizeof(bmh_sw_task_t)), swr = take(tc * sizeof(bmh_sw_result_t)), reg = take(ts * sizeof(bmh_alnreg_t));
		nreg = take((n + 1) * 8), roff = take((n + 1) * 8 + (n / 2 + 1) * 4), cand = roff + (n + 1) * 8; // (the words share roff's block)
		out = take(ts * sizeof(bmh_alnreg_t)), part = take((n / 64 + 1) * kPlanPartWords * sizeof(long long)), total = o;
	}
};

// What runs behind the replay loop: the context's switches for the two calls that fill the host's vectors (c2r_post_of), a session's own
// for the two that leave the regions resident.  collect_opt: the options the words are collected under.
struct C2rPost {
	bool dedup;
	float mask;
	bool drop, collect;
	bmh_sam_opt_t collect_opt;
};

// (a NULL context is c2r_check's to refuse)
C2rPost c2r_post_of(const bmh_ctx *ctx)
{
	return ctx ? C2rPost{ctx->regs_dedup, ctx->regs_dedup_mask, ctx->regs_drop_exact, ctx->pestat_collect, ctx->pestat_opt} : C2rPost{false, 0.f, false, false, {}};
}

// The workspace of a call, at the start of ctx->d_c2r (a caller that keeps its own input there puts it behind C2rLayout::total and has
// made the buffer large enough), and room in ctx->h_down for the status record and down_extra bytes behind it.
int c2r_workspace(bmh_ctx *ctx, const C2rIn &in, size_t down_extra, C2rWs *ws)
{
	const C2rLayout L((size_t)in.n_reads, (size_t)in.tc, (size_t)in.ts);
	int rc;
	if ((rc = ensure(ctx, ctx->d_c2r, L.total)) || (rc = ensure_host(ctx, ctx->h_down, 256 + down_extra))) return rc;
	uint8_t *d = (uint8_t *)ctx->d_c2r.p;
	*ws = C2rWs{(uint32_t *)(d + L.status), (C2rChain *)(d + L.chn), (C2rState *)(d + L.state), (uint64_t *)(d + L.srt), (uint32_t *)(d + L.slot),
	            (bmh_seed_task_t *)(d + L.tasks), (bmh_seed_result_t *)(d + L.res), (bmh_sw_task_t *)(d + L.swt), (bmh_sw_result_t *)(d + L.swr),
	            (bmh_alnreg_t *)(d + L.reg), (unsigned long long *)(d + L.nreg), (unsigned long long *)(d + L.roff), (uint32_t *)(d + L.cand),
	            (bmh_alnreg_t *)(d + L.out), (long long *)(d + L.part)};
	return BMH_OK;
}

// The window kernel, a 16-byte look at the status words, and the short chains' Smith-Watermans
int c2r_windows(bmh_ctx *ctx, int64_t l_pac, const uint8_t *d_pool, const C2rIn &in, const C2rWs &ws, int msl, bmh_driver_stats_t *st)
{
	const bmh_params_t &p = ctx->params;
	const C2rSwRule sw{msl, ctx->dev.max_mat, ctx->wide_sw ? 1 : 0, sw_byte_gaps_wrap(p) ? 1 : 0};
	uint32_t *h = (uint32_t *)ctx->h_down.p;
	hipStream_t s = ctx->stream;
	int rc;
	hipLaunchKernelGGL(c2r_window_kernel, dim3((unsigned)((in.n_reads + 63) / 64)), dim3(64), 0, s, p, l_pac, in, ws, sw);
	BMH_HIP(ctx, hipGetLastError());
	BMH_HIP(ctx, hipMemcpyAsync(h, ws.status, 16, hipMemcpyDeviceToHost, s));
	BMH_HIP(ctx, stream_wait(ctx, s));
	if ((int)h[C2R_ERR]) {
		ctx->last_error = (int)h[C2R_ERR] == BMH_E_RANGE ? "chains to regions: a seed outside its chain's window, a window over 2^31, or a short-chain task outside the Smith-Waterman range"
		                                                 : "chains to regions: the chains are inconsistent (a seed outside its read, offsets outside the arrays, or a chain off the doubled coordinate)";
		return (int)h[C2R_ERR];
	}
	const uint32_t n_short = h[C2R_N_SHORT];
	st->short_sw = n_short;
	// mem_chain2aln_short's bounds (bmh_c2a_short_candidate): qlen, tlen < MEM_SHORT_LEN, and qlen > 2 * MEM_SHORT_EXT.
	// The caps are given, and must stay given: in the fused call d_pool lies in ctx->d_scratch, which launch_sw's own reduction of
	// the caps (qcap < 0) would reallocate or overwrite.  Nothing else between here and the gather touches d_scratch.
	if (n_short && (rc = launch_sw(ctx, d_pool, ws.swt, n_short, ws.swr, BMH_MEM_SHORT_LEN - 1, BMH_MEM_SHORT_LEN - 1, 2 * BMH_MEM_SHORT_EXT + 1)))
		return abandon_call(ctx, rc);
	return BMH_OK;
}

// The replay rounds, up to the one in which no read stops: a 16-byte look at the status words per round.  *n_tasks_: the extensions
// requested in all.
int c2r_rounds(bmh_ctx *ctx, const uint8_t *d_pool, const C2rIn &in, const C2rWs &ws, int lmax, bmh_driver_stats_t *st, uint32_t *n_tasks_)
{
	const bmh_params_t &p = ctx->params;
	const unsigned rb = (unsigned)((in.n_reads + 63) / 64);
	uint32_t *h = (uint32_t *)ctx->h_down.p;
	hipStream_t s = ctx->stream;
	int rc;
	const int qmax = std::max(lmax, 1); // no flank is longer than its read
	uint32_t n_done = 0, n_tasks = (uint32_t)in.tc; // round 1: the task of chain c at index c (the window kernel set the counter to tc)
	for (;;) {
		const bool ext = n_tasks > n_done;
		if (ext) {
			++st->rounds;
			if ((rc = launch_seedext(ctx, d_pool, ws.tasks + n_done, (int64_t)(n_tasks - n_done), ws.res + n_done, qmax))) return abandon_call(ctx, rc);
			n_done = n_tasks;
		}
		BMH_HIP(ctx, hipMemsetAsync(&ws.status[C2R_N_STOPPED], 0, 4, s));
		hipLaunchKernelGGL(c2r_replay_kernel, dim3(rb), dim3(64), 0, s, p, in, ws, n_done, ext ? seedext_counters(ctx) : nullptr, ctx->d_err);
		BMH_HIP(ctx, hipGetLastError());
		BMH_HIP(ctx, hipMemcpyAsync(h, ws.status, 16, hipMemcpyDeviceToHost, s));
		BMH_HIP(ctx, stream_wait(ctx, s));
		if ((int)h[C2R_ERR]) {
			ctx->last_error = (int)h[C2R_ERR] == BMH_E_RANGE ? "chains to regions: a task was outside the supported range (see bwamem_hip.h)"
			                                                 : "chains to regions: a seed outside its read, or a read's regions do not fit its arena slice";
			return (int)h[C2R_ERR];
		}
		n_tasks = h[C2R_N_TASKS];
		if (h[C2R_N_STOPPED] == 0) break;
		if (n_tasks == n_done) { // cannot happen: a stopped read always asks for its seed
			ctx->last_error = "chains to regions: a read is stopped and nothing was requested";
			return BMH_E_ARG;
		}
	}
	*n_tasks_ = n_tasks;
	return BMH_OK;
}

// The driver proper, on the context's stream, the same for every caller: the two steps above, what post switches on, then the gather.
// It returns behind c2r_place_kernel without having read the final status words: that is the tail's wait.
int c2r_enqueue(bmh_ctx *ctx, int64_t l_pac, const uint8_t *d_pool, const C2rIn &in, const C2rWs &ws, int lmax, int msl, bmh_driver_stats_t *st,
                const C2rPost &post, uint32_t *n_tasks)
{
	const int n = in.n_reads;
	hipStream_t s = ctx->stream;
	int rc;
	BMH_HIP(ctx, hipMemsetAsync(ws.status, 0, C2R_STATUS_BYTES + sizeof(C2rPlan), s)); // the error flag starts clean on every call, and the plan's ticket at 0
	if ((rc = c2r_windows(ctx, l_pac, d_pool, in, ws, msl, st)) || (rc = c2r_rounds(ctx, d_pool, in, ws, lmax, st, n_tasks))) return rc;
	// with the switch on: mem_sort_and_dedup on every read's arena slice, so that the gather places and downloads the survivors only
	if (post.dedup && (rc = launch_region_dedup(ctx, ws.reg, in.soff, ws.nreg, n, in.ts, post.mask, (unsigned long long *)&ws.status[C2R_DEDUP_REMOVED],
	                                            (int *)&ws.status[C2R_ERR])))
		return rc;
	// with either of its switches on: mem_test_and_remove_exact on the survivors, then mem_pestat's word per pair from what is left
	if ((post.collect || post.drop) &&
	    (rc = launch_pestat_collect(ctx, ws.reg, in.soff, ws.nreg, in.len, n, in.ts, post.collect_opt, l_pac, ctx->params.a, post.drop, post.collect ? ws.cand : nullptr,
	                                (unsigned long long *)&ws.status[C2R_DROP_REMOVED], (int *)&ws.status[C2R_ERR])))
		return rc;
	// gather: count -> scan -> place
	hipLaunchKernelGGL(c2r_scan, dim3(1), dim3(1024), 0, s, (const unsigned long long *)ws.nreg, n, ws.roff);
	hipLaunchKernelGGL(c2r_place_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, in, ws);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

// What every tail does behind its wait, the status words in ctx->h_down and tr the total as the tail learnt it: the status check, the
// driver's statistics and those of the switches.  *chains_in (not null): the chains before the filter, also of a refused call.
struct C2rCounts {
	unsigned long long tr, removed, dropped; // regions left, removed by the de-duplication, removed by drop-exact
	float pestat_ms;
};
int c2r_settle(bmh_ctx *ctx, const C2rIn &in, const C2rPost &post, unsigned long long tr, uint32_t n_tasks, bmh_driver_stats_t *st, long long *chains_in, C2rCounts *c)
{
	const uint32_t *h = (const uint32_t *)ctx->h_down.p;
	unsigned long long u64s[4];
	*c = C2rCounts{tr, 0, 0, -1.f};
	memcpy(u64s, h + C2R_EXT_TASKS, 32), memcpy(&c->removed, h + C2R_DEDUP_REMOVED, 8), memcpy(&c->dropped, h + C2R_DROP_REMOVED, 8);
	if (chains_in) *chains_in = (long long)u64s[3];
	if ((int)h[C2R_ERR] || tr > in.ts) {
		ctx->last_error = "chains to regions: the region counts are inconsistent";
		return BMH_E_ARG;
	}
	st->ext_tasks = (int64_t)u64s[0], st->seeds_extended = (int64_t)u64s[1], st->seeds_skipped = (int64_t)u64s[2];
	st->seeds_speculated = (int64_t)n_tasks - st->seeds_extended; // extended on the device but never used
	if (post.dedup) { // (the driver's statistics are about extensions and stay what they are without the switch)
		ctx->dedup_in = (long long)(tr + c->dropped + c->removed), ctx->dedup_out = (long long)(tr + c->dropped), ctx->dedup_ms = -1.f;
		if (ctx->timing) BMH_HIP(ctx, hipEventElapsedTime(&ctx->dedup_ms, ctx->ev_dedup[0], ctx->ev_dedup[1]));
	}
	if ((post.collect || post.drop) && ctx->timing) BMH_HIP(ctx, hipEventElapsedTime(&c->pestat_ms, ctx->ev_pestat[0], ctx->ev_pestat[1]));
	if (post.drop) ctx->drop_exact_removed = (long long)c->dropped;
	return BMH_OK;
}

// gives back the arrays of reads [0, upto) -- those this call made, not what a caller left in the .a of a read without regions
void c2r_free_vectors(int upto, const unsigned long long *roff, bmh_alnreg_v *regs)
{
	for (int q = 0; q < upto; ++q)
		if (roff[q + 1] > roff[q]) free(regs[q].a), regs[q].a = nullptr, regs[q].n = regs[q].m = 0;
}

// regs[r] receive malloc'd arrays with n == m, cut from the downloaded table; a read without regions is left as the caller gave it
int c2r_make_vectors(bmh_ctx *ctx, int n, const unsigned long long *roff, const bmh_alnreg_t *ra, bmh_alnreg_v *regs)
{
	for (int r = 0; r < n; ++r) {
		const size_t k = (size_t)(roff[r + 1] - roff[r]);
		if (!k) continue;
		bmh_alnreg_t *a = (bmh_alnreg_t *)malloc(k * sizeof(bmh_alnreg_t));
		if (!a) {
			c2r_free_vectors(r, roff, regs);
			ctx->last_error = "chains to regions: out of host memory for the regions";
			return BMH_E_NOMEM;
		}
		memcpy(a, ra + roff[r], k * sizeof(bmh_alnreg_t));
		regs[r].a = a, regs[r].n = regs[r].m = k;
	}
	return BMH_OK;
}

// Tail 1, vectors for the host (bmh_chains2regs_device, bmh_seed_chain_regs_batch): the status words and the total in one wait, the
// offsets -- with the insert-size words right behind them -- and the compact records in a second.
int c2r_tail_vectors(bmh_ctx *ctx, const C2rIn &in, const C2rWs &ws, const C2rPost &post, uint32_t n_tasks, bmh_driver_stats_t *st, long long *chains_in,
                     bmh_alnreg_v *regs)
{
	const int n = in.n_reads;
	uint32_t *h = (uint32_t *)ctx->h_down.p;
	hipStream_t s = ctx->stream;
	BMH_HIP(ctx, hipMemcpyAsync(h, ws.status, C2R_STATUS_BYTES, hipMemcpyDeviceToHost, s));
	BMH_HIP(ctx, hipMemcpyAsync(h + 16, &ws.roff[n], 8, hipMemcpyDeviceToHost, s));
	BMH_HIP(ctx, stream_wait(ctx, s));
	unsigned long long tr;
	memcpy(&tr, h + 16, 8);
	C2rCounts c;
	int rc;
	if ((rc = c2r_settle(ctx, in, post, tr, n_tasks, st, chains_in, &c))) return rc;
	const size_t b_roff = ((size_t)n + 1) * 8 + (post.collect ? ((size_t)n / 2) * 4 : 0);
	const size_t b_off = al256(b_roff + 4), b_reg = (size_t)tr * sizeof(bmh_alnreg_t);
	if ((rc = ensure_host(ctx, ctx->h_down, b_off + b_reg + 64))) return rc;
	uint8_t *hb = (uint8_t *)ctx->h_down.p;
	BMH_HIP(ctx, hipMemcpyAsync(hb, ws.roff, b_roff, hipMemcpyDeviceToHost, s));
	if (b_reg) BMH_HIP(ctx, hipMemcpyAsync(hb + b_off, ws.out, b_reg, hipMemcpyDeviceToHost, s));
	BMH_HIP(ctx, stream_wait(ctx, s));
	const unsigned long long *roff = (const unsigned long long *)hb;
	if ((rc = c2r_make_vectors(ctx, n, roff, (const bmh_alnreg_t *)(hb + b_off), regs))) return rc;
	if (post.collect) { // of a successful call only (bmh_last_pestat_candidates)
		const uint32_t *w = (const uint32_t *)(hb + ((size_t)n + 1) * 8);
		try {
			ctx->pestat_cand.assign(w, w + n / 2);
		} catch (const std::bad_alloc &) {
			c2r_free_vectors(n, roff, regs);
			ctx->last_error = "chains to regions: out of host memory for the insert-size words";
			return BMH_E_NOMEM;
		}
		ctx->pestat_pairs = n / 2, ctx->pestat_ms = c.pestat_ms;
	}
	return BMH_OK;
}

// Tail 2, resident regions with the plan (reads_regs_resident): the compact records stay in ws.out, their offsets in ws.roff -- a table
// with in.ts records of room --, table_plan_kernel folds them into the record behind the status words, and the 128 bytes of both come
// down in the hand-off's one wait.  *out and ctx->rs up to the hand-off are the call's.
int c2r_tail_plan(bmh_ctx *ctx, const C2rIn &in, const C2rWs &ws, const C2rPost &post, uint32_t n_tasks, bmh_driver_stats_t *st, long long *chains_in,
                  const bmh_sam_opt_t &o, ResidentRegs *out)
{
	const int n = in.n_reads;
	uint32_t *h = (uint32_t *)ctx->h_down.p;
	hipStream_t s = ctx->stream;
	int rc;
	if ((rc = launch_table_plan(ctx, o, n, ws.roff, ws.out, in.ts, nullptr, ws.part, (uint8_t *)ws.status + C2R_STATUS_BYTES, (int *)&ws.status[C2R_ERR]))) return rc;
	BMH_HIP(ctx, hipMemcpyAsync(h, ws.status, C2R_STATUS_BYTES + sizeof(C2rPlan), hipMemcpyDeviceToHost, s));
	BMH_HIP(ctx, stream_wait(ctx, s));
	ResidentRegs R;
	const bool whole = table_plan_read(h + C2R_STATUS_BYTES / 4, n, &R, nullptr); // (false cannot happen: refused as a total past the table)
	C2rCounts c;
	if ((rc = c2r_settle(ctx, in, post, whole ? (unsigned long long)R.total : in.ts + 1, n_tasks, st, chains_in, &c))) return rc;
	R.roff = ws.roff, R.reg = ws.out, R.pair_kmax = 0; // (single-end reads: what the kernel folds over neighbours is no pair's)
	*out = R;
	ctx->rs = bmh_reads_sam_stats_t{n, (int64_t)(c.tr + c.dropped + c.removed), (int64_t)c.tr, R.kmax, R.opool_cap, (int64_t)(C2R_STATUS_BYTES + sizeof(C2rPlan)),
	                                1, -1.f, R.neg ? 1 : 0, 0};
	if (ctx->timing) BMH_HIP(ctx, hipEventElapsedTime(&ctx->rs.plan_ms, ctx->ev_plan[0], ctx->ev_plan[1]));
	return BMH_OK;
}

// Tail 3, resident regions with the total and the words (pairs_regs_resident): no plan -- mate rescue changes the table first --, the
// total comes down beside the status words and the insert-size words, collected into out->cand's room, behind them in the same wait.
// ctx->rs and the context's words are left alone.
int c2r_tail_pairs(bmh_ctx *ctx, const C2rIn &in, const C2rWs &ws, const C2rPost &post, uint32_t n_tasks, bmh_driver_stats_t *st, long long *chains_in,
                   PairsPhase1 *out)
{
	const int n = in.n_reads;
	const size_t b_words = post.collect ? out->cand.size() * 4 : 0;
	uint32_t *h = (uint32_t *)ctx->h_down.p;
	hipStream_t s = ctx->stream;
	BMH_HIP(ctx, hipMemcpyAsync(h, ws.status, C2R_STATUS_BYTES, hipMemcpyDeviceToHost, s));
	BMH_HIP(ctx, hipMemcpyAsync(h + 16, &ws.roff[n], 8, hipMemcpyDeviceToHost, s));
	if (b_words) BMH_HIP(ctx, hipMemcpyAsync(h + 64, ws.cand, b_words, hipMemcpyDeviceToHost, s));
	BMH_HIP(ctx, stream_wait(ctx, s));
	unsigned long long tr;
	memcpy(&tr, h + 16, 8);
	C2rCounts c;
	int rc;
	if ((rc = c2r_settle(ctx, in, post, tr, n_tasks, st, chains_in, &c))) return rc;
	out->regs = ResidentRegs{};
	out->regs.roff = ws.roff, out->regs.reg = ws.out, out->regs.total = (long long)tr;
	out->regions_in = (long long)(tr + c.dropped + c.removed), out->d2h_bytes = (long long)(C2R_STATUS_BYTES + 8 + b_words);
	if (b_words) memcpy(out->cand.data(), h + 64, b_words);
	return BMH_OK;
}

// a successful call without reads ran no kernel: what the switches report of "the last successful call" is that of an empty batch
void c2r_empty(bmh_ctx *ctx)
{
	if (ctx->pestat_collect) ctx->pestat_cand.clear(), ctx->pestat_pairs = 0, ctx->pestat_ms = -1.f;
	if (ctx->regs_drop_exact) ctx->drop_exact_removed = 0;
}

// with_regs false: a call that makes no vectors (the resident tails), post being its own and not the context's switches
int c2r_check(bmh_ctx *ctx, int64_t l_pac, int n_reads, const bmh_read_t *reads, int min_seed_len, const bmh_alnreg_v *regs, const char *who,
              const C2rPost &post, bool with_regs = true)
{
	if (!ctx || n_reads < 0 || l_pac < 0 || min_seed_len < 0 || (n_reads > 0 && (!reads || (with_regs && !regs)))) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	// the two switches behind the de-duplication (pestat.hip): refused here, before anything is enqueued; the switches stay as set
	if ((post.collect || post.drop) && !post.dedup) {
		ctx->last_error = std::string(who) + ": " + (post.collect ? "bmh_ctx_set_pestat_collect" : "bmh_ctx_set_regs_drop_exact") +
		                  " is on, which needs bmh_ctx_set_regs_dedup on: both run on the regions mem_sort_and_dedup leaves";
		return BMH_E_ARG;
	}
	if (post.collect && (n_reads & 1)) {
		ctx->last_error = std::string(who) + ": bmh_ctx_set_pestat_collect is on and n_reads is odd: reads 2p and 2p+1 are mates";
		return BMH_E_ARG;
	}
	if (post.collect && post.collect_opt.max_ins > BMH_PS_MAX_INS) {
		ctx->last_error = std::string(who) + ": bmh_ctx_set_pestat_collect is on with max_ins >= 2^30, which the word cannot hold";
		return BMH_E_RANGE;
	}
	if (!ctx->dev.pac || ctx->dev.l_pac != l_pac) {
		ctx->last_error = std::string(who) + ": needs the 2-bit reference of this l_pac resident on the device (bmh_ctx_set_pac)";
		return BMH_E_ARG;
	}
	for (int r = 0; r < n_reads; ++r)
		if (reads[r].l_seq > 65535) {
			ctx->last_error = std::string(who) + ": read " + std::to_string(r) + " is longer than 65535 bases";
			return BMH_E_RANGE;
		}
	for (int r = 0; with_regs && r < n_reads; ++r)
		if (regs[r].n) {
			ctx->last_error = std::string(who) + ": regs[" + std::to_string(r) + "] is not empty";
			return BMH_E_ARG;
		}
	return BMH_OK;
}

// what the fused call refuses of its two option records
int fused_check_opts(bmh_ctx *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, const char *who)
{
	if (co->min_seed_len < 0 || co->max_occ < 0) return BMH_E_ARG;
	if (so->min_seed_len != co->min_seed_len || so->split_len != co->split_len || so->split_width != co->split_width || so->min_emit_len < 0 ||
	    so->min_emit_len > co->min_seed_len) {
		ctx->last_error = std::string(who) + ": min_seed_len / split_len / split_width must agree and min_emit_len <= min_seed_len";
		return BMH_E_ARG;
	}
	return BMH_OK;
}

enum C2rTail { kTailVectors, kTailPlan, kTailPairs };
struct FusedArgs {
	const bmh_chain_opt_t *co;
	int64_t l_pac;
	int lmax, msl;
	bmh_driver_stats_t *st;
	C2rPost post;
	C2rTail tail;
	bmh_alnreg_v *regs = nullptr;              // kTailVectors: the caller's vectors
	const bmh_sam_opt_t *plan_opt = nullptr;   // kTailPlan: the options of the plan ...
	ResidentRegs *resident = nullptr;          // ... and where the table and the plan are reported
	PairsPhase1 *pairs = nullptr;              // kTailPairs: the table, the words (cand sized by the caller) and the bases
	size_t bases = 0;                          // ... the bases of all reads
};

// The bases where nothing between here and mate rescue's last round writes: seeding's pool lies in ctx->d_scratch, which launch_sw may
// reallocate or overwrite, and the rescue's rounds call launch_sw.  ctx->d_pbase is this copy's alone: [soff[n + 1] | the reads | 16
// zero bytes], matesw_resident's form.  Seeding laid the reads end to end in read order, so the pool moves as one copy.
__global__ __launch_bounds__(256) void bases_soff_kernel(const uint64_t *__restrict__ read_off, const int *__restrict__ len, int n, unsigned long long *__restrict__ soff)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n) return;
	soff[r] = read_off[r];
	if (r == n - 1) soff[n] = read_off[r] + (unsigned long long)len[r];
}

int bases_keep(bmh_ctx *ctx, const DevSeedTables &t, size_t bytes, PairsPhase1 *out)
{
	const size_t n = (size_t)t.n_reads, o_pool = al256((n + 1) * 8);
	int rc;
	if ((rc = ensure(ctx, ctx->d_pbase, o_pool + bytes + 16))) return rc;
	uint8_t *d = (uint8_t *)ctx->d_pbase.p;
	hipStream_t s = ctx->stream;
	if (n) hipLaunchKernelGGL(bases_soff_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t.read_off, t.len, (int)n, (unsigned long long *)d);
	else BMH_HIP(ctx, hipMemsetAsync(d, 0, 8, s));
	BMH_HIP(ctx, hipGetLastError());
	if (bytes) BMH_HIP(ctx, hipMemcpyAsync(d + o_pool, t.pool, bytes, hipMemcpyDeviceToDevice, s));
	BMH_HIP(ctx, hipMemsetAsync(d + o_pool + bytes, 0, 16, s));
	out->soff = (const unsigned long long *)d, out->pool = d + o_pool;
	return BMH_OK;
}

// seeding's tables -> compact chains -> regions, all where they lie on the device; the reads are the pool seeding uploaded
int fused_cb(bmh_ctx *ctx, const DevSeedTables &t, void *user)
{
	const FusedArgs *u = (const FusedArgs *)user;
	DevChains dc;
	int rc;
	if ((rc = chain_compact_device(ctx, u->co, u->l_pac, t, &dc))) return rc;
	const int n = t.n_reads;
	// (the chains before the filter, for bmh_chain_stats, are summed on the device and come back in the status words)
	const C2rIn in{n, t.read_off, t.len, dc.coff, dc.soff, dc.cn, dc.seeds, dc.tc, dc.ts, dc.n_keys};
	long long before = 0;
	C2rWs ws;
	uint32_t n_tasks;
	const size_t b_words = u->tail == kTailPairs && u->post.collect ? u->pairs->cand.size() * 4 : 0; // come down behind the status record
	if ((rc = c2r_workspace(ctx, in, b_words, &ws)) || (rc = c2r_enqueue(ctx, u->l_pac, t.pool, in, ws, u->lmax, u->msl, u->st, u->post, &n_tasks))) return rc;
	if (u->tail == kTailVectors) rc = c2r_tail_vectors(ctx, in, ws, u->post, n_tasks, u->st, &before, u->regs);
	else if (u->tail == kTailPlan) rc = c2r_tail_plan(ctx, in, ws, u->post, n_tasks, u->st, &before, *u->plan_opt, u->resident);
	else rc = c2r_tail_pairs(ctx, in, ws, u->post, n_tasks, u->st, &before, u->pairs);
	if (rc) return rc;
	if (u->tail == kTailPairs && (rc = bases_keep(ctx, t, u->bases, u->pairs))) return rc;
	ctx->cstats = bmh_chain_stats_t{n, before, (int64_t)dc.tc, (int64_t)dc.ts, (int64_t)dc.n_equal, dc.kernel_ms}; // of a successful call only
	return BMH_OK;
}

} // namespace

extern "C" {

int bmh_chains2regs_device(bmh_ctx_t *ctx, int64_t l_pac, int n_reads, const bmh_read_t *reads, const bmh_chain_v *chains, int min_seed_len,
                           bmh_alnreg_v *regs)
{
	int rc;
	if ((rc = c2r_check(ctx, l_pac, n_reads, reads, min_seed_len, regs, "bmh_chains2regs_device", c2r_post_of(ctx)))) return rc;
	if (n_reads > 0 && !chains) return BMH_E_ARG;
	bmh_driver_stats_t st{};
	ctx->dstats = st;
	if (n_reads == 0) {
		c2r_empty(ctx);
		return BMH_OK;
	}
	// the compact form of the chains (empty chains do nothing in the reference's loop and are left out), and the reads
	size_t tc = 0, ts = 0, bytes = 0;
	int lmax = 1;
	for (int r = 0; r < n_reads; ++r) {
		if (reads[r].l_seq < 0 || (reads[r].l_seq > 0 && !reads[r].seq) || (chains[r].n && !chains[r].a)) return BMH_E_ARG;
		bytes += (size_t)reads[r].l_seq, lmax = std::max(lmax, reads[r].l_seq);
		for (size_t c = 0; c < chains[r].n; ++c)
			if (chains[r].a[c].n > 0) {
				if (!chains[r].a[c].seeds) return BMH_E_ARG;
				++tc, ts += (size_t)chains[r].a[c].n;
			}
	}
	if (tc > 0x7fffffffu || ts > 0x7fffffffu) return BMH_E_ARG;
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	const size_t nr1 = (size_t)n_reads + 1;
	const size_t i_pool = 0, i_off = al256(bytes + 16), i_len = i_off + al256(nr1 * 8), i_coff = i_len + al256(nr1 * 4), i_soff = i_coff + al256(nr1 * 8),
	             i_cn = i_soff + al256(nr1 * 8), i_seed = i_cn + al256((tc + 1) * 4), i_total = i_seed + al256((ts + 1) * sizeof(bmh_seed_t));
	const C2rLayout L((size_t)n_reads, tc, ts);
	if ((rc = ensure(ctx, ctx->d_c2r, L.total + i_total)) || (rc = ensure_host(ctx, ctx->h_up, i_total))) return rc;
	uint8_t *h = (uint8_t *)ctx->h_up.p;
	uint64_t *off = (uint64_t *)(h + i_off);
	int *len = (int *)(h + i_len);
	unsigned long long *coff = (unsigned long long *)(h + i_coff), *soff = (unsigned long long *)(h + i_soff);
	uint32_t *cn = (uint32_t *)(h + i_cn);
	bmh_seed_t *sd = (bmh_seed_t *)(h + i_seed);
	size_t at = 0, c_at = 0, s_at = 0;
	for (int r = 0; r < n_reads; ++r) {
		off[r] = at, len[r] = reads[r].l_seq, coff[r] = c_at, soff[r] = s_at;
		if (reads[r].l_seq) memcpy(h + i_pool + at, reads[r].seq, (size_t)reads[r].l_seq);
		at += (size_t)reads[r].l_seq;
		for (size_t c = 0; c < chains[r].n; ++c) {
			const bmh_chain_t &ch = chains[r].a[c];
			if (ch.n <= 0) continue;
			cn[c_at++] = (uint32_t)ch.n;
			memcpy(sd + s_at, ch.seeds, (size_t)ch.n * sizeof(bmh_seed_t));
			s_at += (size_t)ch.n;
		}
	}
	off[n_reads] = at, coff[n_reads] = c_at, soff[n_reads] = s_at;
	memset(h + i_pool + bytes, 0, i_off - bytes);
	uint8_t *d = (uint8_t *)ctx->d_c2r.p + L.total;
	BMH_HIP(ctx, hipMemcpyAsync(d, h, i_total, hipMemcpyHostToDevice, ctx->stream));
	st.pool_bytes = (int64_t)bytes + 16; // the reads and the 16 bytes of padding behind them, as the host driver counts its pool
	const C2rIn in{n_reads, (const uint64_t *)(d + i_off), (const int *)(d + i_len), (const unsigned long long *)(d + i_coff),
	               (const unsigned long long *)(d + i_soff), (const uint32_t *)(d + i_cn), (const bmh_seed_t *)(d + i_seed), tc, ts, nullptr};
	const C2rPost post = c2r_post_of(ctx);
	C2rWs ws;
	uint32_t n_tasks;
	if (!(rc = c2r_workspace(ctx, in, 0, &ws)) && !(rc = c2r_enqueue(ctx, l_pac, d + i_pool, in, ws, lmax, min_seed_len, &st, post, &n_tasks)))
		rc = c2r_tail_vectors(ctx, in, ws, post, n_tasks, &st, nullptr, regs);
	ctx->dstats = st;
	return rc;
}

int bmh_seed_chain_regs_batch(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac, int n_reads,
                              const bmh_read_t *reads, int min_seed_len, bmh_alnreg_v *regs)
{
	int rc;
	if (!so || !co) return BMH_E_ARG;
	if ((rc = c2r_check(ctx, l_pac, n_reads, reads, min_seed_len, regs, "bmh_seed_chain_regs_batch", c2r_post_of(ctx)))) return rc;
	if ((rc = fused_check_opts(ctx, so, co, "bmh_seed_chain_regs_batch"))) return rc;
	bmh_driver_stats_t st{}; // (pool_bytes stays 0: the reads are where seeding uploaded them)
	ctx->dstats = st;
	int lmax = 1;
	for (int r = 0; r < n_reads; ++r) lmax = std::max(lmax, reads[r].l_seq);
	FusedArgs u{co, l_pac, lmax, min_seed_len, &st, c2r_post_of(ctx), kTailVectors, regs};
	rc = seed_tables_device(ctx, so, co->max_occ, n_reads, reads, fused_cb, &u);
	if (!rc && n_reads == 0) c2r_empty(ctx);
	ctx->dstats = st;
	return rc;
}

} // extern "C"

// ---- bmh_reads_sam_device's phase 1 (api.hip): bmh_seed_chain_regs_batch with its own post-processing and the regions left resident

// a session's switches: the de-duplication at o->mask_level_redun, drop-exact with MEM_F_NO_EXACT, the words under *o where wanted
static C2rPost session_post(const bmh_sam_opt_t *o, bool collect)
{
	return C2rPost{true, o->mask_level_redun, (o->flag & BMH_MEM_F_NO_EXACT) != 0, collect, *o};
}

int bmh::reads_regs_check(bmh_ctx *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                          int min_seed_len, const char *who)
{
	int rc;
	if (!so || !co) return BMH_E_ARG;
	const C2rPost post{true, 0.f, false, false, {}}; // (the context's switches are not this call's)
	if ((rc = c2r_check(ctx, l_pac, n_reads, reads, min_seed_len, nullptr, who, post, false)) || (rc = fused_check_opts(ctx, so, co, who))) return rc;
	if (!ctx->bwt_bind) { // what seeding refuses before its upload
		ctx->last_error = "no FM-index on the device (bmh_ctx_set_bwt)";
		return BMH_E_ARG;
	}
	for (int r = 0; r < n_reads; ++r)
		if (reads[r].l_seq < 0 || (reads[r].l_seq > 0 && !reads[r].seq)) return BMH_E_ARG;
	return BMH_OK;
}

int bmh::reads_regs_resident(bmh_ctx *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                             int min_seed_len, const bmh_sam_opt_t *o, ResidentRegs *out)
{
	bmh_driver_stats_t st{};
	ctx->dstats = st;
	int lmax = 1;
	for (int r = 0; r < n_reads; ++r) lmax = std::max(lmax, reads[r].l_seq);
	FusedArgs u{co, l_pac, lmax, min_seed_len, &st, session_post(o, false), kTailPlan, nullptr, o, out};
	const int rc = seed_tables_device(ctx, so, co->max_occ, n_reads, reads, fused_cb, &u);
	ctx->dstats = st;
	return rc;
}

int bmh::pairs_regs_resident(bmh_ctx *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                             int min_seed_len, const bmh_sam_opt_t *o, bool collect, PairsPhase1 *out)
{
	bmh_driver_stats_t st{};
	ctx->dstats = st;
	int lmax = 1;
	size_t bytes = 0;
	for (int r = 0; r < n_reads; ++r) lmax = std::max(lmax, reads[r].l_seq), bytes += (size_t)reads[r].l_seq;
	try {
		out->cand.assign((size_t)n_reads / 2, 0u);
	} catch (const std::bad_alloc &) {
		ctx->last_error = "chains to regions: out of host memory for the insert-size words";
		return BMH_E_NOMEM;
	}
	FusedArgs u{co, l_pac, lmax, min_seed_len, &st, session_post(o, collect), kTailPairs, nullptr, nullptr, nullptr, out, bytes};
	const int rc = seed_tables_device(ctx, so, co->max_occ, n_reads, reads, fused_cb, &u);
	ctx->dstats = st;
	return rc;
}
