// extend_dispatch.hip -- routes every extension task to the kernel built for its query length.
//
//   bin 0: qlen <= 32    extend_lane_kernel<32>   (64 tasks per wave, one lane per task)
//   bin 1: qlen <= 64    extend_lane_kernel<64>
//   bin 2: qlen <= 128   extend_lane_kernel<128>
//   bin 3: qlen <= 256   extend_lanex_kernel<2>   (32 tasks per wave, two lanes x 128 columns per task)
//   bin 4: qlen <= 512   extend_lanex_kernel<4>   (16 tasks per wave; only with BMH_EXT_MODE=lanex4: with the few
//                        such tasks a 150-300 bp run produces, one wave per task keeps more of the chip busy)
//   bin 5: longer or qlen == 0                     extend_lds_kernel  (one wave per task)
//   bin 6: only with bmh_ctx_set_wide_extension on: what the 16-bit kernels cannot take -- h0 + qlen*max(mat) > 32000 or
//          qlen > kLdsQcap, or every task when the gap costs fail ext_gaps_too_large -> extend_wide_kernel (int32)
//   bin 7: qlen > the launch's qmax (only a *_device call's qcap can be below a query length): no kernel; the sort writes the
//          failure record and raises BMH_E_RANGE, so that the bins qmax calls empty can be left out
// BMH_EXT_MODE=reg | grp | lds in the environment selects the one-task-per-wave register kernels, the
// four-tasks-per-wave group kernels, or the LDS kernel for bins 0-2 instead (A/B runs, profiles/); BMH_EXT_MODE=wide sends every
// task of a context with the switch on to bin 6 (A/B against the 16-bit kernels; no effect with the switch off).
//
// The bins are built ON THE DEVICE (a counting sort by bin and expected row count), and every
// extension kernel reads its bin size from device memory, so a launch needs no
// host round trip and the *_device entry point stays asynchronous on the caller's stream.
#include <algorithm>

#include "bmh_ctx.h"
#include "bmh_device.h"
#include "../host/extband_core.h"

namespace bmh {

// Counting sort of the tasks by (bin, expected row count): three tiny kernels, no host round trip.
// The lane-per-task kernels want neighbouring tasks to run for a similar number of rows.
constexpr int kSortKeys = 2048;

// (the binning rule itself -- ext_bin_of, ext_goes_wide, ext_sort_key, ext_binkey_of -- is in bmh_ctx.h: the fused per-seed record's
// kernels apply it too)
constexpr int kSortThreads = 256;
constexpr int kLanexMinTasks = 4096; // below this many 129-256 bp flanks one wave per task fills the chip better

// pass 1: per-block histogram in LDS over a contiguous chunk, flushed with one global atomic per used key
__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(const bmh_ext_task_t *__restrict__ tasks,
                                                                 const uint32_t *__restrict__ order, long long n,
                                                                 uint32_t *__restrict__ hist,
                                                                 uint16_t *__restrict__ binkey, ExtBinRule rule,
                                                                 const uint32_t *__restrict__ dn)
{
	__shared__ uint32_t lh[kSortBins * kSortKeys];
	for (int t = threadIdx.x; t < kSortBins * kSortKeys; t += kSortThreads) lh[t] = 0;
	__syncthreads();
	if (dn) n = min(n, (long long)*dn); // the list was built on the device (fused per-seed pipeline)
	const long long chunk = (n + gridDim.x - 1) / gridDim.x, lo = chunk * blockIdx.x, hi = min(lo + chunk, n);
	for (long long k = lo + threadIdx.x; k < hi; k += kSortThreads) {
		const uint32_t idx = order ? order[k] : (uint32_t)k;
		const int bk = ext_binkey_of(rule, tasks[idx].qlen, tasks[idx].tlen, tasks[idx].h0, idx);
		binkey[k] = (uint16_t)bk;
		atomicAdd(&lh[bk], 1u);
	}
	__syncthreads();
	for (int t = threadIdx.x; t < kSortBins * kSortKeys; t += kSortThreads)
		if (lh[t]) atomicAdd(&hist[t], lh[t]);
}

// the eight base codes at positions [s, s + 8) of a byte sequence (base 0 at pool[off]; with rev it runs downwards), position s in the low byte
__device__ __forceinline__ uint64_t seq_word(const uint8_t *pool, uint64_t off, int s, bool rev)
{
	uint64_t v;
	__builtin_memcpy(&v, rev ? pool + off - (uint64_t)s - 7 : pool + off + (uint64_t)s, 8);
	return rev ? __builtin_bswap64(v) : v;
}

// positions [from, from + 16) of a sequence of len >= 8 bases as two words, position from + j in byte j.  No byte outside the sequence is
// read: a window that would pass its end is moved back to end there and shifted (what lies past the end reads as 0)
__device__ __forceinline__ void seq_share(const uint8_t *pool, uint64_t off, int from, int len, bool rev, uint64_t w[2])
{
#pragma unroll
	for (int k = 0; k < 2; ++k) {
		const int at = from + 8 * k, s = min(at, len - 8), d = at - s;
		const uint64_t v = seq_word(pool, off, s, rev);
		w[k] = d < 8 ? v >> (8 * d) : 0;
	}
}

// pass 1 with the band pass (host/extband_core.h) in it, for launches whose bins 0-2 run on the lane kernels: per task
// the band its result needs, as one byte by input position (bmh_extband_byte), and bin and sort key from it -- the band's class is
// part of the key, so both must be known in the same pass.  EIGHT lanes share a task, each an eighth of the plain diagonal's pairs,
// joined in order: their loads fall into the task's few cache lines in the same instruction (one lane per task re-fetched lines 16x in
// the global path's band pass, profiles/global_band.md).  1024 threads: with the histogram's 64 KiB two blocks fill a CU's wave slots.
// marked: binkey[] holds the caller's marks (ExtBinned::band); an entry without a task gets the byte 255 and is not counted.
// narrow == 0 (the switch off, or the rows diagnostic armed): no walk, every task's own w.
constexpr int kBandThreads = 1024, kBandLanes = 8, kBandShare = 128 / kBandLanes; // (a lane kernel's query has at most 128 columns)
__global__ __launch_bounds__(kBandThreads) void ext_band_hist_kernel(const uint8_t *__restrict__ pool, const bmh_ext_task_t *__restrict__ tasks,
                                                                     const uint32_t *__restrict__ order, long long n,
                                                                     uint32_t *__restrict__ hist, uint16_t *__restrict__ binkey,
                                                                     ExtBinRule rule, const uint32_t *__restrict__ dn,
                                                                     uint8_t *__restrict__ band, DevParams P, int marked, int narrow, int bandkey)
{
	__shared__ uint32_t lh[kSortBins * kSortKeys];
	__shared__ int8_t smat[32];
	for (int t = threadIdx.x; t < kSortBins * kSortKeys; t += kBandThreads) lh[t] = 0;
	if (threadIdx.x < 25) smat[threadIdx.x] = (int8_t)mat_at(P, threadIdx.x);
	__syncthreads();
	const int amax = bmh_extband_amax(smat);
	const bool applies = narrow && bmh_extband_applies(amax, P.o_del, P.e_del, P.o_ins, P.e_ins);
	if (dn) n = min(n, (long long)*dn);
	const long long chunk = (n + gridDim.x - 1) / gridDim.x, lo = chunk * blockIdx.x, hi = min(lo + chunk, n);
	const int g = threadIdx.x & (kBandLanes - 1);
	constexpr int kPer = kBandThreads / kBandLanes;
	// The entry's mark and record are fetched one turn ahead, so that their round trip runs beside the walk of the entry before.  (The
	// record of a marked entry without a task is read as well: it lies inside the caller's array, and nothing of it is used.)
	struct Entry {
		uint4 a, b;
		uint32_t idx;
		bool has;
	};
	auto fetch = [&](long long k) {
		Entry e;
		e.has = !(marked && binkey[k] == kNoTask);
		e.idx = order ? order[k] : (uint32_t)k;
		const uint4 *tp = (const uint4 *)(tasks + e.idx);
		e.a = tp[0], e.b = tp[1];
		return e;
	};
	long long k = lo + threadIdx.x / kBandLanes; // (uniform in a group of eight)
	Entry nx = {};
	if (k < hi) nx = fetch(k);
	for (; k < hi; k += kPer) {
		const Entry cur = nx;
		if (k + kPer < hi) nx = fetch(k + kPer);
		if (!cur.has) {
			if (g == 0) band[k] = 255;
			continue;
		}
		const uint32_t idx = cur.idx;
		const uint4 ta = cur.a, tb = cur.b;
		const uint64_t q_off = (uint64_t)ta.y << 32 | ta.x, t_off = (uint64_t)ta.w << 32 | ta.z;
		const int qlen = (int)(tb.x & 0xffff), tlen = (int)(tb.x >> 16), h0 = (int)tb.y;
		const int w = (int)(int16_t)(tb.z & 0xffff);
		const int bin = ext_task_bin(rule, qlen, tlen, h0);
		int we = w;
		if (applies && bin <= 2 && qlen >= 1 && qlen <= kBandShare * kBandLanes && tlen >= qlen && w >= 1) { // (bins 0-2: qlen <= 128 and within the launch's qmax)
			const bool qrev = tb.w & BMH_F_QREV, trev = tb.w & BMH_F_TREV, tpac = tb.w & BMH_F_TPAC;
			const int per = (qlen + kBandLanes - 1) / kBandLanes;
			const int from = min(g * per, qlen), to = min(from + per, qlen);
			// A lane's share is at most kBandShare = 16 pairs: two eight-base loads per sequence, so the eight lanes fetch the task's one or
			// two cache lines per sequence once (byte loads touched them once per pair: 1.82 ms per launch against 1.46, profiles/ext_band.md).
			// Flanks of fewer than eight bases have one pair per lane, and a packed target (BMH_F_TPAC) is decoded base by base -- byte
			// loads, all unconditional (a pair past the share reads the query's last pair again and is not counted) and issued together.
			const int p0 = min(from, qlen - 1);
			uint64_t qw[2] = {0, 0}, tw[2] = {0, 0};
			if (qlen >= 8) seq_share(pool, q_off, from, qlen, qrev, qw);
			else qw[0] = pool[qrev ? q_off - (uint64_t)p0 : q_off + (uint64_t)p0];
			if (tpac) {
#pragma unroll
				for (int j = 0; j < kBandShare; ++j) tw[j >> 3] |= (uint64_t)tgt_base(pool, P, t_off, min(from + j, qlen - 1), trev, true) << (8 * (j & 7));
			} else if (qlen >= 8) seq_share(pool, t_off, from, tlen, trev, tw);
			else tw[0] = pool[trev ? t_off - (uint64_t)p0 : t_off + (uint64_t)p0];
			bmh_xb_part_t mine = {0, 0};
#pragma unroll
			for (int j = 0; j < kBandShare; ++j) {
				const int qb = (int)(qw[j >> 3] >> (8 * (j & 7)) & 255), tg = (int)(tw[j >> 3] >> (8 * (j & 7)) & 255);
				if (from + j < to) bmh_extband_pair(&mine, smat[min(tg, 4) * 5 + min(qb, 4)]);
			}
			bmh_xb_part_t acc = {0, 0};
#pragma unroll
			for (int j = 0; j < kBandLanes; ++j) { // every lane joins the eight parts in order
				const bmh_xb_part_t nx = {__shfl(mine.sum, j, kBandLanes), __shfl(mine.mn, j, kBandLanes)};
				bmh_extband_join(&acc, &nx);
			}
			we = bmh_extband_from_walk(amax, P.o_del, P.e_del, P.o_ins, P.e_ins, P.zdrop, qlen, tlen, h0, w, acc.sum, acc.mn);
		}
		if (g == 0) {
			const int byte = bmh_extband_byte(we);
			band[k] = (uint8_t)byte;
			const int bk = ext_binkey_of(rule, qlen, tlen, h0, idx, bandkey && bin <= 2 ? bmh_extband_class(byte) : -1);
			binkey[k] = (uint16_t)bk;
			atomicAdd(&lh[bk], 1u);
		}
	}
	__syncthreads();
	for (int t = threadIdx.x; t < kSortBins * kSortKeys; t += kBandThreads)
		if (lh[t]) atomicAdd(&hist[t], lh[t]);
}

// pass 2: exclusive scan of each bin's histogram (in place -> cursors) and the bin sizes; total (nullable): their sum
__global__ __launch_bounds__(1024) void sort_scan_kernel(uint32_t *__restrict__ hist, uint32_t *__restrict__ counts,
                                                         uint32_t *__restrict__ total)
{
	static_assert(kSortKeys == 2048, "two keys per thread");
	__shared__ uint32_t part[1024];
	const int t = threadIdx.x;
	uint32_t sum = 0;
	for (int b = 0; b < kSortBins; ++b) {
		const uint32_t v0 = hist[b * kSortKeys + 2 * t], v1 = hist[b * kSortKeys + 2 * t + 1];
		part[t] = v0 + v1;
		__syncthreads();
		for (int d = 1; d < 1024; d <<= 1) { // Hillis-Steele inclusive scan over the pair sums
			const uint32_t add = t >= d ? part[t - d] : 0;
			__syncthreads();
			part[t] += add;
			__syncthreads();
		}
		const uint32_t excl = part[t] - (v0 + v1);
		hist[b * kSortKeys + 2 * t] = excl;
		hist[b * kSortKeys + 2 * t + 1] = excl + v0;
		if (t == 1023) counts[b] = part[t], sum += part[t];
		__syncthreads();
	}
	if (t == 1023 && total) *total = sum;
}

// pass 3: every block re-counts its chunk, reserves one range per used key from the global cursors and
// places its tasks inside those ranges with LDS atomics.  Entries marked kNoTask (only a kernel that bins entries which may
// hold no task writes them) are neither counted nor placed
__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const uint32_t *__restrict__ order, long long n,
                                                                    uint32_t *__restrict__ cursor,
                                                                    const uint16_t *__restrict__ binkey,
                                                                    uint32_t *__restrict__ lists, long long stride,
                                                                    const uint32_t *__restrict__ dn,
                                                                    const uint8_t *__restrict__ payload,
                                                                    uint8_t *__restrict__ plists)
{
	__shared__ uint32_t lh[kSortBins * kSortKeys];
	for (int t = threadIdx.x; t < kSortBins * kSortKeys; t += kSortThreads) lh[t] = 0;
	__syncthreads();
	if (dn) n = min(n, (long long)*dn);
	const long long chunk = (n + gridDim.x - 1) / gridDim.x, lo = chunk * blockIdx.x, hi = min(lo + chunk, n);
	for (long long k = lo + threadIdx.x; k < hi; k += kSortThreads) {
		const uint32_t bk = binkey[k];
		if (bk != kNoTask) atomicAdd(&lh[bk], 1u);
	}
	__syncthreads();
	for (int t = threadIdx.x; t < kSortBins * kSortKeys; t += kSortThreads)
		if (lh[t]) lh[t] = atomicAdd(&cursor[t], lh[t]); // count -> start of this block's range
	__syncthreads();
	for (long long k = lo + threadIdx.x; k < hi; k += kSortThreads) {
		const uint32_t bk = binkey[k];
		if (bk == kNoTask) continue;
		const uint32_t pos = atomicAdd(&lh[bk], 1u);
		const size_t at = (size_t)(bk / kSortKeys) * (size_t)stride + pos;
		lists[at] = order ? order[k] : (uint32_t)k;
		if (payload) plists[at] = payload[k]; // a byte that belongs to the input position travels with it (the global dispatcher's band)
	}
}

// shared by the extension and the global dispatchers: workspace layout + the scan/scatter passes
static_assert(kSortKeys == kSortKeysHost, "keep bmh_ctx.h in sync");
int sort_tasks_begin(bmh_ctx *ctx, int64_t n, uint32_t **counts, uint32_t **lists)
{
	const size_t N = (size_t)n, hist_words = (size_t)kSortBins * kSortKeys;
	ctx->gbins_valid = false; // the counters of the last global launch go with the workspace (launch_global sets it again for its own)
	int rc = ensure(ctx, ctx->d_bins, (16 + hist_words + (N + 1) / 2 + 1 + (size_t)kSortBins * N) * 4);
	if (rc) return rc;
	*counts = (uint32_t *)ctx->d_bins.p;
	*lists = *counts + 16 + hist_words + (N + 1) / 2 + 1;
	BMH_HIP(ctx, hipMemsetAsync(*counts, 0, (16 + hist_words) * 4, ctx->stream));
	return BMH_OK;
}

int sort_tasks_finish(bmh_ctx *ctx, int64_t n, const uint32_t *d_order, unsigned blocks, const uint32_t *d_n, uint32_t *d_total,
                      const uint8_t *d_payload, uint8_t *d_plists)
{
	const size_t N = (size_t)n, hist_words = (size_t)kSortBins * kSortKeys;
	uint32_t *counts = (uint32_t *)ctx->d_bins.p, *hist = counts + 16;
	uint16_t *binkey = (uint16_t *)(hist + hist_words);
	uint32_t *lists = hist + hist_words + (N + 1) / 2 + 1;
	hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, hist, counts, d_total);
	hipLaunchKernelGGL(sort_scatter_kernel, dim3(blocks), dim3(kSortThreads), 0, ctx->stream, d_order, (long long)n, hist, binkey,
	                   lists, (long long)n, d_n, d_payload, d_plists);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

// ---- bin-size hints (bmh_ctx::BinHint): the counts of the previous launch of the same kind, if they have arrived
static void hint_poll(bmh_ctx *ctx, int kind)
{
	bmh_ctx::BinHint &h = ctx->hint[kind];
	if (h.pending && hipEventQuery(h.ev) == hipSuccess) {
		for (int b = 0; b < 8; ++b) h.cnt[b] = h.h[b];
		h.pending = false, h.valid = true;
	}
}

static int hint_post(bmh_ctx *ctx, int kind, const uint32_t *d_counts)
{
	bmh_ctx::BinHint &h = ctx->hint[kind];
	if (h.pending) return BMH_OK; // the previous copy has not landed yet; do not overwrite what it is writing
	if (!h.h) {
		if (hipHostMalloc((void **)&h.h, 64, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&h.ev, hipEventDisableTiming) != hipSuccess) {
			(void)hipGetLastError();
			return BMH_OK; // no hints then
		}
	}
	BMH_HIP(ctx, hipMemcpyAsync(h.h, d_counts, 32, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, hipEventRecord(h.ev, ctx->stream));
	h.pending = true;
	return BMH_OK;
}

// a list whose length lives on the device and that the last launch of this kind found (almost) empty -- the band-doubling
// retries of the fused per-seed pipeline, for reads that need none: no sort, no bins, ONE launch of the any-length kernel
// (one wave per task) over the list as it stands.  Correct for any count; a count that has grown shows in the next hint.
constexpr uint32_t kTinyList = 2048;
static int launch_extend_tiny(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n, bmh_ext_result_t *d_res,
                              const uint32_t *d_order, int qmax, const uint32_t *d_n, int kind)
{
	bmh_ctx::BinHint &h = ctx->hint[kind];
	int rc = launch_extend_lds(ctx, d_pool, d_tasks, n, d_res, d_order, d_n, qmax, 2 * kTinyList);
	if (rc) return rc;
	if (!h.pending && h.h) { // the list length stands in for the bin counts: it is all the next decision needs
		for (int b = 0; b < 8; ++b) h.h[b] = 0;
		BMH_HIP(ctx, hipMemcpyAsync(h.h + 5, d_n, 4, hipMemcpyDeviceToHost, ctx->stream));
		BMH_HIP(ctx, hipEventRecord(h.ev, ctx->stream));
		h.pending = true;
	}
	return BMH_OK;
}

constexpr int64_t kForkMinTasks = 131072; // batches below this run their bins on one stream (see launch_extend)

int wide_stats_begin(bmh_ctx *ctx)
{
	ctx->wide_last = ctx->wide_ext, ctx->wide_ms_sum = 0.0;
	if (ctx->wide_ext) BMH_HIP(ctx, hipMemsetAsync(ctx->d_wide_stat, 0, sizeof(unsigned long long), ctx->stream));
	return BMH_OK;
}

// ---- A dispatcher launch in two halves.  The first decides how the batch is binned and gets the bins built: extend_plan, then
// either sort_hist_kernel over the caller's tasks (launch_extend) or the caller's own make-and-bin kernel (extend_binned_begin /
// _finish), then the scan and scatter passes.  The second, extend_run_bins, runs every bin on its kernel.
struct ExtPlan {
	int wide; // bin 6 (switch on only): 1 the tasks outside the 16-bit domain, 2 every task (gap costs past 16 bits, or BMH_EXT_MODE=wide)
	int mode; // see ext_bin_of
	bool tiny; // the hint calls a device-counted batch (almost) empty: no bins, one launch of the any-length kernel
	int64_t n_eff; // tasks expected: n, or what the hint says of a device-counted list
	bool band; // the launch has a band pass: its bins 0-2 run on the lane kernels, and it is a flat batch or a big round of the fused call
};

// device_count: how many of the n entries are tasks is known on the device only, so the hinted size stands in for it
static int extend_plan(bmh_ctx *ctx, int64_t n, int kind, bool device_count, ExtPlan *pl)
{
	const bool gaps_wide = ext_gaps_too_large(ctx->params);
	ctx->ext_rows_n = 0;
	if (gaps_wide && !ctx->wide_ext) {
		ctx->last_error = "the extension kernels need o_del+e_del, o_ins+e_ins <= 65535 and e_del, e_ins <= 16383";
		return BMH_E_RANGE;
	}
	pl->wide = !ctx->wide_ext ? 0 : gaps_wide || (ctx->ext_mode_forced && ctx->force_kernel == 5) ? 2 : 1;
	hint_poll(ctx, kind);
	const bmh_ctx::BinHint &hint = ctx->hint[kind];
	int64_t est_total = 0;
	for (int b = 0; b < kExtBins; ++b) est_total += hint.valid ? hint.cnt[b] : 0;
	// (the tiny path's one LDS launch cannot take bin 6's tasks)
	pl->tiny = device_count && hint.valid && !ctx->ext_mode_forced && !pl->wide && est_total <= kTinyList;
	if (!hint.valid) est_total = n;
	// 0 lane-per-task, 1 lds, 2 reg (1 task/wave), 3 grp (4 tasks/wave).  The lane-per-task kernels are built for
	// throughput: a wave walks ~100 rows x 128 columns for its 64 tasks, about half a millisecond however small the batch.
	// A driver round of a few thousand tasks (bmh_chain2aln_batch: 8 192 reads per call) cannot fill the chip anyway and
	// wants latency: one task per wave finishes in tens of microseconds (8 153 tasks: 0.76 -> 0.26 ms per call, 32 647:
	// 0.84 -> 0.51 ms; level at 65 k).  With a device-side count the decision uses the hinted size.
	const int64_t n_eff = pl->n_eff = device_count ? std::min<int64_t>(n, est_total + (est_total >> 2) + 64) : n;
	pl->mode = ctx->ext_mode_forced ? (ctx->force_kernel == 5 ? 0 : ctx->force_kernel) : n_eff <= ctx->small_batch ? 2 : 0;
	// (the retry rounds of the fused call, kinds 2 and 4, run un-narrowed: a handful of tasks, and the retry rule has asked for 2w)
	pl->band = (pl->mode == 0 || pl->mode == 4) && !pl->tiny && pl->wide != 2 && (kind == 0 || kind == 1 || kind == 3);
	ctx->eband_n = 0;
	return BMH_OK;
}

// the band pass's workspace: n bytes by input position, then (from a multiple of 16 on) kSortBins x n bytes beside the sort's lists
static int band_workspace(bmh_ctx *ctx, int64_t n, uint8_t **band)
{
	int rc = ensure(ctx, ctx->d_eband, (1 + (size_t)kSortBins) * (size_t)n + 16);
	if (rc) return rc;
	*band = (uint8_t *)ctx->d_eband.p;
	return BMH_OK;
}
static uint8_t *band_lists(uint8_t *band, int64_t n) { return band ? band + (((size_t)n + 15) & ~(size_t)15) : nullptr; }

static void launch_band_hist(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, const uint32_t *d_order, int64_t n,
                             uint32_t *hist, uint16_t *binkey, const ExtBinRule &rule, const uint32_t *d_n, uint8_t *band, unsigned blocks,
                             bool marked)
{
	const int narrow = ctx->ext_narrow && ctx->ext_rows_cap <= 0; // (the rows diagnostic reports the rows of the reference's band)
	hipLaunchKernelGGL(ext_band_hist_kernel, dim3(blocks), dim3(kBandThreads), 0, ctx->stream, d_pool, d_tasks, d_order, (long long)n, hist,
	                   binkey, rule, d_n, band, ctx->dev, marked ? 1 : 0, narrow, ctx->ext_bandkey);
	ctx->eband_n = n;
}

static unsigned sort_blocks_for(int64_t n)
{
	const int64_t cg = (n + 1023) / 1024;
	return (unsigned)std::min<int64_t>(std::max<int64_t>(cg, 1), kSortBlocks);
}

static int extend_run_bins(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n, bmh_ext_result_t *d_res,
                           int qmax, int kind, const ExtPlan &pl, const uint8_t *blists);

int launch_extend(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n,
                  bmh_ext_result_t *d_res, const uint32_t *d_order, int qmax, const uint32_t *d_n, int kind)
{
	if (n <= 0) return BMH_OK;
	if (kind < 0 || kind >= bmh_ctx::kHintKinds) kind = 0;
	int rc;
	if (kind == 0 && (rc = wide_stats_begin(ctx))) return rc; // (the fused per-seed call begins its span itself)
	ExtPlan pl;
	if ((rc = extend_plan(ctx, n, kind, d_n != nullptr, &pl))) return rc;
	if (pl.tiny) return launch_extend_tiny(ctx, d_pool, d_tasks, n, d_res, d_order, qmax, d_n, kind);
	uint32_t *counts, *lists;
	if ((rc = sort_tasks_begin(ctx, n, &counts, &lists))) return rc;
	uint32_t *hist = counts + 16;
	uint16_t *binkey = (uint16_t *)(hist + (size_t)kSortBins * kSortKeys);
	const unsigned cg = sort_blocks_for(pl.n_eff);
	const ExtBinRule rule = {pl.mode, pl.wide, ctx->dev.max_mat, qmax, d_res, ctx->d_err};
	uint8_t *band = nullptr;
	if (pl.band) {
		if ((rc = band_workspace(ctx, n, &band))) return rc;
		launch_band_hist(ctx, d_pool, d_tasks, d_order, n, hist, binkey, rule, d_n, band, cg, false);
	} else
		hipLaunchKernelGGL(sort_hist_kernel, dim3(cg), dim3(kSortThreads), 0, ctx->stream, d_tasks, d_order, (long long)n, hist, binkey,
		                   rule, d_n);
	if ((rc = sort_tasks_finish(ctx, n, d_order, cg, d_n, nullptr, band, band_lists(band, n)))) return rc;
	return extend_run_bins(ctx, d_pool, d_tasks, n, d_res, qmax, kind, pl, band_lists(band, n));
}

int extend_binned_begin(bmh_ctx *ctx, int64_t n, bmh_ext_result_t *d_res, int qmax, int kind, ExtBinned *p)
{
	ExtPlan pl;
	int rc = extend_plan(ctx, n, kind, true, &pl);
	if (rc) return rc;
	uint32_t *counts, *lists;
	if ((rc = sort_tasks_begin(ctx, n, &counts, &lists))) return rc;
	// a batch the hint calls (almost) empty: every task to bin 5, whose list the any-length kernel then walks in ONE launch
	p->tiny = pl.tiny;
	p->rule = ExtBinRule{pl.tiny ? 1 : pl.mode, pl.wide, ctx->dev.max_mat, qmax, d_res, ctx->d_err};
	p->hist = counts + 16;
	p->binkey = (uint16_t *)(p->hist + (size_t)kSortBins * kSortKeys);
	p->blocks = sort_blocks_for(n);
	p->band = nullptr;
	if (pl.band && (rc = band_workspace(ctx, n, &p->band))) return rc;
	return BMH_OK;
}

int extend_binned_finish(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n, bmh_ext_result_t *d_res,
                         int qmax, int kind, const ExtBinned &p, uint32_t *d_total)
{
	if (p.band) launch_band_hist(ctx, d_pool, d_tasks, nullptr, n, p.hist, p.binkey, p.rule, nullptr, p.band, p.blocks, true);
	int rc = sort_tasks_finish(ctx, n, nullptr, p.blocks, nullptr, d_total, p.band, band_lists(p.band, n)); // (the position in binkey[] is the task index)
	if (rc) return rc;
	if (p.tiny) {
		uint32_t *counts = (uint32_t *)ctx->d_bins.p;
		const uint32_t *lists = counts + 16 + (size_t)kSortBins * kSortKeys + ((size_t)n + 1) / 2 + 1;
		if ((rc = launch_extend_lds(ctx, d_pool, d_tasks, n, d_res, lists + (size_t)5 * (size_t)n, counts + 5, qmax, 2 * kTinyList))) return rc;
		return hint_post(ctx, kind, counts); // (all of it in bin 5: the total is what the next decision needs)
	}
	const ExtPlan pl = {p.rule.wide, p.rule.mode, false, n, p.band != nullptr};
	return extend_run_bins(ctx, d_pool, d_tasks, n, d_res, qmax, kind, pl, band_lists(p.band, n));
}

// the second half: the bins stand in ctx->d_bins (sizes, cursors, lists), enqueued on ctx->stream
// blists (nullable): the band pass's bytes beside the lists, for the lane kernels of bins 0-2; the other families keep the task's band
static int extend_run_bins(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n, bmh_ext_result_t *d_res,
                           int qmax, int kind, const ExtPlan &pl, const uint8_t *blists)
{
	int rc;
	const int wide = pl.wide, mode = pl.mode;
	const size_t N = (size_t)n;
	uint32_t *counts = (uint32_t *)ctx->d_bins.p, *hist = counts + 16;
	const uint32_t *lists = hist + (size_t)kSortBins * kSortKeys + (N + 1) / 2 + 1;
	const bmh_ctx::BinHint &hint = ctx->hint[kind];
	// expected size of bin b: the previous launch's count with a margin -- or, with no hint, the whole batch
	int64_t est[kExtBins];
	for (int b = 0; b < kExtBins; ++b) est[b] = hint.valid ? std::min<int64_t>(n, (int64_t)hint.cnt[b] + (hint.cnt[b] >> 4) + 64) : n;
	if ((rc = hint_post(ctx, kind, counts))) return rc;
	if (ctx->ext_rows_cap > 0 && kind == 0) { // the diagnostic of bmh_last_extend_rows: the lane kernels write it, everything else leaves 0xffff
		const size_t bytes = (size_t)ctx->ext_rows_cap * sizeof(uint16_t);
		if ((rc = ensure(ctx, ctx->d_ext_rows, bytes))) return rc;
		BMH_HIP(ctx, hipMemsetAsync(ctx->d_ext_rows.p, 0xff, bytes, ctx->stream));
		ctx->ext_rows_n = ctx->ext_rows_cap;
	}
	const bool tm = ctx->timing;
	if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	// Bins 0-2 (lane-per-task kernels, almost all tasks) run on the caller's stream; the few long flanks of bins 3-5
	// (few waves, each running for many rows) run BESIDE them on a second stream instead of as a serial tail.
	hipStream_t main_s = ctx->stream;
	// A small batch (the preload shim's: 33 k seeds) runs its bins one after the other on the caller's stream: the side
	// stream buys nothing there, costs 2.7 ms to create per context and one more stream to share the hardware queues with.
	const bool fork = n >= kForkMinTasks || ctx->ext_sched >= 0;
	if (fork && !ctx->aux_stream) BMH_HIP(ctx, hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
	hipStream_t side_s = fork ? ctx->aux_stream : main_s;
	if (fork) {
		BMH_HIP(ctx, hipEventRecord(ctx->ev_fork, main_s));
		BMH_HIP(ctx, hipStreamWaitEvent(side_s, ctx->ev_fork, 0));
	}
	static const int orders[5][kExtBins] = {{3, 4, 5, 0, 1, 2}, {3, 4, 5, 2, 1, 0}, {3, 4, 5, 2, 1, 0}, {3, 4, 5, 2, 1, 0}, {2, 1, 0, 3, 4, 5}};
	// 0: short bins first; 1: long bins first; 2: bins 0-1 behind the long flanks on the second stream, beside bin 2;
	// 3: bins 0-1 on a third stream of their own (A/B knob BMH_EXT_SCHED)
	// Default: long bins first.  When no query is longer than 160 (150 bp reads: bins 3-5 hold a handful of tasks) the two
	// short-query bins go behind them on the second stream and run beside the 128-column bin, whose two waves per SIMD leave
	// issue slots free: 4.61 -> 4.41 ms per 1 M reads.  With many long flanks (100-300 bp reads) that delays bins 3-4, which
	// are the critical path there (17.8 against 16.8 ms), so they keep the second stream to themselves.
	const int sched = ctx->ext_sched >= 0 ? ctx->ext_sched : !fork ? 1 : qmax <= 160 ? 2 : 1;
	const int *order = orders[sched];
	if (sched == 3) { // (an A/B knob: its stream is made when first asked for -- a stream costs 2.7 ms to create)
		if (!ctx->aux2_stream) BMH_HIP(ctx, hipStreamCreateWithFlags(&ctx->aux2_stream, hipStreamNonBlocking));
		BMH_HIP(ctx, hipStreamWaitEvent(ctx->aux2_stream, ctx->ev_fork, 0));
	}
	for (int k = 0; k < kExtBins; ++k) {
		const int b = order[k];
		ctx->stream = b >= 3 ? side_s : b < 2 && (sched == 2 || sched == 4) ? side_s : b < 2 && sched == 3 ? ctx->aux2_stream : main_s; // the launchers enqueue on ctx->stream
		if (tm) {
			rc = (int)hipEventRecord(ctx->ev_bin[b], ctx->stream);
			if (rc) { ctx->stream = main_s; return set_hip_error(ctx, (hipError_t)rc, "hipEventRecord"); }
		}
		const uint32_t *lst = lists + (size_t)b * N, *cnt = counts + b;
		const uint8_t *bnd = blists ? blists + (size_t)b * N : nullptr;
		const int qlo = b == 0 ? 0 : 16 << b; // bins 0..4 hold qlen <= 32,64,128,256,512
		// grid of the bin's kernel: sized for the expected count (every kernel strides over its bin, so any grid is
		// correct); a bin the hint calls empty still gets a few hundred waves in case the batch differs from the last one
		const int64_t eb = std::max<int64_t>(est[b], 16384);
		rc = BMH_OK;
		if (wide == 2 || (b < 5 && (mode == 1 || (qmax <= qlo && !(mode == 3 && b == 3))))) { // (mode 3 routes long targets of short queries to bin 3)
			// provably empty bin
		} else if (b <= 2) {
			if ((mode == 0 || mode == 4) && b == 2 && ctx->ext_split96) {
				// the 65-128 bin is sorted by query length first (16 buckets of 4 columns): its tasks of up to 96 columns are the head of
				// the list, and where it ends stands in the sort's cursor array -- the key range of buckets 0-7 closes at key 1023.  They go
				// to a 96-column instantiation, whose 120 state registers leave room for 3 waves per SIMD (the 128-column one: 2).
				const uint32_t *n96 = hist + (size_t)2 * kSortKeys + 1023;
				rc = launch_extend_lane(ctx, 96, d_pool, d_tasks, hint.valid ? est[b] : n, d_res, lst, n96, true, nullptr, bnd); // (no pick-up launch: see `rem` in the kernel)
				if (!rc) rc = launch_extend_lane(ctx, 128, d_pool, d_tasks, hint.valid ? est[b] : n, d_res, lst, cnt, !hint.valid, n96, bnd);
			} else if (mode == 0 || mode == 4) rc = launch_extend_lane(ctx, 32 << b, d_pool, d_tasks, hint.valid ? est[b] : n, d_res, lst, cnt, !hint.valid, nullptr, bnd);
			else if (mode == 3) rc = launch_extend_grp(ctx, 2 << b, d_pool, d_tasks, n, d_res, lst, cnt);
			else rc = launch_extend_reg(ctx, b == 2 ? 2 : 1, d_pool, d_tasks, n, d_res, lst, cnt, 0, est[b]);
		} else if (b == 3) {
			if (mode == 0 || mode == 4) {
				// the bin size (known on the device only) decides which kernel works: many 129-256 bp flanks -> two lanes per
				// task, a handful -> one wave per task.  With a hint exactly one of them is launched (either handles any count);
				// without one both are, and each looks at the count
				if (hint.valid) {
					if (hint.cnt[3] >= (uint32_t)kLanexMinTasks) rc = launch_extend_lanex(ctx, 2, d_pool, d_tasks, eb, d_res, lst, cnt, 0);
					else rc = launch_extend_reg(ctx, 4, d_pool, d_tasks, n, d_res, lst, cnt, 0, std::max<int64_t>(est[3], 1024));
				} else {
					rc = launch_extend_lanex(ctx, 2, d_pool, d_tasks, n, d_res, lst, cnt, kLanexMinTasks);
					if (!rc) rc = launch_extend_reg(ctx, 4, d_pool, d_tasks, n < kLanexMinTasks ? n : kLanexMinTasks, d_res, lst, cnt, kLanexMinTasks);
				}
			} else rc = launch_extend_reg(ctx, 4, d_pool, d_tasks, n, d_res, lst, cnt, 0, est[b]);
		} else if (b == 4 && mode == 4) rc = launch_extend_lanex(ctx, 4, d_pool, d_tasks, eb, d_res, lst, cnt, 0);
		else if (b == 5) // (with the switch on, longer queries are bin 6's: the LDS kernel is sized for what it can hold)
			rc = launch_extend_lds(ctx, d_pool, d_tasks, n, d_res, lst, cnt, wide ? std::min(qmax, kLdsQcap) : qmax,
			                       hint.valid ? std::max<int64_t>(est[5], 512) : (mode != 1 && qmax <= 256 ? 4096 : 0));
		if (!rc && tm) rc = (int)hipEventRecord(ctx->ev_bin_end[b], ctx->stream) ? BMH_E_HIP : BMH_OK;
		if (rc) { ctx->stream = main_s; return rc; }
	}
	if (wide) { // bin 6 beside the long bins; its time goes to bmh_extend_wide_stats, not to the six bins' arrays
		ctx->stream = side_s;
		rc = BMH_OK;
		if (tm) rc = (int)hipEventRecord(ctx->ev_bin[kWideBin], side_s) ? BMH_E_HIP : BMH_OK;
		const int64_t ew = hint.valid ? std::min<int64_t>(n, (int64_t)hint.cnt[kWideBin] + (hint.cnt[kWideBin] >> 4) + 64) : n;
		if (!rc) rc = launch_extend_wide(ctx, d_pool, d_tasks, n, d_res, lists + (size_t)kWideBin * N, counts + kWideBin, qmax, std::max<int64_t>(ew, 512));
		if (!rc && tm) rc = (int)hipEventRecord(ctx->ev_bin_end[kWideBin], side_s) ? BMH_E_HIP : BMH_OK;
		if (rc) { ctx->stream = main_s; return rc; }
	}
	ctx->stream = main_s;
	if (fork) {
		BMH_HIP(ctx, hipEventRecord(ctx->ev_join, side_s));
		BMH_HIP(ctx, hipStreamWaitEvent(main_s, ctx->ev_join, 0));
	}
	if (sched == 3) {
		BMH_HIP(ctx, hipEventRecord(ctx->ev_join2, ctx->aux2_stream));
		BMH_HIP(ctx, hipStreamWaitEvent(main_s, ctx->ev_join2, 0));
	}
	if (tm) {
		BMH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
		ctx->ev_valid = ctx->ev_bin_valid = true;
		// timing mode is a measurement mode: wait here and add this launch's per-bin durations to the running sums, so that a
		// caller of the fused per-seed pipeline (four dispatcher launches per call) can attribute its time to kernels
		BMH_HIP(ctx, hipEventSynchronize(ctx->ev1));
		for (int b = 0; b < kExtBins; ++b) {
			float ms = 0.f;
			if (hipEventElapsedTime(&ms, ctx->ev_bin[b], ctx->ev_bin_end[b]) == hipSuccess && ms > 0.f) ctx->ext_bin_ms_sum[b] += ms;
			else (void)hipGetLastError();
		}
		if (wide) {
			float ms = 0.f;
			if (hipEventElapsedTime(&ms, ctx->ev_bin[kWideBin], ctx->ev_bin_end[kWideBin]) == hipSuccess && ms > 0.f) ctx->wide_ms_sum += ms;
			else (void)hipGetLastError();
		}
		++ctx->ext_bin_launches;
	}
	return BMH_OK;
}

} // namespace bmh
