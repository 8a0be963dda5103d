// chain.hip -- seeds to chains on the device (last slice): the device driver of host/chain_core.h, the
// chainer host/chain_batch.c's bmh_chain_reads runs too.  One lane per read, over the per-read seeding tables as bmh_seed_batch holds
// them on the device (smem_order_* + sa_of_intervals_kernel).
// Sizes are known before the launch: chain_size_kernel computes each read's seed bound S_r and node bound, chain_scan2 turns them into
// arena slices, chain_kernel chains every read in its slice (the core checks every write against it anyway), and the kept chains are
// compacted count -> scan -> place: no overflow, no retry.
#include <algorithm>
#include <cstring>
#include <utility>

#include "bmh_ctx.h"
#include "bmh_device.h"
#include "../host/chain_core.h"

namespace bmh {

struct ChainIn { // the per-read seeding tables on the device (bmh_seed_batch's output form)
	int n_reads;
	const int *len;
	bmh_cc_tables_t t;
};

// Per read: the seed bound S_r (positions of its long and rare intervals) and the node bound.  Inconsistent offsets raise the flag.
__global__ void chain_size_kernel(bmh_chain_opt_t o, ChainIn in, unsigned long long *__restrict__ seeds, unsigned long long *__restrict__ nodes,
                                  int *__restrict__ err)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= in.n_reads) return;
	unsigned long long s;
	if (bmh_cc_seed_bound(&o, &in.t, r, in.len[r], &s)) atomicOr(err, 1);
	seeds[r] = s, nodes[r] = bmh_cc_node_bound(s);
}

// exclusive sums of two count arrays, n + 1 outputs each (the last one is the total); one block of 1024 threads
__global__ __launch_bounds__(1024) void chain_scan2(const unsigned long long *__restrict__ a, const unsigned long long *__restrict__ b, int n,
                                                    unsigned long long *__restrict__ pa, unsigned long long *__restrict__ pb)
{
	__shared__ unsigned long long sa[1024], sb[1024];
	const int t = threadIdx.x, per = (n + 1023) / 1024, lo = min(t * per, n), hi = min(lo + per, n);
	unsigned long long xa = 0, xb = 0;
	for (int k = lo; k < hi; ++k) xa += a[k], xb += b[k];
	sa[t] = xa, sb[t] = xb;
	__syncthreads();
	for (int d = 1; d < 1024; d <<= 1) {
		const unsigned long long ya = t >= d ? sa[t - d] : 0, yb = t >= d ? sb[t - d] : 0;
		__syncthreads();
		sa[t] += ya, sb[t] += yb;
		__syncthreads();
	}
	unsigned long long ca = sa[t] - xa, cb = sb[t] - xb;
	for (int k = lo; k < hi; ++k) {
		pa[k] = ca, pb[k] = cb;
		ca += a[k], cb += b[k];
	}
	if (t == 1023) pa[n] = sa[1023], pb[n] = sb[1023];
}

struct ChainWs { // arena and outputs
	bmh_seed_t *seed;
	int32_t *next;
	bmh_cc_chn_t *chn;
	bmh_cc_flt_t *flt;
	bmh_cc_pair_t *ord;
	bmh_cc_node_t *node;
	bmh_cc_pair_t *walk;
	bmh_sort_stk_t *sstk;
	const unsigned long long *seed_base, *node_base; // exclusive sums of the per-read bounds
	unsigned long long seed_cap, node_cap;          // slots allocated
	unsigned long long *n_chn, *n_seed;              // out per read: chains and seeds after the filter
	uint32_t *n_keys;                                // out per read: chains before it
	int *err;
	unsigned long long *n_equal; // look-ups that met an equal key, summed over the batch
};

// One lane per read: bmh_cc_chain_read in the read's arena slice.  The kept chains stay there, best first; chain_place_kernel gathers them.
__global__ __launch_bounds__(64) void chain_kernel(bmh_chain_opt_t o, int64_t l_pac, ChainIn in, ChainWs ws)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= in.n_reads) return;
	ws.n_chn[r] = 0, ws.n_seed[r] = 0, ws.n_keys[r] = 0;
	const unsigned long long s0 = ws.seed_base[r], n0 = ws.node_base[r];
	if (ws.seed_base[r + 1] > ws.seed_cap || ws.node_base[r + 1] > ws.node_cap) { atomicOr(ws.err, 1); return; }
	const bmh_cc_arena_t A{ws.seed + s0, ws.next + s0, ws.chn + s0, ws.flt + s0, ws.ord + s0, ws.node + n0, ws.walk + (size_t)r * BMH_CC_STK,
	                       ws.sstk + (size_t)r * BMH_CC_STK, ws.seed_base[r + 1] - s0, ws.node_base[r + 1] - n0};
	bmh_cc_counts_t cnt;
	if (bmh_cc_chain_read(&o, l_pac, &in.t, r, in.len[r], &A, &cnt)) { atomicOr(ws.err, 1); return; }
	if (cnt.n_equal) atomicAdd(ws.n_equal, (unsigned long long)cnt.n_equal);
	ws.n_chn[r] = cnt.kept, ws.n_seed[r] = cnt.seeds, ws.n_keys[r] = cnt.n_keys;
}

// count -> scan -> place: one lane per read copies its surviving chains (seed counts) and their seeds, in chain order, to the compact
// output.  coff / soff: exclusive sums of n_chn / n_seed.
__global__ void chain_place_kernel(int n_reads, ChainWs ws, const unsigned long long *__restrict__ coff, const unsigned long long *__restrict__ soff,
                                   uint32_t *__restrict__ out_n, bmh_seed_t *__restrict__ out_seed, unsigned long long out_chn_cap,
                                   unsigned long long out_seed_cap)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads) return;
	const unsigned long long nc = ws.n_chn[r];
	if (!nc) return;
	if (coff[r + 1] > out_chn_cap || soff[r + 1] > out_seed_cap) { atomicOr(ws.err, 1); return; }
	const unsigned long long s0 = ws.seed_base[r];
	bmh_cc_arena_t A{};
	A.seed = ws.seed + s0, A.next = ws.next + s0, A.chn = ws.chn + s0, A.ord = ws.ord + s0;
	bmh_cc_gather(&A, (uint32_t)nc, out_n + coff[r], out_seed + soff[r]);
}

} // namespace bmh

using namespace bmh;

namespace {

// device tables -> compact chains on the device (what every entry point starts with): sizes, arena, chain_kernel, count -> scan -> place,
// then the error flag and the totals.  The chain statistics are the caller's to set, once its call has succeeded.
// seed_bound: the batch's sum of the per-read seed bounds (positions of the long and rare intervals) -- the arena's size
int chain_compact(bmh_ctx *ctx, const bmh_chain_opt_t *o, int64_t l_pac, const ChainIn &in, uint64_t seed_bound, DevChains *out)
{
	const int n = in.n_reads;
	const unsigned long long seed_cap = std::max<unsigned long long>(seed_bound, 1);
	const unsigned long long node_cap = seed_cap / 7 + 2 * (unsigned long long)n + 2;
	const size_t nr1 = (size_t)n + 1;
	auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
	// layout of d_chain: header (error flag) | per-read counts and sums | arena | compact output
	size_t o_ = 256;
	const size_t o_sb = o_; o_ += al(nr1 * 8);           // seed bound per read
	const size_t o_nb = o_; o_ += al(nr1 * 8);           // node bound per read
	const size_t o_sbase = o_; o_ += al(nr1 * 8);        // ... their exclusive sums
	const size_t o_nbase = o_; o_ += al(nr1 * 8);
	const size_t o_nchn = o_; o_ += al(nr1 * 8);         // out: chains / seeds after the filter, chains before
	const size_t o_nseed = o_; o_ += al(nr1 * 8);
	const size_t o_nkeys = o_; o_ += al(nr1 * 4);
	const size_t o_coff = o_; o_ += al(nr1 * 8);         // ... the sums of the first two
	const size_t o_soff = o_; o_ += al(nr1 * 8);
	const size_t o_seed = o_; o_ += al(seed_cap * sizeof(bmh_seed_t));
	const size_t o_next = o_; o_ += al(seed_cap * 4);
	const size_t o_chn = o_; o_ += al(seed_cap * sizeof(bmh_cc_chn_t));
	const size_t o_flt = o_; o_ += al(seed_cap * sizeof(bmh_cc_flt_t));
	const size_t o_ord = o_; o_ += al(seed_cap * sizeof(bmh_cc_pair_t));
	const size_t o_node = o_; o_ += al(node_cap * sizeof(bmh_cc_node_t));
	const size_t o_walk = o_; o_ += al((size_t)n * BMH_CC_STK * sizeof(bmh_cc_pair_t));
	const size_t o_sstk = o_; o_ += al((size_t)n * BMH_CC_STK * sizeof(bmh_sort_stk_t));
	const size_t o_outn = o_; o_ += al(seed_cap * 4);
	const size_t o_outs = o_; o_ += al(seed_cap * sizeof(bmh_seed_t));
	int rc;
	if ((rc = ensure(ctx, ctx->d_chain, o_))) return rc;
	uint8_t *d = (uint8_t *)ctx->d_chain.p;
	int *d_err = (int *)d;
	BMH_HIP(ctx, hipMemsetAsync(d, 0, 256, ctx->stream)); // the error flag starts clean on every call
	const unsigned rb = (unsigned)((n + 63) / 64);
	hipLaunchKernelGGL(chain_size_kernel, dim3(rb), dim3(64), 0, ctx->stream, *o, in, (unsigned long long *)(d + o_sb), (unsigned long long *)(d + o_nb), d_err);
	hipLaunchKernelGGL(chain_scan2, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long *)(d + o_sb), (const unsigned long long *)(d + o_nb), n,
	                   (unsigned long long *)(d + o_sbase), (unsigned long long *)(d + o_nbase));
	BMH_HIP(ctx, hipGetLastError());
	ChainWs ws{(bmh_seed_t *)(d + o_seed), (int32_t *)(d + o_next), (bmh_cc_chn_t *)(d + o_chn), (bmh_cc_flt_t *)(d + o_flt), (bmh_cc_pair_t *)(d + o_ord),
	           (bmh_cc_node_t *)(d + o_node), (bmh_cc_pair_t *)(d + o_walk), (bmh_sort_stk_t *)(d + o_sstk), (const unsigned long long *)(d + o_sbase), (const unsigned long long *)(d + o_nbase),
	           seed_cap, node_cap, (unsigned long long *)(d + o_nchn), (unsigned long long *)(d + o_nseed), (uint32_t *)(d + o_nkeys), d_err,
	           (unsigned long long *)(d + 8)};
	if (ctx->timing) {
		if (!ctx->ev_chain[0]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_chain[0]));
		if (!ctx->ev_chain[1]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_chain[1]));
		BMH_HIP(ctx, hipEventRecord(ctx->ev_chain[0], ctx->stream));
	}
	hipLaunchKernelGGL(chain_kernel, dim3(rb), dim3(64), 0, ctx->stream, *o, l_pac, in, ws);
	BMH_HIP(ctx, hipGetLastError());
	if (ctx->timing) BMH_HIP(ctx, hipEventRecord(ctx->ev_chain[1], ctx->stream));
	hipLaunchKernelGGL(chain_scan2, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long *)(d + o_nchn), (const unsigned long long *)(d + o_nseed), n,
	                   (unsigned long long *)(d + o_coff), (unsigned long long *)(d + o_soff));
	hipLaunchKernelGGL(chain_place_kernel, dim3(rb), dim3(64), 0, ctx->stream, n, ws, (const unsigned long long *)(d + o_coff),
	                   (const unsigned long long *)(d + o_soff), (uint32_t *)(d + o_outn), (bmh_seed_t *)(d + o_outs), seed_cap, seed_cap);
	BMH_HIP(ctx, hipGetLastError());
	// the flag, the equal-key count and the two totals, then everything else at its size
	if ((rc = ensure_host(ctx, ctx->h_down, 64))) return rc;
	uint8_t *h = (uint8_t *)ctx->h_down.p;
	BMH_HIP(ctx, hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, hipMemcpyAsync(h + 16, d + o_coff + (size_t)n * 8, 8, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, hipMemcpyAsync(h + 24, d + o_soff + (size_t)n * 8, 8, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	int err;
	unsigned long long tc, ts, n_equal;
	memcpy(&err, h, 4), memcpy(&n_equal, h + 8, 8), memcpy(&tc, h + 16, 8), memcpy(&ts, h + 24, 8);
	if (err) {
		ctx->last_error = "chaining: the seeding tables are inconsistent (call list out of smem_next2's order, or an interval without its positions)";
		return BMH_E_ARG;
	}
	*out = DevChains{n, (const unsigned long long *)(d + o_coff), (const unsigned long long *)(d + o_soff), (const uint32_t *)(d + o_outn),
	                 (const bmh_seed_t *)(d + o_outs), (const uint32_t *)(d + o_nkeys), tc, ts, n_equal, -1.f};
	if (ctx->timing) BMH_HIP(ctx, hipEventElapsedTime(&out->kernel_ms, ctx->ev_chain[0], ctx->ev_chain[1]));
	return BMH_OK;
}

// device tables -> chains on the host (the rest of bmh_chain_batch and bmh_seed_chain_batch)
int chain_device(bmh_ctx *ctx, const bmh_chain_opt_t *o, int64_t l_pac, const ChainIn &in, uint64_t seed_bound, bmh_chain_v *chains)
{
	const int n = in.n_reads;
	const size_t nr1 = (size_t)n + 1;
	auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
	DevChains dc;
	int rc;
	if ((rc = chain_compact(ctx, o, l_pac, in, seed_bound, &dc))) return rc;
	const unsigned long long tc = dc.tc, ts = dc.ts;
	const size_t b_off = al(nr1 * 8), b_keys = al(nr1 * 4), b_n = al(tc * 4), b_s = tc ? ts * sizeof(bmh_seed_t) : 0;
	if ((rc = ensure_host(ctx, ctx->h_down, 2 * b_off + b_keys + b_n + b_s + 64))) return rc;
	uint8_t *h = (uint8_t *)ctx->h_down.p;
	BMH_HIP(ctx, hipMemcpyAsync(h, dc.coff, nr1 * 8, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, hipMemcpyAsync(h + b_off, dc.soff, nr1 * 8, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, hipMemcpyAsync(h + 2 * b_off, dc.n_keys, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	if (tc) BMH_HIP(ctx, hipMemcpyAsync(h + 2 * b_off + b_keys, dc.cn, tc * 4, hipMemcpyDeviceToHost, ctx->stream));
	if (b_s) BMH_HIP(ctx, hipMemcpyAsync(h + 2 * b_off + b_keys + b_n, dc.seeds, b_s, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	const unsigned long long *coff = (const unsigned long long *)h, *soff = (const unsigned long long *)(h + b_off);
	const uint32_t *nkeys = (const uint32_t *)(h + 2 * b_off), *cn = (const uint32_t *)(h + 2 * b_off + b_keys);
	const bmh_seed_t *sd = (const bmh_seed_t *)(h + 2 * b_off + b_keys + b_n);
	long long before = 0;
	for (int r = 0; r < n; ++r) {
		before += nkeys[r];
		if (bmh_cc_emit(nkeys[r], (uint32_t)(coff[r + 1] - coff[r]), cn + coff[r], sd + soff[r], &chains[r])) {
			bmh_cc_release(n, chains);
			ctx->last_error = "chaining: out of host memory for the chains";
			return BMH_E_NOMEM;
		}
	}
	ctx->cstats.reads = n, ctx->cstats.chains_in = before, ctx->cstats.chains_out = (int64_t)tc, ctx->cstats.seeds = (int64_t)ts;
	ctx->cstats.equal_keys = (int64_t)dc.n_equal;
	ctx->cstats.kernel_ms = dc.kernel_ms;
	return BMH_OK;
}

ChainIn chain_in_of(const DevSeedTables &t)
{
	return ChainIn{t.n_reads, t.len, {t.coff, t.calls, t.ioff, t.intv, t.sa_off, t.sa_pos, t.n_calls, t.n_intv, t.n_pos}};
}

int seed_chain_cb(bmh_ctx *ctx, const DevSeedTables &t, void *user)
{
	const auto *u = (const std::pair<const bmh_chain_opt_t *, std::pair<int64_t, bmh_chain_v *>> *)user;
	return chain_device(ctx, u->first, u->second.first, chain_in_of(t), t.n_pos, u->second.second); // (sa_of_intervals_kernel used the same two filters)
}

bool chain_opt_ok(const bmh_chain_opt_t *o) { return o && o->min_seed_len >= 0 && o->max_occ >= 0; }

} // namespace

// the fused seeding -> chaining -> regions call (chain2reg.hip) stops here: the compact chains stay in ctx->d_chain
int bmh::chain_compact_device(bmh_ctx *ctx, const bmh_chain_opt_t *o, int64_t l_pac, const DevSeedTables &t, DevChains *out)
{
	if (!chain_opt_ok(o)) return BMH_E_ARG;
	return chain_compact(ctx, o, l_pac, chain_in_of(t), t.n_pos, out);
}

extern "C" {

int bmh_chain_batch(bmh_ctx_t *ctx, const bmh_chain_opt_t *o, int64_t l_pac, int n_reads, const bmh_read_t *reads, const uint32_t *call_off,
                    const bmh_smem_call_t *calls, const uint64_t *intv_off, const bmh_smem_intv_t *intv, const uint64_t *sa_off,
                    const uint64_t *sa_pos, uint64_t n_pos, bmh_chain_v *chains)
{
	if (!ctx || !chain_opt_ok(o) || n_reads < 0 || l_pac < 0 ||
	    (n_reads > 0 && (!reads || !call_off || !intv_off || !chains || (call_off[n_reads] && !calls) || (intv_off[n_reads] && (!intv || !sa_off)) ||
	                     (n_pos && !sa_pos))))
		return BMH_E_ARG;
	for (int r = 0; r < n_reads; ++r) chains[r].n = chains[r].m = 0, chains[r].a = nullptr;
	if (n_reads == 0) return BMH_OK;
	const uint64_t n_calls = call_off[n_reads], n_intv = intv_off[n_reads];
	for (int r = 0; r < n_reads; ++r)
		if (reads[r].l_seq < 0 || call_off[r] > call_off[r + 1] || intv_off[r] > intv_off[r + 1]) return BMH_E_ARG;
	const uint64_t n_seed = bmh_chain_sa_keys(o, n_intv, intv, nullptr, nullptr); // the seed bound of the batch (what the size kernel sums per read)
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	int rc;
	// upload: lengths | call offsets | calls | interval offsets | intervals | sa_off | sa_pos, one pinned image, one copy
	auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
	const size_t nr1 = (size_t)n_reads + 1;
	const size_t o_len = 0, o_coff = al(nr1 * 4), o_calls = o_coff + al(nr1 * 4), o_ioff = o_calls + al(n_calls * sizeof(bmh_smem_call_t)),
	             o_intv = o_ioff + al(nr1 * 8), o_so = o_intv + al(n_intv * sizeof(bmh_smem_intv_t)), o_pos = o_so + al(n_intv * 8),
	             total = o_pos + al(n_pos * 8) + 256;
	if ((rc = ensure_host(ctx, ctx->h_up, total)) || (rc = ensure(ctx, ctx->d_scratch, total))) return rc;
	uint8_t *h = (uint8_t *)ctx->h_up.p;
	for (int r = 0; r < n_reads; ++r) ((int *)(h + o_len))[r] = reads[r].l_seq;
	memcpy(h + o_coff, call_off, nr1 * 4);
	if (n_calls) memcpy(h + o_calls, calls, n_calls * sizeof(bmh_smem_call_t));
	memcpy(h + o_ioff, intv_off, nr1 * 8);
	if (n_intv) memcpy(h + o_intv, intv, n_intv * sizeof(bmh_smem_intv_t)), memcpy(h + o_so, sa_off, n_intv * 8);
	if (n_pos) memcpy(h + o_pos, sa_pos, n_pos * 8);
	uint8_t *d = (uint8_t *)ctx->d_scratch.p;
	BMH_HIP(ctx, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, ctx->stream));
	ChainIn in{n_reads, (const int *)(d + o_len), {(const uint32_t *)(d + o_coff), (const bmh_smem_call_t *)(d + o_calls), (const uint64_t *)(d + o_ioff),
	           (const bmh_smem_intv_t *)(d + o_intv), (const uint64_t *)(d + o_so), (const uint64_t *)(d + o_pos), n_calls, n_intv, n_pos}};
	return chain_device(ctx, o, l_pac, in, n_seed, chains);
}

int bmh_seed_chain_batch(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                         bmh_chain_v *chains)
{
	if (!ctx || !so || !chain_opt_ok(co) || n_reads < 0 || l_pac < 0 || (n_reads > 0 && (!reads || !chains))) return BMH_E_ARG;
	if (so->min_seed_len != co->min_seed_len || so->split_len != co->split_len || so->split_width != co->split_width || so->min_emit_len < 0 ||
	    so->min_emit_len > co->min_seed_len) {
		ctx->last_error = "bmh_seed_chain_batch: min_seed_len / split_len / split_width must agree and min_emit_len <= min_seed_len";
		return BMH_E_ARG;
	}
	for (int r = 0; r < n_reads; ++r) chains[r].n = chains[r].m = 0, chains[r].a = nullptr;
	std::pair<const bmh_chain_opt_t *, std::pair<int64_t, bmh_chain_v *>> u{co, {l_pac, chains}};
	return seed_tables_device(ctx, so, co->max_occ, n_reads, reads, seed_chain_cb, &u);
}

int bmh_chain_stats(bmh_ctx_t *ctx, bmh_chain_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->cstats;
	return BMH_OK;
}

} // extern "C"
