// region_long.hip -- the long round of bmh_region_cigar_batch_long: the regions region_finish_kernel flagged, because their final
// CIGAR or MD outgrew the fixed slots, are finished on the device, where the oriented copies already lie (d_pool is only read).
//
//   list    the flagged records, compacted in region order: count -> scan -> place, as the chains-to-regions gather does it.  The
//           place kernel replays the band loop (host/regfinish_core.h) for the index of each entry's final task.
//   tasks   a 64-bit exclusive scan of n_cigar gives every entry its words in one dense CIGAR pool; a CIGAR-cut entry gets its
//           final try's task again, with exactly n_cigar slots there, and launch_global runs these tasks (global_kernel.hip)
//   check   the rerun must give round 1's score and n_cigar (else BMH_E_ARG into the error word and the entry is left out of the
//           walk); an entry whose CIGAR fitted its slot (only the MD was cut) has it copied into the pool
//   NM/MD   region_md_kernel, one lane per entry, two instantiations over regfinish_core.h's walk: the size pass gives NM and
//           md_len; after a scan of md_len the write pass puts the bytes into one dense MD pool, without NUL, as in the slots
// Every kernel is a few bytes per base once per flagged region, as region_finish_kernel is; the alignments are the cost.
#include <hip/hip_runtime.h>

#include "bmh_ctx.h"
#include "bmh_device.h"
#include "../host/regfinish_core.h"

namespace bmh {

constexpr int kScanThreads = 256;

__device__ __forceinline__ RegionLongSum operator+(RegionLongSum x, RegionLongSum y) { return RegionLongSum{x.a + y.a, x.b + y.b}; }

// exclusive prefix of v over the block's 256 threads, and the block's total; every thread of the block calls it
__device__ __forceinline__ RegionLongSum block_excl_scan(RegionLongSum v, RegionLongSum *total)
{
	__shared__ RegionLongSum wsum[kScanThreads / 64];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	RegionLongSum inc = v;
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long a = __shfl_up(inc.a, d), b = __shfl_up(inc.b, d);
		if (lane >= d) inc.a += a, inc.b += b;
	}
	__syncthreads(); // (a second call in the same kernel: the first one's readers are done)
	if (lane == 63) wsum[wv] = inc;
	__syncthreads();
	RegionLongSum base{0, 0}, tot{0, 0};
	for (int k = 0; k < kScanThreads / 64; ++k) {
		if (k < wv) base = base + wsum[k];
		tot = tot + wsum[k];
	}
	*total = tot;
	return RegionLongSum{base.a + inc.a - v.a, base.b + inc.b - v.b};
}

// what one position adds to the scans.  LIST: over the region records, a = 1 for a flagged one.  CIGAR: over the entries, a = the
// words of its CIGAR, b = 1 if it is rerun.  MD: over the entries, a = the bytes of its MD.
enum { kSumList = 0, kSumCigar = 1, kSumMd = 2 };
template <int WHAT>
__device__ __forceinline__ RegionLongSum long_value(const bmh_region_res_t *__restrict__ res, const RegionLongEnt *__restrict__ ent, long long k,
                                                    long long n)
{
	if (k >= n) return RegionLongSum{0, 0};
	if (WHAT == kSumList) return RegionLongSum{res[k].flags != 0 ? 1ull : 0ull, 0};
	if (WHAT == kSumCigar) return RegionLongSum{(unsigned long long)ent[k].n_cigar, (ent[k].flags & BMH_REGION_CIGAR_CUT) ? 1ull : 0ull};
	return RegionLongSum{(unsigned long long)ent[k].md_len, 0};
}

template <int WHAT>
__global__ __launch_bounds__(kScanThreads) void region_long_count_kernel(const bmh_region_res_t *__restrict__ res,
                                                                         const RegionLongEnt *__restrict__ ent, long long n,
                                                                         RegionLongSum *__restrict__ bsum)
{
	RegionLongSum tot;
	(void)block_excl_scan(long_value<WHAT>(res, ent, (long long)blockIdx.x * kScanThreads + threadIdx.x, n), &tot);
	if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one block: bsum[0, nb) becomes its exclusive prefix, bsum[nb] the total
__global__ __launch_bounds__(kScanThreads) void region_long_scan_kernel(RegionLongSum *__restrict__ bsum, long long nb)
{
	RegionLongSum carry{0, 0};
	for (long long base = 0; base < nb; base += kScanThreads) { // (uniform bounds: every thread takes every round)
		const long long k = base + threadIdx.x;
		const RegionLongSum v = k < nb ? bsum[k] : RegionLongSum{0, 0};
		RegionLongSum tot;
		const RegionLongSum ex = block_excl_scan(v, &tot);
		if (k < nb) bsum[k] = carry + ex;
		carry = carry + tot;
	}
	if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(kScanThreads) void region_long_list_kernel(const bmh_region_req_t *__restrict__ reqs,
                                                                        const bmh_region_res_t *__restrict__ res, long long n,
                                                                        const bmh_glb_result_t *__restrict__ gres,
                                                                        const RegionLongSum *__restrict__ bsum, RegionLongEnt *__restrict__ ent,
                                                                        long long n_ent, int a, int *__restrict__ err_flag)
{
	const long long k = (long long)blockIdx.x * kScanThreads + threadIdx.x;
	RegionLongSum tot;
	const RegionLongSum v = long_value<kSumList>(res, nullptr, k, n);
	const unsigned long long e = bsum[blockIdx.x].a + block_excl_scan(v, &tot).a;
	if (!v.a) return;
	if (e >= (unsigned long long)n_ent) { // the host counted the same flags: cannot happen
		atomicExch(err_flag, BMH_E_ARG);
		return;
	}
	const bmh_region_req_t rq = reqs[k];
	const bmh_region_res_t r = res[k];
	RegionLongEnt x;
	x.region = k, x.cigar_off = 0, x.md_off = 0, x.fin = -1, x.tix = -1;
	x.n_cigar = r.n_cigar, x.score = r.score, x.NM = -1, x.md_len = 0, x.flags = r.flags, x.bad = 0, x.rsv_ = 0;
	if (rq.task[0] >= 0) {
		bmh_rf_replay_t rp;
		bmh_rf_replay(rq.task, rq.truesc, a, gres, &rp);
		x.fin = rp.fin;
		if (rp.score != r.score || rp.n_cigar != r.n_cigar || rp.tries != r.tries) x.bad = 1, atomicExch(err_flag, BMH_E_ARG);
	} else if (r.flags & BMH_REGION_CIGAR_CUT) x.bad = 1, atomicExch(err_flag, BMH_E_ARG); // (one match run never outgrows a slot)
	if (x.n_cigar < 1) x.n_cigar = 0, x.bad = 1, atomicExch(err_flag, BMH_E_ARG);
	ent[e] = x;
}

__global__ __launch_bounds__(kScanThreads) void region_long_task_kernel(RegionLongEnt *__restrict__ ent, long long n_ent,
                                                                        const RegionLongSum *__restrict__ bsum,
                                                                        const bmh_glb_task_t *__restrict__ tasks, bmh_glb_task_t *__restrict__ ltasks,
                                                                        long long n_cut, unsigned long long words, int *__restrict__ err_flag)
{
	const long long k = (long long)blockIdx.x * kScanThreads + threadIdx.x;
	RegionLongSum tot;
	const RegionLongSum v = long_value<kSumCigar>(nullptr, ent, k, n_ent);
	const RegionLongSum ex = block_excl_scan(v, &tot), at = bsum[blockIdx.x] + ex;
	if (k >= n_ent) return;
	if (at.a + v.a > words || (v.b && at.b >= (unsigned long long)n_cut)) { // the host summed the same records: cannot happen
		ent[k].bad = 1;
		atomicExch(err_flag, BMH_E_ARG);
		return;
	}
	ent[k].cigar_off = at.a;
	if (!v.b || ent[k].bad) return;
	ent[k].tix = (int32_t)at.b;
	bmh_glb_task_t t = tasks[ent[k].fin];
	t.cigar_off = (uint32_t)at.a, t.cigar_cap = (uint32_t)v.a;
	ltasks[at.b] = t;
}

// a one-cell, score-only task in every slot first: launch_global runs all n_cut of them, and an entry left out (bad) fills none
__global__ __launch_bounds__(kScanThreads) void region_long_fill_kernel(bmh_glb_task_t *__restrict__ ltasks, long long n_cut)
{
	const long long k = (long long)blockIdx.x * kScanThreads + threadIdx.x;
	if (k >= n_cut) return;
	bmh_glb_task_t t;
	t.q_off = 0, t.t_off = 0, t.qlen = 1, t.tlen = 1, t.w = 1, t.cigar_off = 0, t.cigar_cap = 0; // one cell, score only
	ltasks[k] = t;
}

__global__ __launch_bounds__(kScanThreads) void region_long_check_kernel(RegionLongEnt *__restrict__ ent, long long n_ent,
                                                                         const bmh_glb_result_t *__restrict__ lres,
                                                                         const uint32_t *__restrict__ cig_out, int cig_cap,
                                                                         uint32_t *__restrict__ lcig, int *__restrict__ err_flag)
{
	const long long k = (long long)blockIdx.x * kScanThreads + threadIdx.x;
	if (k >= n_ent) return;
	const RegionLongEnt x = ent[k];
	if (x.bad) return;
	if (x.flags & BMH_REGION_CIGAR_CUT) {
		const bmh_glb_result_t r = lres[x.tix];
		if (r.score != x.score || r.n_cigar != x.n_cigar) ent[k].bad = 1, atomicExch(err_flag, BMH_E_ARG);
		return;
	}
	if (x.n_cigar > cig_cap) { // (an entry that is not CIGAR-cut has its CIGAR in the slot)
		ent[k].bad = 1, atomicExch(err_flag, BMH_E_ARG);
		return;
	}
	const uint32_t *src = cig_out + (size_t)x.region * cig_cap;
	for (int i = 0; i < x.n_cigar; ++i) lcig[x.cigar_off + i] = src[i];
}

// NM and MD of the entries (bwa.c:134-164), one lane per entry.  WRITE = false: the size pass, NM and md_len into the entry.
// WRITE = true: md_off from the scan of md_len (bsum) and the bytes, through a sink of exactly md_len bytes.
template <bool WRITE>
__global__ __launch_bounds__(kScanThreads) void region_md_kernel(const uint8_t *__restrict__ pool, const bmh_region_req_t *__restrict__ reqs,
                                                                 RegionLongEnt *__restrict__ ent, long long n_ent,
                                                                 const uint32_t *__restrict__ lcig, const RegionLongSum *__restrict__ bsum,
                                                                 char *__restrict__ lmd, unsigned long long md_bytes, DevParams P,
                                                                 int *__restrict__ err_flag)
{
	const long long k = (long long)blockIdx.x * kScanThreads + threadIdx.x;
	unsigned long long md_off = 0;
	if (WRITE) {
		RegionLongSum tot;
		md_off = bsum[blockIdx.x].a + block_excl_scan(long_value<kSumMd>(nullptr, ent, k, n_ent), &tot).a;
	}
	if (k >= n_ent) return;
	const RegionLongEnt x = ent[k];
	if (x.bad) return;
	if (WRITE && md_off + (unsigned long long)x.md_len > md_bytes) { // the host read the same total: cannot happen
		atomicExch(err_flag, BMH_E_ARG);
		return;
	}
	const bmh_region_req_t rq = reqs[x.region];
	const uint8_t *q = pool + rq.o_off, *t = q + rq.ql;
	bmh_rf_sink_t md;
	md.s = WRITE ? lmd + md_off : nullptr, md.l = 0, md.cap = WRITE ? x.md_len : 0;
	const int nm = bmh_rf_nm_md(x.n_cigar, lcig + x.cigar_off, q, rq.ql, t, rq.tl, rq.rb >= P.l_pac, &md);
	if (nm < 0 || (WRITE && (nm != x.NM || md.l != x.md_len))) {
		ent[k].bad = 1, atomicExch(err_flag, BMH_E_ARG);
		if (!WRITE) ent[k].md_len = 0;
		return;
	}
	if (WRITE) ent[k].md_off = md_off;
	else ent[k].NM = nm, ent[k].md_len = (int32_t)md.l;
}

static unsigned scan_blocks(int64_t n) { return (unsigned)((n + kScanThreads - 1) / kScanThreads); }

int launch_region_long_list(bmh_ctx *ctx, const bmh_region_req_t *d_reqs, const bmh_region_res_t *d_res, int64_t n,
                            const bmh_glb_result_t *d_gres, RegionLongSum *d_bsum, RegionLongEnt *d_ent, int64_t n_ent)
{
	const unsigned nb = scan_blocks(n);
	hipLaunchKernelGGL(region_long_count_kernel<kSumList>, dim3(nb), dim3(kScanThreads), 0, ctx->stream, d_res, (const RegionLongEnt *)nullptr,
	                   (long long)n, d_bsum);
	hipLaunchKernelGGL(region_long_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, d_bsum, (long long)nb);
	hipLaunchKernelGGL(region_long_list_kernel, dim3(nb), dim3(kScanThreads), 0, ctx->stream, d_reqs, d_res, (long long)n, d_gres,
	                   (const RegionLongSum *)d_bsum, d_ent, (long long)n_ent, ctx->params.a, ctx->d_err);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

int launch_region_long_tasks(bmh_ctx *ctx, RegionLongEnt *d_ent, int64_t n_ent, RegionLongSum *d_bsum, const bmh_glb_task_t *d_tasks,
                             bmh_glb_task_t *d_ltasks, int64_t n_cut, uint64_t words)
{
	const unsigned nb = scan_blocks(n_ent);
	if (n_cut > 0) hipLaunchKernelGGL(region_long_fill_kernel, dim3(scan_blocks(n_cut)), dim3(kScanThreads), 0, ctx->stream, d_ltasks, (long long)n_cut);
	hipLaunchKernelGGL(region_long_count_kernel<kSumCigar>, dim3(nb), dim3(kScanThreads), 0, ctx->stream, (const bmh_region_res_t *)nullptr,
	                   (const RegionLongEnt *)d_ent, (long long)n_ent, d_bsum);
	hipLaunchKernelGGL(region_long_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, d_bsum, (long long)nb);
	hipLaunchKernelGGL(region_long_task_kernel, dim3(nb), dim3(kScanThreads), 0, ctx->stream, d_ent, (long long)n_ent,
	                   (const RegionLongSum *)d_bsum, d_tasks, d_ltasks, (long long)n_cut, (unsigned long long)words, ctx->d_err);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

int launch_region_long_sizes(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_region_req_t *d_reqs, RegionLongEnt *d_ent, int64_t n_ent,
                             const bmh_glb_result_t *d_lres, const uint32_t *d_cig_out, int cig_cap, uint32_t *d_lcig, RegionLongSum *d_bsum)
{
	const unsigned nb = scan_blocks(n_ent);
	hipLaunchKernelGGL(region_long_check_kernel, dim3(nb), dim3(kScanThreads), 0, ctx->stream, d_ent, (long long)n_ent, d_lres, d_cig_out,
	                   cig_cap, d_lcig, ctx->d_err);
	hipLaunchKernelGGL(region_md_kernel<false>, dim3(nb), dim3(kScanThreads), 0, ctx->stream, d_pool, d_reqs, d_ent, (long long)n_ent,
	                   (const uint32_t *)d_lcig, (const RegionLongSum *)nullptr, (char *)nullptr, 0ull, ctx->dev, ctx->d_err);
	hipLaunchKernelGGL(region_long_count_kernel<kSumMd>, dim3(nb), dim3(kScanThreads), 0, ctx->stream, (const bmh_region_res_t *)nullptr,
	                   (const RegionLongEnt *)d_ent, (long long)n_ent, d_bsum);
	hipLaunchKernelGGL(region_long_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, d_bsum, (long long)nb);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

int launch_region_long_md(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_region_req_t *d_reqs, RegionLongEnt *d_ent, int64_t n_ent,
                          const uint32_t *d_lcig, const RegionLongSum *d_bsum, char *d_lmd, uint64_t md_bytes)
{
	hipLaunchKernelGGL(region_md_kernel<true>, dim3(scan_blocks(n_ent)), dim3(kScanThreads), 0, ctx->stream, d_pool, d_reqs, d_ent,
	                   (long long)n_ent, d_lcig, d_bsum, d_lmd, (unsigned long long)md_bytes, ctx->dev, ctx->d_err);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

} // namespace bmh
