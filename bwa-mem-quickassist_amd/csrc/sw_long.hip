// sw_long.hip -- word-mode local Smith-Waterman (ksw_align2 over ksw_i16, reference bwa-0.7.8/ksw.c:231-364) with one WAVE per
// task for queries of any length up to 65 535, including scores past the 16-bit range (opt-in per context: bmh_ctx_set_wide_sw).
//
// The row is sw_wave.hip's: with a(j) = max(min(H(i-1,j-1) + S, 32767), E(i,j)) and w(j) = a(j) - o_ins - e_ins +
// e_ins*j, F is an exclusive max-plus prefix scan of w -- Ffull over the whole padded row (the lazy-F pass), Fseg restricted to the
// column's own segment [k*slen, (k+1)*slen) (the main loop's f) -- and Hpre = max(a, Fseg), H = max(Hpre, Ffull),
// E' = max(0, E - e_del, Hpre - o_del - e_del).  The clamp at 32 767 is ksw_i16's _mm_adds_epi16 (ksw.c:263), the only place its
// 16-bit lanes change a result: every other value stays in [0, 32767] (tests/swsatlib.py states this and
// tests/test_wide_sw_cpu.py pins it to the reference).  What is new against sw_wave is the length: the padded query is walked in
// chunks of 512 columns, lane l owning columns [512c + 8l, 512c + 8l + 8) of chunk c, and three wave-uniform carries cross the
// chunks -- H(i-1, last column of the chunk) for the diagonal, and the running maxima of both scans.  The segmented scan adds
// seg(j) * 2^25 to w, which puts every entry of an earlier segment below anything of the current one and below zero once the
// column's own offset is taken off, so the carry needs no reset at a segment boundary.
//
// State per padded column: H and E as two u16 halves of one u32, and one byte holding the query code (0-4, 5 = pad column, 6 = past
// the padded query) and the segment index (bits 3-5).  Substitution scores come from the row's target base through an 8-byte table
// in LDS (no per-task profile).  Two variants: SLAB = false keeps the state in LDS for padded queries up to kSwLongLdsCols columns,
// SLAB = true in a per-block slice of an HBM slab for the rest.  Every lane reads and writes only its own columns, so neither needs
// a barrier inside a row.  Row maxima for the second-best score go to a per-block u16 slab of the batch's longest target.
#include <algorithm>

#include "bmh_ctx.h"
#include "bmh_device.h"
#include "sw_common.h"

namespace bmh {

constexpr int kSwLongCpl = 8;                    // columns per lane
constexpr int kSwLongChunk = 64 * kSwLongCpl;    // columns per chunk
constexpr int kSwLongSegBig = 1 << 25;           // > 32767 + 255 * 65536 + 510: the span of w inside one segment
constexpr long long kSwLongSlabBudget = 1LL << 30;
static_assert(7LL * kSwLongSegBig + 32767 + 255LL * 65536 < 0x7fffffffLL, "segmented scan terms stay inside int32");
static_assert(kSwLongLdsCols % kSwLongChunk == 0, "the LDS cutoff is a whole number of chunks");
static_assert((sw_long_state_bytes(kSwLongLdsCols) + 64) * 7 <= 160 * 1024, "seven LDS-variant waves at the cutoff fit one CU");

struct SwLongSeq {
	const uint8_t *pool;
	uint64_t q_off, t_off;
	bool qrev, qcomp, trev, tpac;
	int qfold, tfold; // second pass: query base k = q(qfold-k); target row r = r <= tfold ? t(tfold-r) : t(r)
};

__device__ __forceinline__ int swl_qbase(const SwLongSeq &s, int k)
{
	const int kk = s.qfold >= 0 ? s.qfold - k : k;
	int c = seq_base(s.pool, s.q_off, kk, s.qrev);
	c = c > 4 ? 4 : c;
	return s.qcomp && c < 4 ? 3 - c : c;
}

__device__ __forceinline__ int swl_tbase(const SwLongSeq &s, const DevParams &P, int r)
{
	const int rr = r <= s.tfold ? s.tfold - r : r;
	const int c = tgt_base(s.pool, P, s.t_off, rr, s.trev, s.tpac);
	return c > 4 ? 4 : c;
}

// one pass of ksw_i16 by the whole wave over state he[cols] (u32: H | E << 16) and qc[cols] (code | seg << 3); every lane returns
// the same SwCore.  rm: the block's row-maximum slab (pass 1 with KSW_XSUBO), or null.
__device__ SwCore sw_long_pass(const SwLongSeq &seq, const DevParams &P, const uint2 *srow, int qlen, int tlen, int minsc, int endsc,
                               uint32_t *he, uint8_t *qc, uint16_t *rm)
{
	const int lane = threadIdx.x & 63;
	const int slen = (qlen + 7) >> 3, Q = slen * 8, nch = (Q + kSwLongChunk - 1) / kSwLongChunk;
	const int e_del = P.e_del, oe_del = P.o_del + P.e_del, e_ins = P.e_ins, o_ins = P.o_ins, g_ins = P.o_ins + P.e_ins;
	for (int j0 = lane * kSwLongCpl; j0 < nch * kSwLongChunk; j0 += kSwLongChunk) {
		uint32_t lo = 0, hi = 0;
#pragma unroll
		for (int c = 0; c < kSwLongCpl; ++c) {
			const int j = j0 + c;
			const uint32_t code = j < qlen ? (uint32_t)swl_qbase(seq, j) : j < Q ? 5u : 6u;
			const uint32_t b = code | (uint32_t)(j < Q ? j / slen : 0) << 3;
			if (c < 4) lo |= b << (8 * c);
			else hi |= b << (8 * (c - 4));
		}
		*(uint2 *)(qc + j0) = make_uint2(lo, hi);
		uint4 *h = (uint4 *)(he + j0);
		h[0] = make_uint4(0, 0, 0, 0), h[1] = make_uint4(0, 0, 0, 0);
	}
	SwCore r;
	r.score = 0, r.te = -1, r.qe = -1, r.score2 = -1, r.te2 = -1;
	int gmax = 0, te = -1, qe = -1, nrows = 0, tc = 4;
	constexpr int NEG = INT32_MIN / 2;
	for (int i = 0; i < tlen && slen > 0; ++i) {
		if ((i & 63) == 0) tc = i + lane < tlen ? swl_tbase(seq, P, i + lane) : 4; // the next 64 target bases, one per lane
		const uint2 sr = srow[__builtin_amdgcn_readlane(tc, i & 63)];
		int hcarry = 0, fcarry = NEG, scarry = NEG; // H(i-1, chunk start - 1) and the scans' maxima of the chunks to the left
		uint32_t key = 0;
		for (int ch = 0; ch < nch; ++ch) {
			const int j0 = ch * kSwLongChunk + lane * kSwLongCpl;
			uint4 *hp = (uint4 *)(he + j0);
			const uint4 x0 = hp[0], x1 = hp[1];
			const uint2 qq = *(const uint2 *)(qc + j0);
			const uint32_t x[kSwLongCpl] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
			const int hlast = (int)(x[kSwLongCpl - 1] & 0xffff);
			const int hleft = wave_shr1(hlast, hcarry); // H(i-1, j0-1)
			hcarry = __builtin_amdgcn_readlane(hlast, 63);
			int a[kSwLongCpl], pre[kSwLongCpl], spre[kSwLongCpl], fs[kSwLongCpl], sf[kSwLongCpl];
			int loc = NEG, sloc = NEG;
			const int wadd0 = e_ins * j0 - g_ins;
#pragma unroll
			for (int c = 0; c < kSwLongCpl; ++c) {
				const uint32_t b = (c < 4 ? qq.x >> (8 * c) : qq.y >> (8 * (c - 4))) & 0xff;
				const int diag = c == 0 ? hleft : (int)(x[c - 1] & 0xffff);
				const int sc = (int)__builtin_amdgcn_perm(sr.y, sr.x, 0x0c0c0c00u | (b & 7)) - 128;
				a[c] = max(min(diag + sc, 32767), (int)(x[c] >> 16)); // ksw.c:263-265: adds_epi16, then max with E
				const int wadd = wadd0 + e_ins * c, sbig = (int)(b & 0x38) << 22;
				fs[c] = wadd + o_ins, sf[c] = fs[c] + sbig; // e_ins * (j - 1), and seg * 2^25 on top
				pre[c] = loc, spre[c] = sloc;
				const int w = a[c] + wadd;
				loc = max(loc, w), sloc = max(sloc, w + sbig);
			}
			const int incl = wave_scan_max(loc), sincl = wave_scan_max(sloc);
			const int ex = max(wave_shr1(incl, NEG), fcarry), sex = max(wave_shr1(sincl, NEG), scarry);
			fcarry = max(fcarry, __builtin_amdgcn_readlane(incl, 63)), scarry = max(scarry, __builtin_amdgcn_readlane(sincl, 63));
			uint32_t y[kSwLongCpl];
			uint32_t ck = 0;
#pragma unroll
			for (int c = 0; c < kSwLongCpl; ++c) {
				const int ffull = max(max(ex, pre[c]) - fs[c], 0);
				const int fseg = max(max(sex, spre[c]) - sf[c], 0); // an earlier segment's entry ends below zero
				const int hpre = max(a[c], fseg), h = max(hpre, ffull);
				const int e = max(max((int)(x[c] >> 16) - e_del, hpre - oe_del), 0); // ksw.c:268-270, from the uncorrected H
				y[c] = (uint32_t)e << 16 | (uint32_t)h;
				ck = max(ck, (uint32_t)h << 16 | (uint32_t)(65535 - (j0 + c))); // ties -> the smallest column
			}
			hp[0] = make_uint4(y[0], y[1], y[2], y[3]), hp[1] = make_uint4(y[4], y[5], y[6], y[7]);
			if (j0 < Q) key = max(key, ck); // (a lane's eight columns are all inside the padded query or all past it)
		}
		const uint32_t rk = (uint32_t)wave_reduce_max((int)key); // h <= 32767: the key stays positive
		const int imax = (int)(rk >> 16), arg = 65535 - (int)(rk & 0xffff);
		nrows = i + 1;
		if (rm && lane == 0) rm[i] = (uint16_t)imax;
		if (imax > gmax) { // ksw.c:306-311
			gmax = imax, te = i, qe = arg;
			if (gmax >= endsc) break;
		}
	}
	r.score = gmax, r.te = te, r.qe = te < 0 ? 0 : qe; // Hmax stays all zero when nothing scored: index 0 wins, ksw.c:316-320
	if (rm) {
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); // lane 0's row maxima before every lane reads them
		int s2 = -1, t2 = -1;
		sw_second_best(rm, 1, nrows, minsc, r.score, te, P.max_mat, &s2, &t2);
		r.score2 = s2, r.te2 = t2;
	}
	return r;
}

// cols: state capacity of this variant (a multiple of kSwLongChunk); qskip: the LDS variant leaves tasks whose padded query exceeds
// it to the slab variant (-1: none), the slab variant leaves those at or below it; wave_cols: tasks sw_wave_kernel takes at that
// width have been served; stat: running count of the tasks this kernel served (bmh_sw_wide_stats)
template <bool SLAB>
__global__ __launch_bounds__(64) void sw_long_kernel(const uint8_t *__restrict__ pool, const bmh_sw_task_t *__restrict__ tasks,
                                                     const uint32_t *__restrict__ order, const uint32_t *__restrict__ count, long long n,
                                                     bmh_sw_result_t *__restrict__ out, DevParams P, int cols, int qskip, int wave_cols,
                                                     uint8_t *__restrict__ slab, long long slice, uint16_t *__restrict__ rmslab,
                                                     int rows_cap, unsigned long long *__restrict__ stat, int *__restrict__ err_flag)
{
	extern __shared__ __align__(16) unsigned char smem[];
	__shared__ uint2 srow[8]; // [t] = scores of target base t against {A, C, G, T, N, pad, past, -}, biased by 128
	const int lane = threadIdx.x;
	if (lane < 8) {
		uint32_t lo = 0x80808080u, hi = 0x80808080u;
		if (lane < 5) {
			lo = 0;
			for (int q = 0; q < 4; ++q) lo |= (uint32_t)(uint8_t)(mat_at(P, lane * 5 + q) + 128) << (8 * q);
			hi = 0x80808000u | (uint32_t)(uint8_t)(mat_at(P, lane * 5 + 4) + 128);
		}
		srow[lane] = make_uint2(lo, hi);
	}
	__syncthreads();
	unsigned char *base = SLAB ? slab + (size_t)blockIdx.x * (size_t)slice : smem;
	uint32_t *he = (uint32_t *)base;        // [cols]
	uint8_t *qc = base + (size_t)cols * 4;  // [cols]
	uint16_t *rm = rmslab + (size_t)blockIdx.x * (size_t)rows_cap;
	const long long cnt = count ? (long long)*count : n;
	for (long long kk = blockIdx.x; kk < cnt; kk += gridDim.x) {
		const long long k = order ? (long long)order[kk] : kk;
		const bmh_sw_task_t tk = tasks[k];
		const int qlen = tk.qlen, tlen = (int)min(tk.tlen, 0x7fffffffu);
		const uint32_t xtra = tk.xtra;
		if (!sw_long_takes(P, qlen, xtra, wave_cols)) continue; // sw_generic_kernel's
		const int Q = (qlen + 7) & ~7;
		if (SLAB ? Q <= qskip : (qskip >= 0 && Q > qskip)) continue; // the other variant's
		if (lane == 0) atomicAdd(stat, 1ull);
		bmh_sw_result_t res;
		res.score = 0, res.te = res.qe = res.score2 = res.te2 = res.tb = res.qb = -1, res.rsv = 0;
		if (Q > cols || tlen > rows_cap) { // (launch_sw_long sizes both from the batch)
			res.score = INT32_MIN;
			if (lane == 0) out[k] = res, atomicExch(err_flag, BMH_E_RANGE);
			continue;
		}
		SwLongSeq seq;
		seq.pool = pool, seq.q_off = tk.q_off, seq.t_off = tk.t_off;
		seq.qrev = tk.flags & BMH_F_QREV, seq.qcomp = tk.flags & BMH_F_QCOMP, seq.trev = tk.flags & BMH_F_TREV;
		seq.tpac = tk.flags & BMH_F_TPAC, seq.qfold = -1, seq.tfold = -1;
		const int thr = (int)(xtra & 0xffff);
		const int minsc = (xtra & BMH_SW_XSUBO) ? thr : 0x10000, endsc = (xtra & BMH_SW_XSTOP) ? thr : 0x10000; // ksw.c:246-247
		const SwCore f = sw_long_pass(seq, P, srow, qlen, tlen, minsc, endsc, he, qc, (xtra & BMH_SW_XSUBO) ? rm : nullptr);
		res.score = f.score, res.te = f.te, res.qe = f.qe, res.score2 = f.score2, res.te2 = f.te2;
		if ((xtra & BMH_SW_XSTART) && !((xtra & BMH_SW_XSUBO) && f.score < thr)) { // ksw.c:351-362
			seq.qfold = f.qe, seq.tfold = f.te;
			const SwCore rr = sw_long_pass(seq, P, srow, f.qe + 1, tlen, 0x10000, f.score, he, qc, nullptr);
			if (rr.score == f.score) res.tb = f.te - rr.te, res.qb = f.qe - rr.qe;
		}
		if (lane == 0) out[k] = res;
	}
}

// Every task listed in d_order[0..*d_count) (or 0..n) that sw_long_takes: padded queries up to kSwLongLdsCols columns on the LDS
// variant, longer ones on the slab variant.  qmax / qmin: longest and shortest query of the batch, tcap: its longest target.
int launch_sw_long(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_sw_task_t *d_tasks, int64_t n, bmh_sw_result_t *d_res,
                   const uint32_t *d_order, const uint32_t *d_count, int qmax, int qmin, int tcap, int wave_cols)
{
	if (n <= 0) return BMH_OK;
	qmax = std::min(std::max(qmax, 1), 65535), qmin = std::max(qmin, 1);
	const int call = (((qmax + 7) & ~7) + kSwLongChunk - 1) / kSwLongChunk * kSwLongChunk;
	const bool need_slab = call > kSwLongLdsCols, need_lds = ((qmin + 7) & ~7) <= kSwLongLdsCols;
	const int clds = std::min(call, kSwLongLdsCols);
	const int rows_cap = (std::max(tcap, 1) + 63) & ~63;
	long long grid = std::min<long long>(n, ext_resident_waves(ctx, 4)); // 4 waves per SIMD: a few thousand tasks in flight
	while (grid > 64 && (long long)rows_cap * 2 * grid > (1LL << 29)) grid /= 2; // the row-maximum slab within 512 MiB
	long long gslab = 0, slice = 0;
	if (need_slab) {
		slice = (sw_long_state_bytes(call) + 255) & ~255LL;
		gslab = std::min<long long>({kSwLongSlabBudget / slice, 2048, n, grid});
	}
	const size_t rm_bytes = ((size_t)grid * (size_t)rows_cap * 2 + 255) & ~(size_t)255;
	int rc;
	if ((rc = ensure(ctx, ctx->d_swl, rm_bytes + (size_t)gslab * (size_t)slice))) return rc;
	uint16_t *d_rm = (uint16_t *)ctx->d_swl.p;
	const bool tm = ctx->timing;
	if (tm && !ctx->ev_swl[0]) {
		BMH_HIP(ctx, hipEventCreate(&ctx->ev_swl[0]));
		BMH_HIP(ctx, hipEventCreate(&ctx->ev_swl[1]));
	}
	if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_swl[0], ctx->stream));
	if (need_lds) {
		hipLaunchKernelGGL(sw_long_kernel<false>, dim3((unsigned)grid), dim3(64), (size_t)sw_long_state_bytes(clds), ctx->stream, d_pool,
		                   d_tasks, d_order, d_count, (long long)n, d_res, ctx->dev, clds, need_slab ? clds : -1, wave_cols,
		                   (uint8_t *)nullptr, 0LL, d_rm, rows_cap, ctx->d_swl_stat, ctx->d_err);
		BMH_HIP(ctx, hipGetLastError());
	}
	if (need_slab) {
		hipLaunchKernelGGL(sw_long_kernel<true>, dim3((unsigned)gslab), dim3(64), 0, ctx->stream, d_pool, d_tasks, d_order, d_count,
		                   (long long)n, d_res, ctx->dev, call, need_lds ? clds : 0, wave_cols, (uint8_t *)ctx->d_swl.p + rm_bytes, slice,
		                   d_rm, rows_cap, ctx->d_swl_stat, ctx->d_err);
		BMH_HIP(ctx, hipGetLastError());
	}
	if (tm) { // (a measurement mode: wait, and add the kernels' time to the running sum bmh_sw_wide_stats reports)
		float ms = 0.f;
		BMH_HIP(ctx, hipEventRecord(ctx->ev_swl[1], ctx->stream));
		BMH_HIP(ctx, hipEventSynchronize(ctx->ev_swl[1]));
		BMH_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_swl[0], ctx->ev_swl[1]));
		ctx->swl_ms_sum += ms;
	}
	return BMH_OK;
}

} // namespace bmh
