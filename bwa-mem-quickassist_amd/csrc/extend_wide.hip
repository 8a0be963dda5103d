// extend_wide.hip -- ksw_extend2 over int32: the extension tasks the 16-bit kernels refuse (opt-in per context,
// bmh_ctx_set_wide_extension).
//
// Replaces ksw_extend2 (reference bwa-0.7.8/ksw.c:379-476) for scores past kScoreLimit, queries past the LDS kernel's
// 13 632 columns, and gap costs past 16 bits.  The walk is extend_lds_kernel's: one wave64 per task, rows in order, the
// adaptive [beg,end) interval, F as a 6-step DPP max-plus scan, z-drop and the m == 0 exit as wave-uniform scalars, the
// interval update from zero-scan ballots.  What changes:
//   * H (shifted, = eh[j].h) and E (= eh[j].e) are two int32 arrays, as in global_kernel; the query profile is five
//     planes of int8 (plane = target base), so a row reads one byte per column: 13 bytes per column in all.
//   * The row maximum is a max-reduction of h followed by a ballot of the lanes that hold it; the highest such lane is
//     the right-most column (ties -> larger j, ksw.c:434).  Chunks run left to right, so a later chunk wins a tie.
//   * Gap costs are int32 operands.  Inside the cell every H, E, F lies in [0, S] with S = h0 + qlen*max(mat), so a gap
//     cost above S acts exactly like S + 1 (anything it subtracts ends at the clamp to 0); the kernel uses that capped
//     value, which keeps lane*e of the scan inside int32 for any e.  The first column, the band clamp and the z-drop
//     test use the uncapped costs in the reference's int arithmetic.
//   * Two variants (SLAB = false / true): the state in LDS while qcap <= kWideLdsQcap, otherwise in a per-block slice of
//     an HBM slab.  The slab variant takes only the tasks the LDS variant cannot hold; every slab write is checked
//     against the slice, and a workgroup fence orders a row's stores before the lanes that read them.
// Integer only (no MFMA: this is a max-plus recurrence, not a contraction).
#include "bmh_ctx.h"
#include "bmh_device.h"

namespace bmh {

constexpr int kWideNeg = -(1 << 29); // scan identity: below every g >= 0, and still inside int32 after 64 * (kWideScoreLimit + 1)

// bytes of one task's state at query capacity qcap: H and E int32 [qcap+2] each, profile int8 [5][qcap]
__host__ __device__ constexpr long long wide_state_bytes(int qcap) { return 8LL * (qcap + 2) + 5LL * qcap; }
static_assert(wide_state_bytes(kWideLdsQcap) + 32 <= 160 * 1024, "the LDS variant must fit 160 KiB");
static_assert(wide_state_bytes(kWideLdsQcap + 64) + 32 > 160 * 1024, "kWideLdsQcap is the largest multiple of 64 that fits");
static_assert(64LL * (kWideScoreLimit + 1) - kWideNeg < 0x7fffffffLL, "scan terms stay inside int32");

__device__ __forceinline__ void wide_store_result(bmh_ext_result_t *o, int score, int qle, int tle, int gtle, int gscore, int max_off)
{
	int *p = (int *)o;
	p[0] = score, p[1] = qle, p[2] = tle, p[3] = gtle, p[4] = gscore, p[5] = max_off;
}

template <bool SLAB>
__device__ __forceinline__ void wide_fence()
{
	if constexpr (SLAB) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); // one wave per block: orders its own lanes' accesses
}

// qcap: query capacity of this variant's state; qskip: tasks with qlen <= qskip belong to the other variant (SLAB) or
// tasks with qlen > qskip do (LDS; -1: none do); slab/slice: the HBM slab and the bytes of one block's slice (SLAB);
// stat: running count of the tasks this bin received (LDS variant, block 0)
template <bool SLAB>
__global__ __launch_bounds__(64) void extend_wide_kernel(const uint8_t *__restrict__ pool, const bmh_ext_task_t *__restrict__ tasks,
                                                         const uint32_t *__restrict__ order, const uint32_t *__restrict__ count, long long n,
                                                         bmh_ext_result_t *__restrict__ out, DevParams P, int qcap, int qskip,
                                                         uint8_t *__restrict__ slab, long long slice,
                                                         unsigned long long *__restrict__ stat, int *__restrict__ err_flag)
{
	extern __shared__ __align__(16) unsigned char smem[];
	__shared__ int8_t smat[32];
	unsigned char *base = SLAB ? slab + (size_t)blockIdx.x * (size_t)slice : smem;
	int *H = (int *)base;                          // [qcap+2] shifted H = eh[j].h
	int *E = H + (qcap + 2);                       // [qcap+2] eh[j].e
	int8_t *PR = (int8_t *)(E + (qcap + 2));       // [5][qcap] score of query column j against target base t
	const int lane = threadIdx.x;

	if (lane < 25) smat[lane] = (int8_t)mat_at(P, lane);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");

	if (count) n = *count; // bin size produced on the device by the dispatcher
	if (!SLAB && stat && blockIdx.x == 0 && lane == 0) atomicAdd(stat, (unsigned long long)n);
	for (long long slot = blockIdx.x; slot < n; slot += gridDim.x) {
		const uint32_t idx = order ? order[slot] : (uint32_t)slot;
		const uint4 *tp = (const uint4 *)(tasks + idx);
		const uint4 ta = tp[0], tb = tp[1];
		const uint64_t q_off = (uint64_t)(uint32_t)uni(ta.y) << 32 | (uint32_t)uni(ta.x);
		const uint64_t t_off = (uint64_t)(uint32_t)uni(ta.w) << 32 | (uint32_t)uni(ta.z);
		const int qlen = uni(tb.x & 0xffff), tlen = uni(tb.x >> 16);
		int h0 = uni(tb.y);
		int w = uni((int)(int16_t)(tb.z & 0xffff));
		const int end_bonus = uni((int)(int16_t)(tb.z >> 16));
		const bool qrev = uni(tb.w) & BMH_F_QREV, trev = uni(tb.w) & BMH_F_TREV, tpac = uni(tb.w) & BMH_F_TPAC;
		if (SLAB ? qlen <= qskip : (qskip >= 0 && qlen > qskip)) continue; // the other variant's task
		if (h0 < 0) h0 = 0; // ksw.c:384

		if (qlen > qcap || (long long)h0 + (long long)qlen * P.max_mat > kWideScoreLimit) { // outside the supported range: fail loudly
			if (lane == 0) {
				wide_store_result(out + idx, INT32_MIN, 0, 0, 0, 0, 0);
				atomicExch(err_flag, BMH_E_RANGE);
			}
			continue;
		}
		// gap costs inside the cell, capped at S + 1 (see the head of the file)
		const int S1 = h0 + qlen * P.max_mat + 1;
		const int e_del = min(P.e_del, S1), e_ins = min(P.e_ins, S1);
		const int oe_del = (int)min((long long)P.o_del + P.e_del, (long long)S1), oe_ins = (int)min((long long)P.o_ins + P.e_ins, (long long)S1);

		// first row (closed form of ksw.c:394-396, no overflow for any e) and query profile (ksw.c:389-392)
		for (int j = lane; j <= qlen; j += 64) {
			const long long v = j == 0 ? h0 : (long long)h0 - ((long long)P.o_ins + P.e_ins) - (long long)(j - 1) * P.e_ins;
			if (!SLAB || j < qcap + 2) H[j] = (int)(v > 0 ? v : 0), E[j] = 0;
			if (j < qlen) {
				const int qb = seq_base(pool, q_off, j, qrev);
				if (!SLAB || j < qcap)
					for (int k = 0; k < 5; ++k) PR[k * qcap + j] = smat[k * 5 + qb];
			}
		}
		wide_fence<SLAB>();

		// band clamp, ksw.c:398-406
		w = min(w, max(1, band_cap(qlen, P.max_mat, end_bonus, P.o_ins, P.e_ins)));
		w = min(w, max(1, band_cap(qlen, P.max_mat, end_bonus, P.o_del, P.e_del)));

		int beg = 0, end = qlen, best = h0, bi = -1, bj = -1, gi = -1, gscore = -1, max_off = 0;
		uint32_t tv = 0;

		for (int i = 0; i < tlen; ++i) {
			if ((i & 255) == 0) { // stage the next 256 target bases, 4 per lane
				tv = 0;
				for (int k = 0; k < 4; ++k) {
					const int r = i + lane * 4 + k;
					if (r < tlen) tv |= (uint32_t)tgt_base(pool, P, t_off, r, trev, tpac) << (8 * k);
				}
			}
			const int tw = __builtin_amdgcn_readlane((int)tv, (i >> 2) & 63);
			const int t = (tw >> ((i & 3) * 8)) & 0xff;
			const int8_t *prt = PR + (t < 4 ? t : 4) * qcap;
			// ksw.c:415-416 in the reference's int arithmetic (two's complement, as its build computes it)
			const int left0 = max(0, (int)((unsigned)h0 - ((unsigned)P.o_del + (unsigned)P.e_del * (unsigned)(i + 1))));
			beg = max(beg, i - w); // ksw.c:418-420
			end = min(end, min(i + w + 1, qlen));

			int carry_h = left0; // H(i, cb-1): what column cb stores as its shifted H
			int fin = 0;         // F(i, cb)
			int m = -1, mj = -1; // row maximum and its right-most column
			for (int cb = beg; cb < end; cb += 64) { // ksw.c:421-445, 64 columns at a time
				const int j = cb + lane;
				const bool act = j < end;
				int M = 0, e = 0, s = 0;
				if (act) M = H[j], e = E[j], s = prt[j];
				const int hh = max(M + s, e);
				const int g = act ? max(hh - oe_ins, 0) + lane * e_ins : kWideNeg;
				const int pm = wave_scan_max(g);
				const int pex = wave_shr1(pm, kWideNeg);
				const int F = max(max(pex - (lane - 1) * e_ins, fin - lane * e_ins), 0);
				const int h = max(hh, F);
				const int en = max(max(e - e_del, h - oe_del), 0);
				const int hprev = wave_shr1(h, carry_h);
				if (act && (!SLAB || j < qcap + 2)) H[j] = hprev, E[j] = en;
				const int nact = end - cb;
				if (nact >= 64) {
					carry_h = __builtin_amdgcn_readlane(h, 63);
					fin = max(fin - 64 * e_ins, __builtin_amdgcn_readlane(pm, 63) - 63 * e_ins);
				} else carry_h = __builtin_amdgcn_readlane(h, nact - 1);
				const int cm = wave_reduce_max(act ? h : -1);
				if (cm >= m) {
					const unsigned long long bm = __ballot(act && h == cm);
					m = cm, mj = cb + 63 - __builtin_clzll(bm);
				}
			}
			if (lane == 0 && (!SLAB || end < qcap + 2)) H[end] = carry_h, E[end] = 0; // eh[end] = {h1, 0}  (ksw.c:446)
			wide_fence<SLAB>();

			if (m < 0) m = 0, mj = -1; // an empty row
			if ((beg < end ? end : beg) == qlen) { // ksw.c:447-450 (`j == qlen` on the loop variable)
				if (!(gscore > carry_h)) gi = i;
				gscore = max(gscore, carry_h);
			}
			if (m == 0) break; // ksw.c:451
			if (m > best) {    // ksw.c:452-454
				best = m, bi = i, bj = mj;
				max_off = max(max_off, abs(mj - i));
			} else if (P.zdrop > 0) { // ksw.c:455-461, int arithmetic as in the reference
				const int di = i - bi, dj = mj - bj;
				if (di > dj) {
					if ((int)((unsigned)(best - m) - (unsigned)(di - dj) * (unsigned)P.e_del) > P.zdrop) break;
				} else {
					if ((int)((unsigned)(best - m) - (unsigned)(dj - di) * (unsigned)P.e_ins) > P.zdrop) break;
				}
			}
			// live-interval update, ksw.c:463-466: nearest zero of H left of mj / right of mj+2
			int nb = beg;
			for (int hi = mj; hi >= beg; hi -= 64) {
				const int j = hi - lane;
				const bool z = j >= beg && H[j] == 0;
				const unsigned long long bm = __ballot(z);
				if (bm) {
					nb = hi - __builtin_ctzll(bm) + 1;
					break;
				}
			}
			int ne;
			for (int lo = mj + 2;; lo += 64) {
				const int j = lo + lane;
				bool z = true;
				if (j <= end) z = H[j] == 0;
				const unsigned long long bm = __ballot(z);
				if (bm) {
					ne = lo + __builtin_ctzll(bm);
					break;
				}
			}
			beg = nb, end = ne;
		}
		if (lane == 0) wide_store_result(out + idx, best, bj + 1, bi + 1, gi + 1, gscore, max_off);
		wide_fence<SLAB>(); // the next task's first row overwrites this one's state
	}
}

// ---- launcher: every task listed in d_order[0..*d_count) (or 0..n when d_count is null).  Tasks of up to kWideLdsQcap
// columns run on the LDS variant; longer ones, when qmax asks for them, on the slab variant, whose grid is capped so that the
// slab stays within kWideSlabBudget.
constexpr long long kWideSlabBudget = 1LL << 30;

int launch_extend_wide(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n, bmh_ext_result_t *d_res,
                       const uint32_t *d_order, const uint32_t *d_count, int qmax, long long grid_cap)
{
	if (n <= 0) return BMH_OK;
	if (qmax < 1) qmax = 1;
	if (qmax > 65535) qmax = 65535;
	const int qall = (qmax + 63) & ~63;
	const bool need_slab = qall > kWideLdsQcap;
	const int qlds = need_slab ? kWideLdsQcap : qall;
	const size_t shmem = (size_t)((wide_state_bytes(qlds) + 15) & ~15LL);
	long long grid = n < kPersistentGrid ? n : kPersistentGrid;
	if (grid_cap > 0 && grid > grid_cap) grid = grid_cap;
	hipLaunchKernelGGL(extend_wide_kernel<false>, dim3((unsigned)grid), dim3(64), shmem, ctx->stream, d_pool, d_tasks, d_order, d_count,
	                   (long long)n, d_res, ctx->dev, qlds, need_slab ? qlds : -1, (uint8_t *)nullptr, 0LL,
	                   (unsigned long long *)ctx->d_wide_stat, ctx->d_err);
	BMH_HIP(ctx, hipGetLastError());
	if (need_slab) {
		const long long slice = (wide_state_bytes(qall) + 255) & ~255LL;
		long long g = kWideSlabBudget / slice; // 1 GiB: 1 260 slices of 65 535 columns
		if (g > 1024) g = 1024;
		if (g > n) g = n;
		if (grid_cap > 0 && g > grid_cap) g = grid_cap;
		int rc = ensure(ctx, ctx->d_wide_slab, (size_t)g * (size_t)slice);
		if (rc) return rc;
		hipLaunchKernelGGL(extend_wide_kernel<true>, dim3((unsigned)g), dim3(64), 0, ctx->stream, d_pool, d_tasks, d_order, d_count,
		                   (long long)n, d_res, ctx->dev, qall, qlds, (uint8_t *)ctx->d_wide_slab.p, slice,
		                   (unsigned long long *)nullptr, ctx->d_err);
		BMH_HIP(ctx, hipGetLastError());
	}
	return BMH_OK;
}

} // namespace bmh
