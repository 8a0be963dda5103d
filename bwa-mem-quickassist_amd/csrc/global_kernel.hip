// global_kernel.hip -- banded global (NW) affine alignment with traceback to a BAM CIGAR.
//
// Replaces ksw_global2 (reference bwa-0.7.8/ksw.c:501-584; spec SURVEY.md A.2).
// One wave64 per task, row-synchronous like the extension kernel:
//   * fixed band [max(0,i-w), min(qlen,i+w+1)) per row (ksw.c:528-529), 64 columns per chunk;
//   * H (shifted) and E as int32 in LDS (scores go far negative, -0x40000000 marks "outside"),
//     query profile 5 signed bytes per column in LDS;
//   * F(i,j+1)=max(F(i,j)-e_ins, M(i,j)-o_ins-e_ins) opens from the DIAGONAL score M
//     (ksw.c:538-541,557-560), so it is an exact max-plus prefix scan over lanes (6 DPP steps);
//   * one direction byte per cell, same encoding as the reference (ksw.c:547-561), written
//     row-contiguously either to LDS (ZLDS) or to a per-block HBM scratch slab;
//   * the traceback (ksw.c:566-581) is wave-parallel: the 64 lanes look 64 cells ahead along
//     the current direction (diagonal / column / row), a ballot finds where the run ends, so
//     one iteration emits a whole CIGAR run instead of one cell.
//   * CIGAR words are produced last-op-first and stored from the back of the task's slot
//     range, which leaves them in forward order; they are then moved to the front.
//   * queries past the LDS row (kGlbLdsQcap columns) run with RING: H and E in a ring of band slots (bin 4).
#include "bmh_ctx.h"
#include "bmh_device.h"
#include "../host/glbband_core.h"
#include "../host/glbbin_core.h"

namespace bmh {

constexpr int kNegInf = -0x40000000; // MINUS_INF, ksw.c:487

struct CigarSink { // wave-uniform run-length CIGAR builder writing backwards from slot cap-1
	uint32_t *base;
	int cap, nw, last_op, last_len;
	__device__ __forceinline__ void flush(int lane)
	{
		if (last_len > 0) {
			if (nw < cap && lane == 0) base[cap - 1 - nw] = (uint32_t)last_len << 4 | (uint32_t)last_op;
			++nw;
		}
	}
	__device__ __forceinline__ void push(int op, int len, int lane)
	{
		if (len <= 0) return;
		if (last_len > 0 && op == last_op) last_len += len; // ksw.c:497
		else {
			flush(lane);
			last_op = op, last_len = len;
		}
	}
};

// One DP body, two state layouts.  RING = false: H, E and the profile of every query column in LDS (global_kernel, qcap =
// query capacity).  RING = true: H and E of column j in slot j mod qcap of a ring of qcap slots (a power of two >=
// 2*min(w,qlen)+2), the query bytes in a ring of 2*qcap, the cell's score formed from the query byte and the target base's
// row of smat.  Only the addressing of H, E and the profile differs; the F scan, the hand-over between
// chunks, the direction bytes and the traceback are the same code.  RING is bin 4's kernel: the tasks of bin 2 whose query
// rows do not fit LDS, direction bytes in the HBM slab; its block 0 adds the bin's size to the context's running count in
// err_flag[2..3] (bmh_global_long_stats).
template <bool ZLDS, bool RING = false>
__global__ __launch_bounds__(64) void global_kernel(const uint8_t *__restrict__ pool,
                                                    const bmh_glb_task_t *__restrict__ tasks,
                                                    const uint32_t *__restrict__ order,
                                                    const uint32_t *__restrict__ count, long long n,
                                                    bmh_glb_result_t *__restrict__ out,
                                                    uint32_t *__restrict__ cigar_pool, DevParams P, int qcap,
                                                    long long zcap, uint8_t *__restrict__ zscratch,
                                                    int *__restrict__ err_flag)
{
	extern __shared__ __align__(16) unsigned char smem[];
	int *H = (int *)smem;                              // [qcap+2] shifted H = eh[j].h  (RING: [qcap] slots)
	int *E = H + (RING ? qcap : qcap + 2);             // [qcap+2]                      (RING: [qcap] slots)
	uint2 *PR = (uint2 *)(E + (qcap + 2));             // [qcap]  (8-byte aligned: 2*(qcap+2) ints precede)
	uint8_t *Q = (uint8_t *)(E + qcap);                // RING: [2*qcap] query bytes, column j in j mod 2*qcap
	int8_t *smat = RING ? (int8_t *)(Q + 2 * qcap) : (int8_t *)(PR + qcap); // [32]
	uint8_t *zl = (uint8_t *)(smat + 32);              // [zcap] when ZLDS
	uint8_t *z = ZLDS ? zl : zscratch + (size_t)blockIdx.x * (size_t)zcap;
	const int rmask = qcap - 1, qmask = 2 * qcap - 1;
	const int lane = threadIdx.x;
	const int oe_del = P.o_del + P.e_del, oe_ins = P.o_ins + P.e_ins;
	const int e_del = P.e_del, e_ins = P.e_ins;

	if (lane < 25) smat[lane] = (int8_t)mat_at(P, lane);
	uint32_t mrow = 0; // RING: lane r < 5 holds smat row r (target base r against query bases 0-3) and its column 4
	int mrow4 = 0;
	if (RING && lane < 5) {
		for (int k = 0; k < 4; ++k) mrow |= (uint32_t)(uint8_t)smat[lane * 5 + k] << (8 * k);
		mrow4 = smat[lane * 5 + 4];
	}
	if (RING && blockIdx.x == 0 && lane == 0) atomicAdd((unsigned long long *)(err_flag + 2), (unsigned long long)(count ? *count : n));

	if (count) n = *count; // bin size produced on the device by the dispatcher
	for (long long slot = blockIdx.x; slot < n; slot += gridDim.x) {
		const uint32_t idx = order ? order[slot] : (uint32_t)slot;
		const uint4 *tp = (const uint4 *)(tasks + idx);
		const uint4 ta = tp[0], tb = tp[1];
		const uint64_t q_off = (uint64_t)(uint32_t)uni(ta.y) << 32 | (uint32_t)uni(ta.x);
		const uint64_t t_off = (uint64_t)(uint32_t)uni(ta.w) << 32 | (uint32_t)uni(ta.z);
		const int qlen = uni(tb.x & 0xffff), tlen = uni(tb.x >> 16);
		const int w = uni((int)tb.y);
		const uint32_t cigar_off = (uint32_t)uni(tb.z);
		const int cigar_cap = uni(tb.w);
		const int n_col = min(qlen, 2 * w + 1); // ksw.c:509
		const bool want = cigar_cap > 0;

		if ((RING ? 2 * min(w, qlen) + 2 > qcap : qlen > qcap) || w < 0 || (want && (long long)n_col * tlen > zcap)) {
			if (lane == 0) {
				out[idx].score = INT32_MIN, out[idx].n_cigar = 0;
				atomicExch(err_flag, BMH_E_RANGE);
			}
			continue;
		}

		// first row, ksw.c:519-522, and profile, ksw.c:514-517
		const int wq = min(w, qlen);
		if (!RING) {
			for (int j = lane; j <= qlen; j += 64) {
				H[j] = j == 0 ? 0 : (j <= w ? -(P.o_ins + e_ins * j) : kNegInf);
				E[j] = kNegInf;
				if (j < qlen) {
					const int qb = pool[q_off + (uint64_t)j];
					uint32_t lo = 0;
					for (int k = 0; k < 4; ++k) lo |= (uint32_t)(uint8_t)smat[k * 5 + qb] << (8 * k);
					PR[j] = make_uint2(lo, (uint32_t)(uint8_t)smat[20 + qb]);
				}
			}
		} else {
			// column j > w enters the band at row j-w and is written one row earlier as H[end], E[end] (ksw.c:563): only
			// columns 0..min(qlen,w) need their initial values; the query bytes of the first band, the rest as the band slides
			for (int j = lane; j <= wq; j += 64) {
				H[j] = j == 0 ? 0 : -(P.o_ins + e_ins * j);
				E[j] = kNegInf;
				if (j < qlen) Q[j] = pool[q_off + (uint64_t)j];
			}
		}

		uint32_t tv = 0;
		for (int i = 0; i < tlen; ++i) { // ksw.c:524-564
			if ((i & 255) == 0) {
				tv = 0;
				for (int k = 0; k < 4; ++k) {
					const int r = i + lane * 4 + k;
					if (r < tlen) tv |= (uint32_t)pool[t_off + (uint64_t)r] << (8 * k);
				}
			}
			const int tw = __builtin_amdgcn_readlane((int)tv, (i >> 2) & 63);
			const int t = (tw >> ((i & 3) * 8)) & 0xff;
			int rlo = 0, r4 = 0;
			if (RING) {
				// every 64 rows: the query bytes of the next 64 columns to enter the band, i+w+1 .. i+w+64.  The columns 2*qcap
				// before them, whose slots they take, left the band before this row (2*qcap >= 2*w + 66: qcap >= 64 and >= 2*w + 2)
				const int c = i + wq + 1 + lane;
				if ((i & 63) == 0 && c < qlen) Q[c & qmask] = pool[q_off + (uint64_t)c];
				rlo = __builtin_amdgcn_readlane((int)mrow, t < 4 ? t : 4), r4 = __builtin_amdgcn_readlane(mrow4, t < 4 ? t : 4);
			}
			const int beg = i > w ? i - w : 0;
			const int end = i + w + 1 < qlen ? i + w + 1 : qlen;
			int carry_h = beg == 0 ? -(P.o_del + e_del * (i + 1)) : kNegInf; // ksw.c:530
			int fin = kNegInf;                                                // F(i, cb)
			uint8_t *zi = z + (size_t)i * n_col;
			for (int cb = beg; cb < end; cb += 64) {
				const int j = cb + lane;
				const bool act = j < end;
				const int js = RING ? j & rmask : j;
				int hs = 0, e = 0, qb = 0;
				uint2 pr = make_uint2(0, 0);
				if (act) {
					hs = H[js], e = E[js];
					if (RING) qb = Q[j & qmask];
					else pr = PR[j];
				}
				const int s = RING ? (qb < 4 ? (int)(int8_t)((uint32_t)rlo >> (qb * 8)) : r4)
				                   : t < 4 ? (int)(int8_t)(pr.x >> (t * 8)) : (int)(int8_t)pr.y;
				const int mm = hs + s;
				// F(i,j) = max(fin - (j-cb)*e_ins, max_{k<j}(mm_k - oe_ins - (j-1-k)*e_ins))
				const int g = act ? mm - oe_ins + lane * e_ins : INT32_MIN / 2;
				const int pm = wave_scan_max(g);
				const int pex = wave_shr1(pm, INT32_MIN / 2);
				const int f = max(pex - (lane - 1) * e_ins, fin - lane * e_ins);
				int d = mm >= e ? 0 : 1; // ksw.c:547-550
				int h = max(mm, e);
				d = h >= f ? d : 2;
				h = max(h, f);
				const int t1 = mm - oe_del, e2 = e - e_del; // ksw.c:552-556
				d |= e2 > t1 ? 1 << 2 : 0;
				const int en = max(e2, t1);
				d |= f - e_ins > mm - oe_ins ? 2 << 4 : 0; // ksw.c:557-559
				const int hprev = wave_shr1(h, carry_h);
				if (act) {
					H[js] = hprev, E[js] = en;
					if (want) zi[j - beg] = (uint8_t)d; // ksw.c:561
				}
				const int nact = end - cb;
				if (nact >= 64) {
					carry_h = __builtin_amdgcn_readlane(h, 63);
					fin = max(fin - 64 * e_ins, __builtin_amdgcn_readlane(pm, 63) - 63 * e_ins);
				} else carry_h = __builtin_amdgcn_readlane(h, nact - 1);
			}
			if (lane == 0 && end >= 0) H[RING ? end & rmask : end] = carry_h, E[RING ? end & rmask : end] = kNegInf; // ksw.c:563
		}
		// ksw.c:565.  When the last row's band ends short of qlen (qlen > tlen + w) no row wrote eh[qlen]: the reference returns its
		// initial value, -inf (qlen > w), which the whole-row layout still holds and the ring does not
		const int score = RING ? (qlen > tlen + w ? kNegInf : uni(H[qlen & rmask])) : uni(H[qlen]);

		int n_cigar = 0;
		if (want) { // traceback, ksw.c:566-581
			// the direction bytes were written by other lanes: drain our stores before reading them back
			__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
			CigarSink cs{cigar_pool + cigar_off, cigar_cap, 0, 0, 0};
			const long long zsize = (long long)n_col * tlen;
			int i = tlen - 1;
			int k = (i + w + 1 < qlen ? i + w + 1 : qlen) - 1;
			int which = 0;
			while (i >= 0 && k >= 0) {
				const int ii = which == 2 ? i : i - lane;
				const int kk = which == 1 ? k : k - lane;
				int f = 3; // "stop" for cells off the matrix
				if (ii >= 0 && kk >= 0) {
					long long zo = (long long)ii * n_col + (kk - (ii > w ? ii - w : 0));
					zo = zo < 0 ? 0 : (zo >= zsize ? zsize - 1 : zo); // stay inside the slab on out-of-domain input
					f = z[zo] >> (which << 1) & 3;
				}
				const unsigned long long bm = __ballot(f != which);
				const int run = bm ? __builtin_ctzll(bm) : 64;
				if (which == 0) {
					cs.push(0, run, lane), i -= run, k -= run;
					if (run < 64 && i >= 0 && k >= 0) {
						which = __builtin_amdgcn_readlane(f, run); // 1: came from E, 2: came from F
						if (which == 1) cs.push(2, 1, lane), --i;
						else cs.push(1, 1, lane), --k;
					}
				} else if (which == 1) {
					cs.push(2, run, lane), i -= run;
					if (run < 64 && i >= 0) cs.push(0, 1, lane), --i, --k, which = 0; // gap opened from the diagonal
				} else {
					cs.push(1, run, lane), k -= run;
					if (run < 64 && k >= 0) cs.push(0, 1, lane), --i, --k, which = 0;
				}
			}
			if (i >= 0) cs.push(2, i + 1, lane); // ksw.c:576-577
			if (k >= 0) cs.push(1, k + 1, lane);
			cs.flush(lane);
			n_cigar = cs.nw;
			// words sit at [cap-n, cap) in forward order; move them to [0, n)
			const int shift = cigar_cap - n_cigar;
			if (shift > 0 && n_cigar <= cigar_cap) {
				__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); // lane 0's words -> visible to all lanes
				for (int c = 0; c < n_cigar; c += 64) {
					uint32_t v = 0;
					if (c + lane < n_cigar) v = cs.base[shift + c + lane];
					if (c + lane < n_cigar) cs.base[c + lane] = v;
				}
			}
			if (n_cigar > cigar_cap && lane == 0) atomicExch(err_flag, BMH_E_CIGAR_CAP);
		}
		if (lane == 0) out[idx].score = score, out[idx].n_cigar = n_cigar;
	}
}

// ---- dispatcher -----------------------------------------------------------------------------------
// (w below: the band the lane kernels run the task on -- the band pass's w_eff, or the task's own with BMH_GLB_NARROW=0)
// bin 6: w <= 3   -> global_narrow_kernel     (eight waves per SIMD, each row on exactly its 2w+1 cells; BMH_GLB_EXACT >= 3)
// bin 7: w 4..7   -> global_narrow_kernel     (BMH_GLB_EXACT=7; the rule: host/glbbin_core.h)
// bin 5: w <= 15  -> global_lane_kernel<32>   (four waves per SIMD; with BMH_GLB_C32=0 these stay in bin 0)
// bin 0: w <= 31  -> global_lane_kernel<64>   (64 tasks per wave, band-relative registers)
// bin 1: w <= 63  -> global_lane_kernel<128>
// bin 3: 32 <= w <= 47 -> global_lane_kernel<96>
//        (an 80-slot instantiation for bands of 32-39 only pays at three waves per SIMD, and under 168 VGPRs its row loop spills
//        49 registers: not used)
// bin 2: wider bands, targets longer than the lane kernels' direction slab, or scores that could leave the
//        16-bit range -> global_kernel (one wave per task, int32 in LDS)
// bin 4: the tasks of bin 2 with more query columns than its LDS row holds (kGlbLdsQcap), when the launch has a bin 4 at all
//        (lds_qcap < 65535) -> global_kernel<false, true> (the band ring)
// Bins and the order inside them (by row count) come from the same device-side counting sort as the extension path.
// A task may run on a lane kernel when its rows fit the direction slab and no cell can leave the 16-bit range; which one, its band
// decides.  (The lane kernels take the sign of 16-bit differences such as m - e - o_del: with |m| < 12000, e and f no lower than
// one gap extension below the -16384 sentinel, and o_del + o_ins < 4000 these stay inside +-32767 -- the extension cancels in
// (m - o - e_x) - (e - e_x), and a large e_x forces short sequences, hence a small m.  tests/test_score_domain_gpu.py runs real
// scores of -11129 .. +11684, opens of 3999 in sum and extensions up to 2596 through every lane kernel.)
__device__ __forceinline__ bool glb_lane_domain(const DevParams &P, int qlen, int tlen, int w, int lane_ok, int rows_cap)
{
	const int emax = max(P.e_del, P.e_ins), smax = max(P.bias, P.max_mat);
	const int worst = P.o_del + P.o_ins + emax * (qlen + tlen) + smax * max(qlen, tlen); // |score| bound of any cell
	return lane_ok && tlen <= rows_cap && worst < kGlbLaneWorst && P.o_del + P.o_ins < 4000 && w >= 0;
}

// The band pass, in front of the sort: band[k] = the band the result of the task at input position k needs (host/glbband_core.h,
// DESIGN.md §4.6), for the tasks a lane kernel can take; 255 stands for "64 or wider", which no lane kernel runs.  By position and
// not by task: the indices in a caller's d_order may be sparse.  EIGHT lanes per task, each an eighth of the pairs in eight-base
// loads, joined in order: the eight lanes' loads fall into the task's two or three cache lines in the same instruction.  (One lane
// per task had every lane walk lines of its own: with all resident waves' lines far beyond the caches each 8-byte load fetched a
// whole line again, 8.6 ms for 8.5 M tasks, profiles/global_band.md.)  No LDS histogram here, so enough waves are resident to hide
// the loads -- inside glb_sort_hist_kernel (64 KiB of LDS, two blocks per CU) they would be exposed.
constexpr int kBandThreads = 256, kBandLanes = 8;
__global__ __launch_bounds__(kBandThreads) void glb_band_kernel(const uint8_t *__restrict__ pool, const bmh_glb_task_t *__restrict__ tasks,
                                                                const uint32_t *__restrict__ order, long long n, uint8_t *__restrict__ band,
                                                                DevParams P, int lane_ok, int rows_cap)
{
	__shared__ int8_t smat[32];
	if (threadIdx.x < 25) smat[threadIdx.x] = (int8_t)mat_at(P, threadIdx.x);
	__syncthreads();
	const int amax = bmh_glbband_amax(smat);
	const bool rule = bmh_glbband_applies(amax, P.o_del, P.e_del, P.o_ins, P.e_ins);
	const int g = threadIdx.x & (kBandLanes - 1);
	constexpr int kPer = kBandThreads / kBandLanes;
	for (long long k = (long long)blockIdx.x * kPer + threadIdx.x / kBandLanes; k < n; k += (long long)gridDim.x * kPer) { // (uniform in a group of eight)
		const uint32_t idx = order ? order[k] : (uint32_t)k;
		const uint4 *tp = (const uint4 *)(tasks + idx);
		const uint4 ta = tp[0], tb = tp[1];
		const int qlen = (int)(tb.x & 0xffff), tlen = (int)(tb.x >> 16);
		int w = (int)tb.y;
		if (rule && qlen >= 1 && tlen >= 1 && w >= abs(qlen - tlen) && glb_lane_domain(P, qlen, tlen, w, lane_ok, rows_cap)) {
			const bmh_gb_walk_t wk = bmh_glbband_walk(P.o_del, P.e_del, P.o_ins, P.e_ins, pool + ((uint64_t)ta.y << 32 | ta.x), qlen,
			                                          pool + ((uint64_t)ta.w << 32 | ta.z), tlen);
			const int per = ((wk.n + 8 * kBandLanes - 1) / (8 * kBandLanes)) * 8; // pairs per lane, a multiple of the eight-base load
			const int from = min(g * per, wk.n), to = min(from + per, wk.n);
			const bmh_gb_part_t mine = bmh_glbband_part(smat, &wk, from, to);
			bmh_gb_part_t acc = {0, 0, 0};
#pragma unroll
			for (int j = 0; j < kBandLanes; ++j) { // every lane joins the eight parts in order
				const bmh_gb_part_t nx = {__shfl(mine.s1, j, kBandLanes), __shfl(mine.d, j, kBandLanes), __shfl(mine.b, j, kBandLanes)};
				bmh_glbband_join(&acc, &nx);
			}
			w = bmh_glbband_from_lb(amax, P.o_del, P.e_del, P.o_ins, P.e_ins, qlen, tlen, w, acc.s1 + acc.b - wk.gap);
		}
		if (g == 0) band[k] = (uint8_t)(w < 0 || w > 255 ? 255 : w);
	}
}

__global__ __launch_bounds__(256) void glb_sort_hist_kernel(const bmh_glb_task_t *__restrict__ tasks,
                                                            const uint32_t *__restrict__ order, long long n,
                                                            uint32_t *__restrict__ hist, uint16_t *__restrict__ binkey,
                                                            DevParams P, int lane_ok, int rows_cap, int lds_qcap,
                                                            const uint8_t *__restrict__ band, int c32, int exact)
{
	__shared__ uint32_t lh[kSortBins * kSortKeysHost];
	for (int t = threadIdx.x; t < kSortBins * kSortKeysHost; t += 256) lh[t] = 0;
	__syncthreads();
	const long long chunk = (n + gridDim.x - 1) / gridDim.x, lo = chunk * blockIdx.x, hi = min(lo + chunk, n);
	for (long long k = lo + threadIdx.x; k < hi; k += 256) {
		const uint32_t idx = order ? order[k] : (uint32_t)k;
		const int qlen = tasks[idx].qlen, tlen = tasks[idx].tlen;
		int bin = 2, w = tasks[idx].w;
		if (glb_lane_domain(P, qlen, tlen, w, lane_ok, rows_cap)) {
			// the band pass has been here (band != null): the lane kernels run the task on band[k], so that picks the bin and the key.
			// It only ever narrows, so the host's gates (which lane kernels are launched at all) still hold
			if (band) w = band[k];
			bin = bmh_glb_lane_bin(w, c32, exact);
		}
		if (bin == 2 && qlen > lds_qcap) bin = 4;
		// inside a lane bin: rows first (lanes of a wave run until their longest target ends), then band width (a wave
		// computes and stores the 8-slot blocks that ANY of its lanes needs, and its lanes' tracebacks share cache lines
		// when they sit in the same block)
		// bins 6 and 7 the other way round, band first: a wave of global_narrow_kernel runs one row pass per band among its lanes
		const int bk = bin * kSortKeysHost + bmh_glb_sort_key(bin, tlen, w);
		binkey[k] = (uint16_t)bk;
		atomicAdd(&lh[bk], 1u);
	}
	__syncthreads();
	for (int t = threadIdx.x; t < kSortBins * kSortKeysHost; t += 256)
		if (lh[t]) atomicAdd(&hist[t], lh[t]);
}

int launch_global(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_glb_task_t *d_tasks, int64_t n,
                  bmh_glb_result_t *d_res, uint32_t *d_cigar, const uint32_t *d_order, int qmax, int tmax,
                  int wmax, int wgate, const GlbLongShape *lg)
{
	ctx->gband_n = 0, ctx->gbins_valid = false;
	if (n <= 0) return BMH_OK;
	int rc;
	const size_t N = (size_t)n;
	const bool lane_ok = ctx->glb_mode == 0;
	const bool longb = lg && lg->qmax > 0; // bin 4 is launched: the tasks of bin 2 past kGlbLdsQcap go to the ring
	const int rows_cap = std::max(tmax, longb ? lg->tmax : 0) < 512 ? std::max(tmax, longb ? lg->tmax : 0) : 512; // rows of the lane kernels' direction slab
	// plan both wave launches first: they share the HBM slab of direction bytes, which grows once, before either runs
	const long long budget = 8LL << 30; // HBM scratch for direction bytes, one slab per resident block
	const int qcap = (std::min(qmax, kGlbLdsQcap) + 63) & ~63;
	const size_t state = glb_state_bytes(qcap);
	const long long ncol = qmax < 2LL * wmax + 1 ? qmax : 2LL * wmax + 1;
	long long zcap = ncol * (long long)tmax;
	zcap = (zcap + 15) & ~15LL;
	if (zcap < 16) zcap = 16;
	if (state > kGlbLdsBytes) return BMH_E_RANGE;
	const bool zlds = state + (size_t)zcap <= 64 * 1024; // keep >= 2 blocks per CU in the LDS variant
	long long grid = n < (1LL << 20) ? n : (1LL << 20);
	if (lane_ok && grid > 8192) grid = 8192; // normally (almost) empty when the lane kernels are on
	if (!zlds) {
		long long g = budget / zcap;
		if (g < 1) return BMH_E_RANGE;
		if (g > 8192) g = 8192;
		if (grid > g) grid = g;
	}
	int ring = 64;
	long long zcap4 = 16, grid4 = 0;
	if (longb) { // bin 4: a ring of 2*min(w,qlen)+2 slots or more (up to kGlbRingMax) and its own slab, sized by the long tasks alone
		const int wq = std::min(lg->wmax, lg->qmax);
		while (ring < 2 * wq + 2 && ring < kGlbRingMax) ring <<= 1; // (a task past the largest ring is refused by the kernel)
		zcap4 = (std::min<long long>(lg->qmax, 2LL * lg->wmax + 1) * (long long)lg->tmax + 15) & ~15LL;
		if (zcap4 < 16) zcap4 = 16;
		long long g = budget / zcap4;
		if (g < 1) return BMH_E_RANGE;
		grid4 = std::min<long long>({g, 8192, std::max<int64_t>(lg->n, 1)});
	}
	const size_t slab = std::max(zlds ? 0 : (size_t)grid * (size_t)zcap, longb ? (size_t)grid4 * (size_t)zcap4 : 0);
	if (slab && (rc = ensure(ctx, ctx->d_scratch, slab))) return rc;

	uint32_t *counts, *lists;
	if ((rc = sort_tasks_begin(ctx, n, &counts, &lists))) return rc;
	uint32_t *hist = counts + 16;
	uint16_t *binkey = (uint16_t *)(hist + (size_t)kSortBins * kSortKeysHost);
	long long cg = (n + 1023) / 1024;
	if (cg > 512) cg = 512;
	// the bands the lane kernels will run on: by input position for the sort's first pass, then listed beside each bin's indices
	uint8_t *band = nullptr, *blists = nullptr;
	if (lane_ok && ctx->glb_narrow) {
		if ((rc = ensure(ctx, ctx->d_gband, (1 + (size_t)kSortBins) * N + 16))) return rc;
		band = (uint8_t *)ctx->d_gband.p, blists = band + ((N + 15) & ~(size_t)15);
		const long long bg = std::min<long long>((n * kBandLanes + kBandThreads - 1) / kBandThreads, (long long)ctx->ncu * 8 * 4);
		hipLaunchKernelGGL(glb_band_kernel, dim3((unsigned)bg), dim3(kBandThreads), 0, ctx->stream, d_pool, d_tasks, d_order, (long long)n,
		                   band, ctx->dev, 1, rows_cap);
		ctx->gband_n = n;
	}
	hipLaunchKernelGGL(glb_sort_hist_kernel, dim3((unsigned)cg), dim3(256), 0, ctx->stream, d_tasks, d_order, (long long)n, hist,
	                   binkey, ctx->dev, lane_ok ? 1 : 0, rows_cap, longb ? kGlbLdsQcap : 65535, band, ctx->glb_c32, ctx->glb_exact);
	if ((rc = sort_tasks_finish(ctx, n, d_order, (unsigned)cg, nullptr, nullptr, band, blists))) return rc;
	ctx->gbins_valid = true;
	const bool tm = ctx->timing;
	if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	if (lane_ok) {
		if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_gbin[0], ctx->stream));
		for (int b = 7; b >= 6; --b) // the exact-band bins, the wider one first
			if (ctx->glb_exact >= (b == 7 ? kGlbExactAll : kGlbExactLow) &&
			    (rc = launch_global_narrow(ctx, b == 7 ? 4 : 0, d_pool, d_tasks, n, d_res, d_cigar, lists + b * N, counts + b, rows_cap, blists ? blists + b * N : nullptr)))
				return rc;
		if (ctx->glb_c32 && (rc = launch_global_lane(ctx, 32, d_pool, d_tasks, n, d_res, d_cigar, lists + 5 * N, counts + 5, rows_cap,
		                                             blists ? blists + 5 * N : nullptr)))
			return rc;
		if ((rc = launch_global_lane(ctx, 64, d_pool, d_tasks, n, d_res, d_cigar, lists, counts + 0, rows_cap, blists))) return rc;
		if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_gbin[1], ctx->stream));
		// bands of 32..47 take the 96-slot instantiation (two waves per SIMD, three quarters of the slots), 48..63 the 128-slot one
		if (wgate > 31 && (rc = launch_global_lane(ctx, 96, d_pool, d_tasks, n, d_res, d_cigar, lists + 3 * N, counts + 3, rows_cap,
		                                             blists ? blists + 3 * N : nullptr)))
			return rc;
		if (wgate > 47 && (rc = launch_global_lane(ctx, 128, d_pool, d_tasks, n, d_res, d_cigar, lists + N, counts + 1, rows_cap,
		                                             blists ? blists + N : nullptr)))
			return rc;
	}
	if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_gbin[2], ctx->stream));
	{ // bin 2: the wave kernel
		const uint32_t *lst = lists + 2 * N, *cnt = counts + 2;
		if (zlds) {
			hipLaunchKernelGGL(global_kernel<true>, dim3((unsigned)grid), dim3(64), state + (size_t)zcap, ctx->stream, d_pool,
			                   d_tasks, lst, cnt, (long long)n, d_res, d_cigar, ctx->dev, qcap, zcap, (uint8_t *)nullptr, ctx->d_err);
		} else {
			hipLaunchKernelGGL(global_kernel<false>, dim3((unsigned)grid), dim3(64), state, ctx->stream, d_pool, d_tasks, lst, cnt,
			                   (long long)n, d_res, d_cigar, ctx->dev, qcap, zcap, (uint8_t *)ctx->d_scratch.p, ctx->d_err);
		}
		BMH_HIP(ctx, hipGetLastError());
	}
	if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_gbin[3], ctx->stream));
	if (longb) { // bin 4: the band ring, after bin 2 on the same stream (the two share the slab)
		if (tm && !ctx->ev_glong[0]) {
			BMH_HIP(ctx, hipEventCreate(&ctx->ev_glong[0]));
			BMH_HIP(ctx, hipEventCreate(&ctx->ev_glong[1]));
		}
		if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_glong[0], ctx->stream));
		hipLaunchKernelGGL((global_kernel<false, true>), dim3((unsigned)grid4), dim3(64), glb_ring_bytes(ring), ctx->stream, d_pool, d_tasks,
		                   lists + 4 * N, counts + 4, (long long)n, d_res, d_cigar, ctx->dev, ring, zcap4, (uint8_t *)ctx->d_scratch.p,
		                   ctx->d_err);
		BMH_HIP(ctx, hipGetLastError());
		if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_glong[1], ctx->stream));
	}
	if (tm) {
		BMH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
		ctx->ev_valid = true, ctx->ev_gbin_valid = lane_ok;
		if (longb) { // (a measurement mode: wait, and add the ring's time to the running sum bmh_global_long_stats reports)
			float ms = 0.f;
			BMH_HIP(ctx, hipEventSynchronize(ctx->ev_glong[1]));
			BMH_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_glong[0], ctx->ev_glong[1]));
			ctx->glong_ms_sum += ms;
		}
	}
	return BMH_OK;
}

} // namespace bmh
