// global_narrow.hip -- global_lane_kernel's method (global_lane.hip: one lane per task, band-relative row state, 4 direction bits per
// cell in a [block][row][lane] slab, the reference's traceback per lane) for bands of 0..7, with the band a COMPILE-TIME constant W of
// the row loop: a row computes exactly its 2W+1 cells, slides (2W+4)/4 window registers and stores one direction dword (W <= 3) or two.
// The 32-slot instantiation of global_lane_kernel charges such a task a whole masked 8-slot block per row (two for W >= 4), four block
// tests and eight window registers (profiles/global_exact.md).
//
// Same results as ksw_global2 (reference bwa-0.7.8/ksw.c:501-584).  Slot s of row i is column j = i-W+s, 0 <= s <= 2W; register s packs
// {H(i-1,j-1), E(i,j-1)} as two signed 16-bit halves, as there.  The vertical neighbour of the top slot, column i+W+1 of row i-1, lies
// outside the band for every row: its E is the constant -inf and needs no register.
//   * An INTERIOR row (W <= i < qlen-W: slots 0..2W are all inside the matrix) of every lane of the wave that still runs takes the
//     unmasked cell; the first W rows and the rows from qlen-W on take the masked one with the first-column fill (ksw.c:530).  The
//     choice is wave-uniform (a ballot), like FAST per block in global_lane_kernel.
//   * The band is per WAVE: the dispatcher sorts the two bins band-major, so the lanes of a wave share their band except where two
//     bands meet in the list.  Such a seam wave runs one row pass per distinct band with the other lanes idle -- never a lane on a band
//     other than its own: a wider one is not exact once it exceeds the task's w.
//   * W = 0 walks its one cell per row like the others (its direction bits are all "diagonal"); the traceback then reads them as for
//     any band.  (Not special-cased: see profiles/global_exact.md.)
//   * The sequences reach the row loop as in global_lane_kernel, through the same routine (glb_fill_stream, seq_stream.h): 64 rows
//     of {target base, incoming query base} staged in LDS per refill, in batches of unconditional loads with one wait each -- a row
//     here is 64..370 instructions, so the 17 and more waits per refill it had, one per four rows and one per byte near a lane's end, were a large part of a wave's lifetime.  The
//     query window of row 0 is one such batch.
// The traceback is a copy of global_lane_kernel's, so that kernel's register figures stay what they were.
#include <algorithm>
#include <type_traits>

#include "bmh_ctx.h"
#include "bmh_device.h"
#include "seq_stream.h"

namespace bmh {

namespace {

constexpr int kNeg16 = -16384;
constexpr int kTbRows = 16;     // rows of a path's block fetched together by the traceback (LDS strip of kTbRows x 64 dwords = 4 KB)
constexpr int kStreamRows = 64; // rows of the {target base, incoming query base} stream staged in LDS at a time
constexpr int kStreamBatch = 2; // dwords of each sequence a refill has in flight per wait: at 4, bands 0..3 spill 40 bytes more per lane
constexpr int kNarrowBlocks = 2; // direction dwords per row the slab has room for (W <= 7: 15 cells)

__device__ __forceinline__ int sel3n(int mask, int a, int b) { return __builtin_amdgcn_bitop3_b32(mask, a, b, 0xca); }

// The lane number, computed where it is used: kept in a register across the row loop it is spilled, and the reload's s_waitcnt vmcnt(0)
// in front of a direction-word store also waits for every such store in flight (see fill_stream in global_lane.hip)
__device__ __forceinline__ int lane_now()
{
	int l;
	asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
	return l;
}

// The rows of the lanes with `mine` set, all of band W.  Returns eh[qlen].h after the lane's last row (ksw.c:565), kNeg16 where no row
// wrote it.  Direction dwords of the lanes with `mine && want` go to zbase[(block * rows_cap + row) * 64 + lane].
template <int W, bool SYM>
__device__ __forceinline__ int narrow_rows(const bool mine, const bool want, const int qlen, const int tlen, const uint32_t idx,
                                           const uint8_t *__restrict__ pool, const bmh_glb_task_t *__restrict__ tasks, const DevParams &P,
                                           const uint2 *srow, uint8_t *strm, uint32_t *__restrict__ zbase, const int rows_cap)
{
	constexpr int NS = 2 * W + 1, NQ = (NS + 3) / 4, NB = (NS + 7) / 8;
	static_assert(NB <= kNarrowBlocks, "the slab holds kNarrowBlocks dwords per row");
	const int oe_del = P.o_del + P.e_del, oe_ins = P.o_ins + P.e_ins;
	const int e_del = P.e_del, e_ins = P.e_ins;
	const uint4 t0 = *(const uint4 *)(tasks + idx);
	const uint64_t q_off0 = (uint64_t)t0.y << 32 | t0.x;

	// ---- row state before row 0 (ksw.c:519-522): slot s is column s-W
	int R[NS], QW[NQ];
#pragma unroll
	for (int s = 0; s < NS; ++s) {
		const int j = s - W;
		const int hd = j < 0 ? kNeg16 : (j == 0 ? 0 : (j <= qlen ? -(P.o_ins + e_ins * j) : kNeg16)); // (j <= W always)
		R[s] = (int)((uint32_t)kNeg16 << 16 | ((uint32_t)hd & 0xffffu)); // {H(-1,j-1) as eh[j].h, E = -inf}
	}
	// the query window of row 0, four v_perm selectors per register: slot s looks at q[s-W]; 4 marks "no base"
	{ // one batch (seq_stream.h): positions [-W, 4 NQ - W)
		uint32_t qw[NQ];
		int ql = qlen; // (opaque, so that what the batch derives from it is not kept for the row loop: see glb_fill_stream)
		asm volatile("" : "+v"(ql));
		seq_issue<NQ>(qw, pool, q_off0, ql, -W, false, mine);
		seq_finish<NQ>(qw, ql, -W, false, mine);
#pragma unroll
		for (int v = 0; v < NQ; ++v) QW[v] = (int)qw[v];
	}
	constexpr int qsh = 4 * NQ - W; // row i takes q[i + qsh] into the top byte of the window for row i+1
	auto fill_stream = [&](int r0) { // rows [r0, r0 + kStreamRows) of the {t, q} stream, one byte per row at [row][lane] (global_lane.hip)
		const uint4 tq = *(const uint4 *)(tasks + idx);
		const uint64_t q_off = (uint64_t)tq.y << 32 | tq.x, t_off = (uint64_t)tq.w << 32 | tq.z;
		glb_fill_stream<kStreamRows, kStreamBatch>(strm, lane_now(), pool, t_off, tlen, q_off, qlen, r0, qsh, mine);
	};

	int score = kNeg16;
	for (int i = 0; __builtin_amdgcn_ballot_w64(mine && i < tlen) != 0; ++i) { // ksw.c:524-564; i is wave-uniform
		const bool rowon = mine && i < tlen;
		if ((i & (kStreamRows - 1)) == 0) fill_stream(i);
		const int lane = lane_now();
		const int sbyte = strm[(i & (kStreamRows - 1)) * 64 + lane];
		const int tcur = sbyte & 15, qin = sbyte >> 4;
		const uint2 row = srow[min(tcur, 4)];
		// masked unless every running lane's row holds all 2W+1 cells
		const bool masked = __builtin_amdgcn_ballot_w64(rowon && (i < W || i + W >= qlen)) != 0;
		uint32_t dzw[NB];
		auto cells = [&](auto MASKED) {
			int am = 0, fill = kNeg16;
			if constexpr (decltype(MASKED)::value) {
				const int lo = max(W - i, 0), hi = min(max(qlen - i + W, 0), NS); // slots [lo, hi) are cells of the matrix
				am = rowon && hi > lo ? (int)((0xffffffffu >> (32 - (hi - lo))) << lo) : 0;
				fill = i < W ? -(P.o_del + e_del * (i + 1)) : kNeg16; // ksw.c:530: first-column value while beg == 0
			}
			int f = kNeg16, dz12 = 0, dz34 = 0, sc4 = 0;
#pragma unroll
			for (int s = 0; s < NS; ++s) {
				const int c4 = s & 3;
				if (c4 == 0) sc4 = (int)__builtin_amdgcn_perm(row.y, row.x, (unsigned)QW[s >> 2]); // four substitution scores with one v_perm
				if ((s & 7) == 0) dz12 = dz34 = 0;
				const int m = c4 == 0 ? add_score<0>(sc4, R[s]) : c4 == 1 ? add_score<1>(sc4, R[s]) : c4 == 2 ? add_score<2>(sc4, R[s]) : add_score<3>(sc4, R[s]); // ksw.c:546
				const int e = s + 1 < NS ? (int)((unsigned)R[s + 1] >> 16) : (kNeg16 & 0xffff); // E(i,j); above the top slot: outside the band
				const int h1 = max16(m, e);                     // ksw.c:547-550
				const int h = max16(h1, f);
				const int t1 = subk16(m, oe_del), e2 = subk16(e, e_del); // ksw.c:552-556
				const int t2 = SYM ? t1 : subk16(m, oe_ins), f2 = subk16(f, e_ins); // ksw.c:557-560
				// the four sign bits of the cell (global_lane.hip): b1 = [m < e], b2 = [max(m,e) < f], b3 = E continues, b4 = F continues
				int x12 = sub16(m, e), x34 = sub16(t1, e2);
				sub16_into_hi(x12, h1, f);
				sub16_into_hi(x34, t2, f2);
				dz12 = __builtin_amdgcn_bitop3_b32((int)((unsigned)dz12 >> 1), x12, (int)0x80008000u, 0xf8); // a | (b & c)
				dz34 = __builtin_amdgcn_bitop3_b32((int)((unsigned)dz34 >> 1), x34, (int)0x80008000u, 0xf8);
				if constexpr (decltype(MASKED)::value) {
					const int actv = (am << (31 - s)) >> 31;
					f = sel3n(actv, max16(f2, t2), kNeg16);
					R[s] = (int)__builtin_amdgcn_perm((unsigned)sel3n(actv, max16(e2, t1), kNeg16), (unsigned)sel3n(actv, h, fill), 0x05040100u);
				} else {
					f = max16(f2, t2);
					int r = h;
					max16_into_hi(r, e2, t1);
					R[s] = r;
				}
				if ((s & 7) == 7 || s == NS - 1) {
					// n cells went through the shift registers: eight would leave b1 / b2 in bytes 1 / 3 of dz12 and b3 / b4 there in dz34
					const int n = (s & 7) + 1;
					dzw[s >> 3] = (uint32_t)dz12 >> (16 - n) | (uint32_t)dz34 >> (8 - n); // bytes b1 b3 b2 b4, cell c at bit c
				}
			}
		};
		if (masked) cells(std::true_type{});
		else cells(std::false_type{});
		if (mine && want) { // ksw.c:561 (row i < rows_cap: the caller refuses longer targets): wave-uniform line address in SGPRs + the lane's byte offset
#pragma unroll
			for (int b = 0; b < NB; ++b) {
				const uint32_t *line = zbase + ((size_t)b * (size_t)rows_cap + (size_t)i) * 64;
				asm volatile("global_store_dword %0, %1, %2" : : "v"(lane * 4), "v"(dzw[b]), "s"(line) : "memory");
			}
		}
		// score = eh[qlen].h after the LAST row of a lane = H(tlen-1, qlen-1), ksw.c:565: slot qlen-tlen+W of that row, if it is a slot
		if (__builtin_amdgcn_ballot_w64(mine && i == tlen - 1)) {
			const int ss = qlen - tlen + W;
			int pick = kNeg16;
#pragma unroll
			for (int s = 0; s < NS; ++s) pick = ss == s ? R[s] : pick;
			if (mine && i == tlen - 1) score = (int)(int16_t)(pick & 0xffff);
		}
		// slide the query window by one base (row i+1 looks at q[i+1-W+s])
#pragma unroll
		for (int v = 0; v + 1 < NQ; ++v) QW[v] = (int)__builtin_amdgcn_alignbyte((unsigned)QW[v + 1], (unsigned)QW[v], 1u);
		QW[NQ - 1] = (int)__builtin_amdgcn_alignbyte((unsigned)qin, (unsigned)QW[NQ - 1], 1u);
	}
	return score;
}

} // namespace

#ifndef BMH_GN_WAVES_LO
#define BMH_GN_WAVES_LO 8 /* bands 0..3 */
#endif
#ifndef BMH_GN_WAVES_HI
#define BMH_GN_WAVES_HI 6 /* bands 4..7: at eight, 64 registers, the row loop of W = 6, 7 goes through scratch */
#endif

// WLO = 0: the bands 0..3 (bin 6); WLO = 4: the bands 4..7 (bin 7)
template <int WLO, bool SYM>
__global__ __launch_bounds__(64, (WLO == 0 ? BMH_GN_WAVES_LO : BMH_GN_WAVES_HI)) void global_narrow_kernel(
    const uint8_t *__restrict__ pool, const bmh_glb_task_t *__restrict__ tasks, const uint32_t *__restrict__ order,
    const uint8_t *__restrict__ band, const uint32_t *__restrict__ count, long long n, bmh_glb_result_t *__restrict__ out,
    uint32_t *__restrict__ cigar_pool, DevParams P, uint32_t *__restrict__ zslab, int rows_cap, int *__restrict__ err_flag)
{
	__shared__ uint2 srow[8];
	__shared__ __attribute__((aligned(16))) uint8_t lds[kStreamRows * 64]; // the per-row stream, then the traceback's strip (kTbRows x 64 dwords)
	static_assert(kStreamRows * 64 == kTbRows * 64 * 4, "one LDS area serves both");
	const int lane = threadIdx.x;
	if (lane < 5) {
		uint32_t lo = 0;
		for (int q = 0; q < 4; ++q) lo |= (uint32_t)(uint8_t)mat_at(P, lane * 5 + q) << (8 * q);
		srow[lane] = make_uint2(lo, (uint32_t)(uint8_t)mat_at(P, lane * 5 + 4));
	}
	const long long cnt = count ? (long long)*count : n;
	uint32_t *__restrict__ zbase = zslab + (size_t)blockIdx.x * (size_t)rows_cap * (size_t)(kNarrowBlocks * 64); // this wave's direction slab

	for (long long base = (long long)blockIdx.x * 64; base < cnt; base += (long long)gridDim.x * 64) {
		const bool valid = base + lane < cnt;
		const long long pos = cnt - 1 - (valid ? base + lane : base); // sorted ascending by band, then rows: widest and longest first
		const uint32_t idx = order ? order[pos] : (uint32_t)pos;
		const uint4 tb = ((const uint4 *)(tasks + idx))[1];
		const int qlen = (int)(tb.x & 0xffff), tlen = (int)(tb.x >> 16);
		const int w = band ? (int)band[pos] : (int)tb.y;
		const bool want = (int)tb.w > 0;
		const bool bad = w < WLO || w > WLO + 3 || tlen > rows_cap;
		if (valid && bad) {
			out[idx].score = INT32_MIN, out[idx].n_cigar = 0;
			atomicExch(err_flag, BMH_E_RANGE);
		}
		const bool live = valid && !bad;

		// ---- the rows: one pass per distinct band among the live lanes (one pass, except in a wave at the seam of two bands)
		int score = kNeg16;
		for (unsigned long long todo = __builtin_amdgcn_ballot_w64(live); todo != 0;) {
			const int wc = __builtin_amdgcn_readlane(w, (int)__builtin_ctzll(todo));
			const bool mine = live && w == wc;
			int sc = kNeg16;
#define BMH_GN_CASE(WW)                                                                                                \
	case WW:                                                                                                           \
		sc = narrow_rows<WW, SYM>(mine, want, qlen, tlen, idx, pool, tasks, P, srow, lds, zbase, rows_cap);            \
		break;
			switch (wc) {
				BMH_GN_CASE(WLO)
				BMH_GN_CASE(WLO + 1)
				BMH_GN_CASE(WLO + 2)
				BMH_GN_CASE(WLO + 3)
			}
#undef BMH_GN_CASE
			if (mine) score = sc;
			todo &= ~__builtin_amdgcn_ballot_w64(mine);
		}
		if (tlen == 0) score = qlen == 0 ? 0 : (qlen <= w ? -(P.o_ins + P.e_ins * qlen) : kNeg16); // eh[qlen].h of ksw.c:519-522
		// No cell written (the band does not reach the last cell, or tlen == 0 with qlen > w): score is still kNeg16, the reference's
		// MINUS_INF.  A real score of an admitted task is above -kGlbLaneWorst (glb_lane_domain), so the test is exact.
		if (score <= -kGlbLaneWorst) score = -0x40000000;

		// ---- traceback, ksw.c:566-581, one path per lane: global_lane_kernel's, every lane on its own band
		const uint2 tc = *(const uint2 *)((const uint8_t *)(tasks + idx) + 24); // {cigar_off, cigar_cap}
		const uint32_t cigar_off = tc.x;
		const int cigar_cap = (int)tc.y;
		int n_cigar = 0;
		if (__builtin_amdgcn_ballot_w64(live && want)) {
			__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); // direction words of this wave are in flight
			uint32_t *cg = cigar_pool + cigar_off;
			int ti = tlen - 1, tk = min(qlen, tlen - 1 + w + 1) - 1, which = 0, last_op = 0, last_len = 0, nw = 0;
			const bool on = live && want;
			uint32_t *strip = (uint32_t *)lds;
			int cblk = -1, ctop = -1; // block and top row of this lane's strip: rows (ctop - kTbRows, ctop]
			while (__builtin_amdgcn_ballot_w64(on && ti >= 0 && tk >= 0)) {
				const bool act = on && ti >= 0 && tk >= 0;
				const int s = min(max(tk - (ti - w), 0), 2 * w);
				if (__builtin_amdgcn_ballot_w64(act && ((s >> 3) != cblk || ti > ctop || ti <= ctop - kTbRows))) {
					if (act) {
						cblk = s >> 3, ctop = ti;
						const uint32_t *src = zbase + ((size_t)cblk * (size_t)rows_cap) * 64 + lane;
						// (in two halves, eight loads in flight: sixteen destinations and their addresses do not fit beside the
						// task's state in the 64 registers of eight waves per SIMD)
#pragma unroll 1
						for (int k0 = 0; k0 < kTbRows; k0 += kTbRows / 2) {
							uint32_t v[kTbRows / 2];
#pragma unroll
							for (int k = 0; k < kTbRows / 2; ++k) v[k] = ti - k0 - k >= 0 ? src[(size_t)(ti - k0 - k) * 64] : 0u;
#pragma unroll
							for (int k = 0; k < kTbRows / 2; ++k) strip[(k0 + k) * 64 + lane] = v[k];
						}
					}
				}
				if (act) {
					const uint32_t dzw = strip[(ctop - ti) * 64 + lane] >> (s & 7);
					// bit 0 = [m < e], bit 16 = [max(m,e) < f], bit 8 = E continues, bit 24 = F continues (see the fill)
					which = which == 0 ? ((dzw >> 16 & 1) ? 2 : (int)(dzw & 1)) : which == 1 ? (int)(dzw >> 8 & 1) : (int)(dzw >> 23 & 2);
					const int op = which == 0 ? 0 : (which == 1 ? 2 : 1);
					if (last_len > 0 && op == last_op) ++last_len; // ksw.c:489-499
					else {
						if (last_len > 0) {
							if (nw < cigar_cap) cg[cigar_cap - 1 - nw] = (uint32_t)last_len << 4 | (uint32_t)last_op;
							++nw;
						}
						last_op = op, last_len = 1;
					}
					ti -= which != 2;
					tk -= which != 1;
				}
			}
			if (on) {
				for (int pass = 0; pass < 2; ++pass) { // leftovers, ksw.c:576-577: deletions then insertions
					const int op = pass == 0 ? 2 : 1, len = pass == 0 ? ti + 1 : tk + 1;
					if (len <= 0) continue;
					if (last_len > 0 && op == last_op) last_len += len;
					else {
						if (last_len > 0) {
							if (nw < cigar_cap) cg[cigar_cap - 1 - nw] = (uint32_t)last_len << 4 | (uint32_t)last_op;
							++nw;
						}
						last_op = op, last_len = len;
					}
				}
				if (last_len > 0) {
					if (nw < cigar_cap) cg[cigar_cap - 1 - nw] = (uint32_t)last_len << 4 | (uint32_t)last_op;
					++nw;
				}
				n_cigar = nw;
				// the words sit at [cap-n, cap) in forward order; move them to [0, n)
				const int shift = cigar_cap - nw;
				if (shift > 0 && nw <= cigar_cap) {
					__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
					for (int c = 0; c < nw; ++c) cg[c] = cg[shift + c];
				}
				if (nw > cigar_cap) atomicExch(err_flag, BMH_E_CIGAR_CAP);
			}
		}
		if (live) out[idx].score = score, out[idx].n_cigar = n_cigar;
	}
}

// ---- launcher: tasks listed in d_order[0..*d_count) must have a band (d_band, or their own w) of wlo..wlo+3, wlo 0 or 4, and tlen <= rows_cap
int launch_global_narrow(bmh_ctx *ctx, int wlo, const uint8_t *d_pool, const bmh_glb_task_t *d_tasks, int64_t n, bmh_glb_result_t *d_res,
                         uint32_t *d_cigar, const uint32_t *d_order, const uint32_t *d_count, int rows_cap, const uint8_t *d_band)
{
	if (n <= 0) return BMH_OK;
	// persistent grid = the waves resident at once, each with a direction slab of its own in d_zslab (see launch_global_lane, with
	// which the slab is shared: the lane launches of a global launch run back to back on the stream)
	if (wlo != 0 && wlo != 4) return BMH_E_ARG;
	const long long grid = std::min<long long>((n + 63) / 64, (long long)ctx->ncu * 4 * (wlo == 0 ? BMH_GN_WAVES_LO : BMH_GN_WAVES_HI));
	int rc = ensure(ctx, ctx->d_zslab, (size_t)grid * (size_t)rows_cap * (size_t)kNarrowBlocks * 64 * 4);
	if (rc) return rc;
	const bool sym = ctx->dev.o_del + ctx->dev.e_del == ctx->dev.o_ins + ctx->dev.e_ins;
#define BMH_LAUNCH_GN(WW, SS)                                                                                                   \
	hipLaunchKernelGGL((global_narrow_kernel<WW, SS>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, d_pool, d_tasks, d_order, d_band, \
	                   d_count, (long long)n, d_res, d_cigar, ctx->dev, (uint32_t *)ctx->d_zslab.p, rows_cap, ctx->d_err)
	if (wlo == 0 && sym) BMH_LAUNCH_GN(0, true);
	else if (wlo == 0) BMH_LAUNCH_GN(0, false);
	else if (sym) BMH_LAUNCH_GN(4, true);
	else BMH_LAUNCH_GN(4, false);
#undef BMH_LAUNCH_GN
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

} // namespace bmh
