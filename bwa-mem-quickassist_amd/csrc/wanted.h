// wanted.h -- what api.hip hands wanted.hip (bmh_wanted_cigar_device): the records of one call's device block and the kernels' arguments.
#pragma once
#include "bmh_ctx.h"
#include "../host/regplan_core.h"

namespace bmh {

struct WantedHdr { // the upload's parameter block
	bmh_rp_opt_t opt;
	int32_t fix_w; // opt->w: the band of bwa_fix_xref2's single alignment (bwa.c:198)
};

// one wanted region, number j in want order, as the planning leaves it (it stays on the device: wanted_result_kernel reads it)
enum { kWantOk = 0, kWantBad = 1, kWantHost = 2 }; // refused (the call ends in an error); its fix outgrew the slot: the host redoes it
struct WantRec { // 80 bytes
	int64_t rb, re; // after bwa_fix_xref2
	int32_t qb, qe;
	int32_t read, k;
	int32_t truesc, reg_w;
	int64_t cb, ce; // the interval a region to fix is cut to
	int32_t band[3];
	int32_t state;
	int32_t v;      // its record in the main round, -1 = none
	uint32_t flags; // BMH_WANTED_MOVED
};

// the only thing the host reads between launches: one per round (0: the regions to fix, 1: every region)
struct WantedStatus { // 64 bytes
	int32_t n_w, n_rec, n_tasks, err; // wanted regions, this round's records and tasks, the first error (also in the context's word)
	int32_t qmax, tmax, wmax, wraw;   // validate_glb's GlbShape of the tasks up to kGlbLdsQcap query columns ...
	int32_t lqmax, ltmax, lwmax, ln;  // ... and of the longer ones, with their count
	unsigned long long opool, slots;  // bytes of oriented copies, CIGAR words of the tasks
};

struct WantedArgs {
	// inputs
	const unsigned long long *roff, *seq_off; // n + 1 each
	const WantedHdr *hdr;
	const int32_t *n_want, *want_k;           // n; total, at roff
	const bmh_alnreg_t *reg;                  // the arena
	unsigned long long total, reads_bytes;    // its records; bytes of the reads pool
	const bmh_refspan_t *ref;                 // the resident sequence table
	int32_t n_seqs, n;
	int64_t l_pac;
	// work and outputs
	unsigned long long *first;                // n + 1: wanted regions before read i
	WantRec *rec;                             // w_cap
	uint32_t *key[4];                         // w_cap each: what the one-block scan sums (records, oriented bytes, tasks, CIGAR words)
	unsigned long long *sum[4];               // ... and its exclusive sums
	bmh_region_req_t *req[2];                 // w_cap each: the rounds' records
	bmh_glb_task_t *task[2];                  // w_cap; 3 * w_cap
	const bmh_region_res_t *fix_res;          // round 0's results, w_cap ...
	const uint32_t *fix_cig;                  // ... and CIGAR slots of BMH_RP_SMALL_CAP words
	const bmh_region_res_t *main_res;         // the main round's results, w_cap ...
	bmh_wanted_res_t *wres;                   // ... and the records wanted_result_kernel makes of them, w_cap
	WantedStatus *status;                     // 2
	unsigned long long w_cap, opool_cap;
	int *err;
};

// ---- the one-block scan of the planning kernels, also samtext.hip's (the sizes of a slice's reads)
constexpr int kScanThreads = 1024;

// Exclusive sums over the block of K values per thread, in thread order; total[] = the block's sums.  Wave scans by shuffle, the 16
// wave totals through LDS (s: 2 * K * 16 + K entries), two barriers and one behind for the next tile.
template <class T, int K> __device__ __forceinline__ void block_excl_scan(T *s, T v[K], T total[K])
{
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	constexpr int W = kScanThreads / 64;
	T inc[K];
	for (int c = 0; c < K; ++c) {
		T x = v[c];
		for (int d = 1; d < 64; d <<= 1) {
			const T y = __shfl_up(x, d);
			if (lane >= d) x += y;
		}
		inc[c] = x;
		if (lane == 63) s[c * W + wave] = x;
	}
	__syncthreads();
	if (wave == 0) {
		for (int c = 0; c < K; ++c) {
			const T w = lane < W ? s[c * W + lane] : 0;
			T x = w;
			for (int d = 1; d < W; d <<= 1) {
				const T y = __shfl_up(x, d);
				if (lane >= d) x += y;
			}
			if (lane < W) s[K * W + c * W + lane] = x - w;
			if (lane == W - 1) s[2 * K * W + c] = x;
		}
	}
	__syncthreads();
	for (int c = 0; c < K; ++c) {
		v[c] = inc[c] - v[c] + s[K * W + c * W + wave];
		total[c] = s[2 * K * W + c];
	}
	__syncthreads();
}

// first[] and the xref test; then round 0's plan.  Behind it status[0] is complete.
int launch_wanted_begin(bmh_ctx *ctx, const WantedArgs &A);
// the cut of the regions round 0 aligned, then every region's plan.  Behind it rec[] and status[1] are complete.
int launch_wanted_main(bmh_ctx *ctx, const WantedArgs &A);
// behind the main round's region kernels, in both forms of the session: wres[j] from rec[j] and its region result, so that rec[] stays
// on the device and the host downloads n_w records
int launch_wanted_results(bmh_ctx *ctx, const WantedArgs &A);

} // namespace bmh
