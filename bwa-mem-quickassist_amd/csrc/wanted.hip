// wanted.hip -- the planning of pass B of phase 2 on the device, behind bmh_wanted_cigar_device (api.hip): from the want list pass A
// left (n_want, want_k, the sorted regions) to the region records and global-alignment tasks that region_cigar.hip and
// launch_global consume, without a host pass over the list.  The rules -- bns_pos2rid, the test, walk and verdict of bwa_fix_xref2
// (reference bwa-0.7.8/bwa.c:179-222), infer_bw and the bands (bwamem.c:884-891, :1187-1191, bwa.c:116-125), one region's record and
// tasks -- are the text of host/regplan_core.h, which gcc compiles for bmh_wanted_cigar_batch: the two give the same bytes.
//
//   wanted_first_kernel  one block: checks every read's offsets and counts, first[] = exclusive sums of n_want (wanted region j of the
//                        call is first[i] + q: the order pass C indexes by)
//   wanted_xref_kernel   one lane per wanted region: finds its read in first[], checks k and the coordinates, runs the xref test;
//                        a region that hangs over an end of its reference sequence gets round 0's keys
//   wanted_scan_kernel   one block: exclusive sums of the four keys (records, oriented bytes, tasks, CIGAR words) and their totals,
//                        in tiles of 1024 regions, one per lane (coalesced), the tile scanned by wave shuffles
//   wanted_emit_kernel   one lane per wanted region: its record and tasks at those sums; GlbShape of the tasks by atomicMax
//   wanted_cut_kernel    one lane per wanted region: walks round 0's CIGAR to the cut points and rewrites the coordinates
//                        (bwa.c:199-221), then plans the main round: bands and its keys
//   wanted_result_kernel one lane per wanted region, behind the main round's region kernels: its bmh_wanted_res_t from its WantRec
//                        and region result, cigar_off / md_off = its slot for the host's packing
// Offsets come from sums over the want order in one block each, never from atomicAdd: they do not depend on block scheduling.  Every
// dependency between blocks is a kernel boundary.  Nothing on the host has seen these records, so the kernels check what
// bmh_region_cigar_batch checks on the host; a refused region writes and addresses nothing, and the first error goes to the
// context's error word and the round's status by atomicCAS from 0 -- the host launches nothing behind a status with an error.
#include "wanted.h"

namespace bmh {

__device__ __forceinline__ void wanted_fail(const WantedArgs &A, int code)
{
	atomicCAS(A.err, 0, code);
	atomicCAS(&A.status[0].err, 0, code);
	atomicCAS(&A.status[1].err, 0, code);
}

// what read i contributes: its n_want, or 0 and an error where its offsets or its count are outside the arrays
__device__ __forceinline__ unsigned long long wanted_of_read(const WantedArgs &A, int i)
{
	const unsigned long long r0 = A.roff[i], r1 = A.roff[i + 1], s0 = A.seq_off[i], s1 = A.seq_off[i + 1];
	const int nw = A.n_want[i];
	if (r0 > r1 || r1 > A.total || r1 - r0 > 0x7fffffffull || s0 > s1 || s1 > A.reads_bytes || s1 - s0 > 0x7fffffffull || nw < 0 ||
	    (unsigned long long)nw > r1 - r0) {
		wanted_fail(A, BMH_E_ARG);
		return 0;
	}
	return (unsigned long long)nw;
}

__global__ __launch_bounds__(kScanThreads) void wanted_first_kernel(WantedArgs A)
{
	__shared__ unsigned long long s[2 * (kScanThreads / 64) + 1];
	const int t = threadIdx.x;
	unsigned long long carry = 0;
	for (int base = 0; base < A.n; base += kScanThreads) { // tiles of one read per lane: neighbouring lanes read neighbouring words
		const int i = base + t;
		unsigned long long v[1] = {i < A.n ? wanted_of_read(A, i) : 0}, total[1];
		block_excl_scan<unsigned long long, 1>(s, v, total);
		if (i < A.n) A.first[i] = carry + v[0];
		carry += total[0];
	}
	if (t == 0) {
		unsigned long long n_w = carry;
		if (n_w > A.w_cap) wanted_fail(A, BMH_E_ARG), n_w = 0; // more than the buffers were sized for: nothing is planned
		A.first[A.n] = carry;
		A.status[0].n_w = A.status[1].n_w = (int32_t)n_w;
	}
}

__global__ __launch_bounds__(256) void wanted_xref_kernel(WantedArgs A)
{
	const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= (unsigned long long)A.status[0].n_w) return;
	int lo = 0, hi = A.n - 1; // the read i with first[i] <= j < first[i + 1]
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (A.first[mid + 1] > j) hi = mid;
		else lo = mid + 1;
	}
	const int i = lo;
	const unsigned long long r0 = A.roff[i], nreg = A.roff[i + 1] - r0;
	const long long l_seq = (long long)(A.seq_off[i + 1] - A.seq_off[i]);
	const int k = A.want_k[r0 + (j - A.first[i])];
	WantRec x;
	x.rb = x.re = 0, x.qb = x.qe = 0, x.read = i, x.k = k, x.truesc = 0, x.reg_w = 0, x.cb = x.ce = 0;
	x.band[0] = x.band[1] = x.band[2] = -1, x.state = kWantBad, x.v = -1, x.flags = 0;
	A.key[0][j] = A.key[1][j] = A.key[2][j] = A.key[3][j] = 0;
	int code = 0;
	if (k < 0 || (unsigned long long)k >= nreg) code = BMH_E_ARG;
	else {
		const bmh_alnreg_t a = A.reg[r0 + (unsigned long long)k];
		x.rb = a.rb, x.re = a.re, x.qb = a.qb, x.qe = a.qe, x.truesc = a.truesc, x.reg_w = a.w;
		if (!(0 <= a.qb && a.qb < a.qe && a.qe <= l_seq)) code = BMH_E_ARG;
		else if (!(a.rb >= 0 && a.rb < a.re && a.re <= A.l_pac << 1)) code = BMH_E_ARG;
		else if (a.rb < A.l_pac && a.re > A.l_pac) code = BMH_E_ARG; // bridges the strands: the reference gives up on the run (bwamem.c:1183-1186)
		else if (a.qe - a.qb > 65535 || a.re - a.rb > 65535) code = BMH_E_RANGE;
	}
	if (code) {
		wanted_fail(A, code);
		A.rec[j] = x;
		return;
	}
	x.state = kWantOk;
	bmh_rp_refv_t rv;
	rv.off0 = &A.ref[0].offset, rv.len0 = &A.ref[0].len, rv.stride = sizeof(bmh_refspan_t), rv.n_seqs = A.n_seqs, rv.l_pac = A.l_pac;
	if (bmh_rp_xref_test(&rv, x.rb, x.re, &x.cb, &x.ce) > 0) { // round 0: one try with band opt->w (bwa.c:198)
		const int ql = x.qe - x.qb, tl = (int)(x.re - x.rb);
		bmh_rp_plan_t pl;
		bmh_rp_plan(&A.hdr->opt, ql, tl, INT32_MIN, A.hdr->fix_w, &pl);
		x.flags = BMH_WANTED_MOVED;
		A.key[0][j] = 1, A.key[1][j] = (uint32_t)(ql + tl), A.key[2][j] = (uint32_t)pl.n_tasks, A.key[3][j] = (uint32_t)pl.n_tasks * pl.cap;
	}
	A.rec[j] = x;
}

__global__ __launch_bounds__(kScanThreads) void wanted_scan_kernel(WantedArgs A, int round)
{
	__shared__ uint32_t s[2 * 4 * (kScanThreads / 64) + 4];
	const int t = threadIdx.x, m = A.status[round].n_w;
	unsigned long long carry[4] = {0, 0, 0, 0};
	for (int base = 0; base < m; base += kScanThreads) { // tiles of one region per lane; a tile's sums fit 32 bits (1024 x (ql + tl) at most)
		const int j = base + t;
		uint32_t v[4], total[4];
		for (int c = 0; c < 4; ++c) v[c] = j < m ? A.key[c][j] : 0;
		block_excl_scan<uint32_t, 4>(s, v, total);
		for (int c = 0; c < 4; ++c) {
			if (j < m) A.sum[c][j] = carry[c] + v[c];
			carry[c] += total[c];
		}
	}
	if (t == 0) {
		WantedStatus *st = &A.status[round];
		if (carry[1] > A.opool_cap || carry[2] > 0x7fffffffull || carry[3] > 0xffffffffull) wanted_fail(A, BMH_E_ARG); // (cannot happen: the host sized for it)
		st->n_rec = (int32_t)carry[0], st->opool = carry[1], st->n_tasks = (int32_t)carry[2], st->slots = carry[3];
	}
}

__global__ __launch_bounds__(256) void wanted_emit_kernel(WantedArgs A, int round)
{
	const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= (unsigned long long)A.status[round].n_w || A.key[0][j] == 0) return;
	WantRec x = A.rec[j];
	const int ql = x.qe - x.qb, tl = (int)(x.re - x.rb), truesc = round ? x.truesc : INT32_MIN;
	const unsigned long long v = A.sum[0][j], o_off = A.sum[1][j], task0 = A.sum[2][j], cig0 = A.sum[3][j];
	bmh_rp_plan_t pl;
	bmh_rp_plan(&A.hdr->opt, ql, tl, truesc, round ? x.reg_w : A.hdr->fix_w, &pl);
	if (v >= A.w_cap || o_off + (unsigned long long)(ql + tl) > A.opool_cap || task0 + (unsigned long long)pl.n_tasks > (round ? 3 : 1) * A.w_cap) {
		wanted_fail(A, BMH_E_ARG); // (cannot happen: the sums are of these very numbers)
		return;
	}
	bmh_glb_task_t *tk = A.task[round] + task0;
	bmh_rp_emit(&pl, A.seq_off[x.read] + (unsigned long long)x.qb, x.rb, o_off, ql, tl, truesc, (int64_t)task0, cig0, &A.req[round][v], tk);
	if (round) {
		x.v = (int32_t)v, x.band[0] = pl.band[0], x.band[1] = pl.band[1], x.band[2] = pl.band[2];
		A.rec[j] = x;
	}
	WantedStatus *st = &A.status[round];
	for (int t = 0; t < pl.n_tasks; ++t) { // validate_glb's shape (api.hip)
		const int w = tk[t].w, wq = w < ql ? w : ql;
		if (ql <= kGlbLdsQcap) atomicMax(&st->qmax, ql), atomicMax(&st->tmax, tl), atomicMax(&st->wmax, wq);
		else atomicMax(&st->lqmax, ql), atomicMax(&st->ltmax, tl), atomicMax(&st->lwmax, wq), atomicAdd(&st->ln, 1);
		atomicMax(&st->wraw, w);
	}
}

__global__ __launch_bounds__(256) void wanted_cut_kernel(WantedArgs A)
{
	const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= (unsigned long long)A.status[1].n_w) return;
	WantRec x = A.rec[j];
	const bool fix = A.key[0][j] != 0;
	const unsigned long long f = A.sum[0][j];
	A.key[0][j] = A.key[1][j] = A.key[2][j] = A.key[3][j] = 0;
	if (x.state != kWantOk) return;
	if (fix) {
		const bmh_region_res_t r = A.fix_res[f];
		if ((r.flags & BMH_REGION_CIGAR_CUT) || r.n_cigar > BMH_RP_SMALL_CAP || r.n_cigar < 0) { // the host redoes it, fix included
			x.state = kWantHost;
			A.rec[j] = x;
			return;
		}
		if (bmh_rp_xref_cut(r.n_cigar, A.fix_cig + f * BMH_RP_SMALL_CAP, x.cb, x.ce, &x.qb, &x.qe, &x.rb, &x.re)) {
			x.state = kWantBad; // bwa_fix_xref2 returns -2: the reference aborts
			A.rec[j] = x;
			wanted_fail(A, BMH_E_ARG);
			return;
		}
		A.rec[j] = x;
	}
	const int ql = x.qe - x.qb, tl = (int)(x.re - x.rb);
	bmh_rp_plan_t pl;
	bmh_rp_plan(&A.hdr->opt, ql, tl, x.truesc, x.reg_w, &pl);
	A.key[0][j] = 1, A.key[1][j] = (uint32_t)(ql + tl), A.key[2][j] = (uint32_t)pl.n_tasks, A.key[3][j] = (uint32_t)pl.n_tasks * pl.cap;
}

__global__ __launch_bounds__(256) void wanted_result_kernel(WantedArgs A)
{
	const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= (unsigned long long)A.status[1].n_w) return;
	const WantRec x = A.rec[j];
	bmh_wanted_res_t o;
	o.rb = x.rb, o.re = x.re, o.qb = x.qb, o.qe = x.qe; // as cut; a region whose fix the host redoes still has its own
	o.score = 0, o.n_cigar = 0, o.NM = 0, o.tries = 0, o.cigar_off = 0, o.md_off = 0, o.md_len = 0, o.flags = x.flags;
	o.band[0] = x.band[0], o.band[1] = x.band[1], o.band[2] = x.band[2], o.rsv_ = 0;
	if (x.state == kWantOk && x.v >= 0 && (unsigned long long)x.v < (unsigned long long)A.status[1].n_rec) {
		const bmh_region_res_t r = A.main_res[x.v];
		o.score = r.score, o.n_cigar = r.n_cigar, o.NM = r.NM, o.tries = r.tries, o.md_len = (uint32_t)r.md_len;
		o.cigar_off = o.md_off = (uint32_t)x.v;
		if (r.flags) o.flags |= BMH_WANTED_HOST;
	} else {
		o.flags |= BMH_WANTED_HOST;
		if (x.state != kWantHost) wanted_fail(A, BMH_E_ARG); // (cannot happen: a refused region has ended the session before)
	}
	A.wres[j] = o;
}

static int wanted_events(bmh_ctx *ctx, int k)
{
	if (!ctx->timing) return BMH_OK;
	if (!ctx->ev_wanted[k]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_wanted[k]));
	BMH_HIP(ctx, hipEventRecord(ctx->ev_wanted[k], ctx->stream));
	return BMH_OK;
}

int launch_wanted_begin(bmh_ctx *ctx, const WantedArgs &A)
{
	const unsigned blocks = (unsigned)((A.w_cap + 255) / 256);
	int rc;
	if (A.n <= 0 || A.w_cap == 0) return BMH_OK;
	if ((rc = wanted_events(ctx, 0))) return rc;
	hipLaunchKernelGGL(wanted_first_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, A);
	hipLaunchKernelGGL(wanted_xref_kernel, dim3(blocks), dim3(256), 0, ctx->stream, A);
	hipLaunchKernelGGL(wanted_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, A, 0);
	hipLaunchKernelGGL(wanted_emit_kernel, dim3(blocks), dim3(256), 0, ctx->stream, A, 0);
	BMH_HIP(ctx, hipGetLastError());
	return wanted_events(ctx, 1);
}

int launch_wanted_main(bmh_ctx *ctx, const WantedArgs &A)
{
	const unsigned blocks = (unsigned)((A.w_cap + 255) / 256);
	int rc;
	if (A.n <= 0 || A.w_cap == 0) return BMH_OK;
	if ((rc = wanted_events(ctx, 2))) return rc;
	hipLaunchKernelGGL(wanted_cut_kernel, dim3(blocks), dim3(256), 0, ctx->stream, A);
	hipLaunchKernelGGL(wanted_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, A, 1);
	hipLaunchKernelGGL(wanted_emit_kernel, dim3(blocks), dim3(256), 0, ctx->stream, A, 1);
	BMH_HIP(ctx, hipGetLastError());
	return wanted_events(ctx, 3);
}

int launch_wanted_results(bmh_ctx *ctx, const WantedArgs &A)
{
	if (A.n <= 0 || A.w_cap == 0) return BMH_OK;
	hipLaunchKernelGGL(wanted_result_kernel, dim3((unsigned)((A.w_cap + 255) / 256)), dim3(256), 0, ctx->stream, A);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

} // namespace bmh
