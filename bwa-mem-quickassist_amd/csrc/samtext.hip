// samtext.hip -- pass C of phase 2 on the device, behind bmh_sam_text_device (api.hip): from the want list, the regions and pass B's
// records to SAM text.  The rules -- mem_reg2aln's second half, the mate records and flags of mem_sam_pe / mem_reg2sam_se, mem_aln2sam's
// columns (reference bwa-0.7.8/bwamem.c:904-1083, :1203-1235) -- are the text of host/samtext_core.h, which gcc compiles for
// bmh_sam_text_batch: the two give the same bytes.
//
//   samtext_size_kernel  one lane per unit (a read, or a pair): checks the unit's offsets, builds its records into alns[], applies the
//                        per-unit rule (plan[] per read) and runs the composer over the counting sink: size[i] = bytes of read i's lines
//   samtext_scan_kernel  one block: toff[] = exclusive 64-bit sums of size[], the total into the status word
//   samtext_emit_kernel  one lane per read: the same composer over the same records, writing into text[toff[i] .. toff[i+1])
// and, for the session that runs passes A, B and C without a host hop (bmh_phase2_text_device):
//   reads_gather_kernel       one wave per read: pass B's contiguous reads pool from the per-read pool that went up for pass C, or,
//                             through the same view, from the bases a parked session kept on the device
//   phase2_text_bind_kernel   one lane per wanted region: the record's slot number becomes the slot's address in pass B's CIGAR and MD
//                             slots, so that pass C reads them where the region kernels wrote them; the regions flagged
//                             BMH_WANTED_HOST are listed for the host and counted.  While that count is not zero the size and scan
//                             kernels leave at once: the host redoes the listed regions, phase2_text_patch_kernel puts their records
//                             in place, and size and scan run again
// The writing sink carries the size of the read's slice (samtext_core.h): a byte past it is not stored.  A slice that does not lie in
// the text buffer is not written at all.  Either raises the error words, and the host delivers nothing.  The emitter's stores are a
// byte stream per lane, 64 slices per wave: uncoalesced by nature.
// Nothing on the device trusts an offset it was handed: a unit whose offsets, counts, indices or pool record lie outside the uploaded
// arrays writes and addresses nothing, and the first error goes to the context's error word and the status by atomicCAS from 0 -- the
// host launches nothing behind a status with an error.
#include <algorithm>

#include "samtext.h"
#include "wanted.h"

namespace bmh {

__device__ __forceinline__ void samtext_fail(const SamtextArgs &A, int code)
{
	atomicCAS(A.err, 0, code);
	atomicCAS(&A.status->err, 0, code);
}

// read i as the composer sees it, from its record in the pool; false where the record does not lie in the pool.  With A.bases the
// record has no bases of its own: the view points at the read's in that pool, checked against soff[] and the pool's size as the record is
// against poff[] and rpool_bytes (the branch is uniform over the launch)
__device__ __forceinline__ bool samtext_read_view(const SamtextArgs &A, int i, bmh_st_read_t *v)
{
	const unsigned long long p0 = A.poff[i], p1 = A.poff[i + 1];
	const bool own = A.bases == nullptr;
	if (p0 > p1 || p1 > A.rpool_bytes || p1 - p0 < sizeof(SamtextRead) || (p0 & 7)) return false;
	const SamtextRead h = *(const SamtextRead *)(A.rpool + p0);
	if (h.l_name < 0 || h.l_seq < 0 || h.l_comment < -1) return false;
	if (samtext_read_bytes((size_t)h.l_name, (size_t)h.l_seq, h.has_qual != 0, h.l_comment, own) > p1 - p0) return false;
	const char *b = (const char *)(A.rpool + p0 + sizeof(SamtextRead));
	v->name = b, v->l_name = h.l_name, b += h.l_name;
	if (own) v->seq = (const uint8_t *)b, b += h.l_seq;
	else {
		const unsigned long long s0 = A.soff[i], s1 = A.soff[i + 1];
		if (s0 > s1 || s1 > A.bases_bytes || s1 - s0 != (unsigned long long)h.l_seq) return false;
		v->seq = A.bases + s0;
	}
	v->l_seq = h.l_seq;
	v->qual = h.has_qual ? b : nullptr, b += h.has_qual ? h.l_seq : 0;
	v->comment = h.l_comment >= 0 ? b : nullptr, v->l_comment = h.l_comment >= 0 ? h.l_comment : 0, v->rsv_ = 0;
	return true;
}

__device__ __forceinline__ void samtext_env(const SamtextArgs &A, bmh_st_env_t *E)
{
	E->names.pool = A.names, E->names.off = A.name_off, E->names.n_seqs = A.n_seqs, E->names.rsv_ = 0;
	E->cig = A.cig, E->md = A.md, E->rg_id = A.rg, E->l_rg = A.hdr->l_rg, E->rsv_ = 0;
}

// read i's offsets and counts against the arrays, then its records; false where something lies outside
__device__ __forceinline__ bool samtext_records(const SamtextArgs &A, const bmh_rp_refv_t &rv, int i, int l_seq)
{
	const int64_t r0 = A.roff[i], r1 = A.roff[i + 1], f0 = A.first[i], f1 = A.first[i + 1];
	if (r0 < 0 || r0 > r1 || (unsigned long long)r1 > A.total || f0 < 0 || f0 > f1 || (unsigned long long)f1 > A.n_w) return false;
	if (f1 - f0 != (int64_t)A.n_want[i] || f1 - f0 > r1 - r0) return false;
	for (int64_t q = f0; q < f1; ++q) {
		const int k = A.want_k[r0 + (q - f0)];
		if (k < 0 || (int64_t)k >= r1 - r0) return false;
		const bmh_wanted_res_t x = A.wr[q];
		if (x.n_cigar < 0 || (unsigned long long)x.cigar_off + (unsigned long long)x.n_cigar > A.cig_words) return false;
		if ((unsigned long long)x.md_off + (unsigned long long)x.md_len > A.md_bytes) return false;
		const bmh_alnreg_t ar = A.reg[r0 + k];
		bmh_st_aln_t a;
		if (bmh_st_record(&rv, &x, &ar, A.reg_mapq[r0 + k], l_seq, A.cig, &a)) return false;
		A.alns[q] = a;
	}
	return true;
}

__global__ __launch_bounds__(256) void samtext_size_kernel(SamtextArgs A)
{
	const int pe = A.pe != 0, nr = pe ? 2 : 1;
	const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (u * nr + nr > (long long)A.n) return;
	if (A.fused && A.fused->n_host) return; // the fused session: records are still the host's to make, the launch is repeated behind them
	const int i0 = (int)(u * nr);
	bmh_rp_refv_t rv;
	rv.off0 = &A.ref[0].offset, rv.len0 = &A.ref[0].len, rv.stride = sizeof(bmh_refspan_t), rv.n_seqs = A.n_seqs, rv.l_pac = A.l_pac;
	bmh_st_read_t rd[2];
	bool ok = true;
	for (int r = 0; r < nr; ++r) {
		A.size[i0 + r] = 0;
		ok = ok && samtext_read_view(A, i0 + r, &rd[r]) && samtext_records(A, rv, i0 + r, rd[r].l_seq);
	}
	if (!ok) {
		samtext_fail(A, BMH_E_ARG);
		return;
	}
	const int32_t *const wk[2] = {A.want_k + A.roff[i0], pe ? A.want_k + A.roff[i0 + 1] : nullptr};
	const bmh_alnreg_t *const ra[2] = {A.reg + A.roff[i0], pe ? A.reg + A.roff[i0 + 1] : nullptr};
	bmh_st_unit(A.hdr->opt_flag, A.l_pac, A.hdr->pes, pe, pe ? &A.pd[u] : nullptr, A.first + i0, wk, ra, A.alns, A.plan + i0);
	bmh_st_env_t E;
	samtext_env(A, &E);
	int lines = 0;
	for (int r = 0; r < nr; ++r) {
		const int i = i0 + r;
		bmh_st_sink_t t = {nullptr, 0, 0, 0, 0};
		lines += bmh_st_read_text(&E, &t, &rd[r], &A.plan[i], (int)(A.first[i + 1] - A.first[i]), A.alns + A.first[i]);
		if (t.err || t.l < 0) {
			samtext_fail(A, BMH_E_ARG);
			return;
		}
		A.size[i] = (unsigned long long)t.l;
	}
	if (A.fused) atomicAdd((unsigned long long *)&A.fused->lines, (unsigned long long)lines);
}

__global__ __launch_bounds__(kScanThreads) void samtext_scan_kernel(SamtextArgs A)
{
	__shared__ unsigned long long s[2 * (kScanThreads / 64) + 1];
	const int t = threadIdx.x;
	unsigned long long carry = 0;
	if (A.fused && A.fused->n_host) return; // (the whole block: see the size kernel)
	for (int base = 0; base < A.n; base += kScanThreads) { // tiles of one read per lane: neighbouring lanes read neighbouring words
		const int i = base + t;
		unsigned long long v[1] = {i < A.n ? A.size[i] : 0}, total[1];
		block_excl_scan<unsigned long long, 1>(s, v, total);
		if (i < A.n) A.toff[i] = carry + v[0];
		carry += total[0];
	}
	if (t == 0) {
		A.toff[A.n] = carry;
		A.status->total = (long long)carry;
	}
}

__global__ __launch_bounds__(256) void samtext_emit_kernel(SamtextArgs A)
{
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (long long)A.n) return;
	const unsigned long long o0 = A.toff[i], o1 = A.toff[i + 1];
	bmh_st_read_t rd;
	if (o0 > o1 || o1 > A.text_cap || o1 - o0 != A.size[i] || !samtext_read_view(A, (int)i, &rd)) { // a slice outside the buffer: nothing is written
		samtext_fail(A, BMH_E_ARG);
		return;
	}
	bmh_st_env_t E;
	samtext_env(A, &E);
	bmh_st_sink_t t = {A.text + o0, 0, (int64_t)(o1 - o0), 0, 0};
	bmh_st_read_text(&E, &t, &rd, &A.plan[i], (int)(A.first[i + 1] - A.first[i]), A.alns + A.first[i]);
	if (t.err || t.l != t.cap) samtext_fail(A, BMH_E_ARG); // (cannot happen: the records and the composer the size came from)
}

// ---- the fused session's joints (bmh_phase2_text_device)

// One wave per read, the lanes on neighbouring bytes: reads and writes coalesce whatever the read's alignment in either pool.
__global__ __launch_bounds__(256) void reads_gather_kernel(SamtextArgs A, const unsigned long long *seq_off, uint8_t *dst, unsigned long long reads_bytes)
{
	const int lane = threadIdx.x & 63;
	const long long waves = ((long long)gridDim.x * blockDim.x) >> 6;
	for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < (long long)A.n; i += waves) {
		const unsigned long long s0 = seq_off[i], s1 = seq_off[i + 1];
		bmh_st_read_t rd;
		if (!samtext_read_view(A, (int)i, &rd) || s0 > s1 || s1 > reads_bytes || s1 - s0 != (unsigned long long)rd.l_seq) { // nothing is copied
			if (lane == 0) samtext_fail(A, BMH_E_ARG);
			continue;
		}
		for (int b = lane; b < rd.l_seq; b += 64) dst[s0 + (unsigned long long)b] = rd.seq[b];
	}
}

__device__ __forceinline__ void bind_fail(const Phase2TextBindArgs &A)
{
	atomicCAS(A.err, 0, BMH_E_ARG);
	atomicCAS(&A.status_out->err, 0, BMH_E_ARG);
}

__global__ __launch_bounds__(256) void phase2_text_bind_kernel(Phase2TextBindArgs A)
{
	const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= (unsigned long long)A.status[1].n_w) return;
	bmh_wanted_res_t x = A.wres[j];
	if (!(x.flags & BMH_WANTED_HOST)) { // its slot's address: v * cap fits 32 bits for every v < w_cap (the host refuses the slice otherwise)
		const unsigned long long v = x.cigar_off;
		if (v >= A.w_cap) {
			bind_fail(A); // (cannot happen: wanted_result_kernel took v from the main round's records)
			return;
		}
		x.cigar_off = (uint32_t)(v * (unsigned long long)A.cig_cap), x.md_off = (uint32_t)(v * (unsigned long long)A.md_cap);
		A.wres[j] = x;
		return;
	}
	const WantRec r = A.rec[j];
	if (r.read < 0 || r.read >= A.n || r.k < 0) {
		bind_fail(A);
		return;
	}
	const unsigned long long r0 = A.roff[r.read], r1 = A.roff[r.read + 1];
	if (r0 > r1 || r1 > A.total || (unsigned long long)r.k >= r1 - r0) {
		bind_fail(A);
		return;
	}
	const unsigned long long at = (unsigned long long)atomicAdd(&A.fused->n_host, 1);
	if (at >= A.w_cap) return; // (cannot happen: one entry per wanted region at most)
	Phase2TextHost h;
	h.j = (int64_t)j, h.read = r.read, h.k = r.k, h.reg = A.reg[r0 + (unsigned long long)r.k];
	h.rb = x.rb, h.re = x.re, h.qb = x.qb, h.qe = x.qe, h.flags = x.flags, h.rsv = 0;
	A.list[at] = h;
}

__global__ __launch_bounds__(256) void phase2_text_patch_kernel(bmh_wanted_res_t *wres, const bmh_wanted_res_t *recs, const int64_t *at, long long m,
                                                                 long long n_w, SamtextStatus *status, int *err)
{
	const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= m) return;
	const int64_t j = at[t];
	if (j < 0 || j >= n_w) {
		atomicCAS(err, 0, BMH_E_ARG);
		atomicCAS(&status->err, 0, BMH_E_ARG);
		return;
	}
	wres[j] = recs[t];
}

int launch_reads_gather(bmh_ctx *ctx, const SamtextArgs &A, const unsigned long long *seq_off, uint8_t *dst, unsigned long long reads_bytes)
{
	if (A.n <= 0) return BMH_OK;
	if (ctx->timing) {
		if (!ctx->ev_gather[0]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_gather[0]));
		if (!ctx->ev_gather[1]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_gather[1]));
		BMH_HIP(ctx, hipEventRecord(ctx->ev_gather[0], ctx->stream));
	}
	const long long blocks = std::min<long long>(((long long)A.n + 3) / 4, 8192); // four reads per block; past that the waves stride
	hipLaunchKernelGGL(reads_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, A, seq_off, dst, reads_bytes);
	BMH_HIP(ctx, hipGetLastError());
	if (ctx->timing) BMH_HIP(ctx, hipEventRecord(ctx->ev_gather[1], ctx->stream));
	return BMH_OK;
}

int launch_phase2_text_bind(bmh_ctx *ctx, const Phase2TextBindArgs &A, int64_t n_w)
{
	if (n_w <= 0) return BMH_OK;
	hipLaunchKernelGGL(phase2_text_bind_kernel, dim3((unsigned)((n_w + 255) / 256)), dim3(256), 0, ctx->stream, A);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

int launch_phase2_text_patch(bmh_ctx *ctx, bmh_wanted_res_t *wres, const bmh_wanted_res_t *recs, const int64_t *at, int64_t m, int64_t n_w,
                             SamtextStatus *status, int *err)
{
	if (m <= 0) return BMH_OK;
	hipLaunchKernelGGL(phase2_text_patch_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, wres, recs, at, (long long)m, (long long)n_w,
	                   status, err);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

static int samtext_events(bmh_ctx *ctx, int k)
{
	if (!ctx->timing) return BMH_OK;
	if (!ctx->ev_samtext[k]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_samtext[k]));
	BMH_HIP(ctx, hipEventRecord(ctx->ev_samtext[k], ctx->stream));
	return BMH_OK;
}

int launch_samtext_size(bmh_ctx *ctx, const SamtextArgs &A)
{
	int rc;
	if (A.n <= 0) return BMH_OK;
	const long long units = A.pe ? A.n >> 1 : A.n;
	if ((rc = samtext_events(ctx, 0))) return rc;
	hipLaunchKernelGGL(samtext_size_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, ctx->stream, A);
	if ((rc = samtext_events(ctx, 1))) return rc;
	hipLaunchKernelGGL(samtext_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, A);
	BMH_HIP(ctx, hipGetLastError());
	return BMH_OK;
}

int launch_samtext_emit(bmh_ctx *ctx, const SamtextArgs &A)
{
	int rc;
	if (A.n <= 0) return BMH_OK;
	if ((rc = samtext_events(ctx, 2))) return rc;
	hipLaunchKernelGGL(samtext_emit_kernel, dim3((unsigned)((A.n + 255) / 256)), dim3(256), 0, ctx->stream, A);
	BMH_HIP(ctx, hipGetLastError());
	return samtext_events(ctx, 3);
}

} // namespace bmh
