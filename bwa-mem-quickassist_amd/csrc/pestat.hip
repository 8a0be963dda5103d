// pestat.hip -- the pair walk of mem_pestat (reference bwa-0.7.8/bwamem_pair.c:46-72) on the device: for every pair the head regions
// of both mates, cal_sub over each mate's other regions, and the answer "no candidate" or (orientation, insert size) as one word.
// The rule is one text with the host's, host/pestat_core.h.  What mem_pestat does with the candidates (a counting sort, three
// percentiles, two ordered sums in double) stays on the host: bmh_pestat_from_candidates.
//
//   pestat_collect_kernel   one lane per pair.  Runs on region slices as mem_sort_and_dedup left them: behind region_dedup_kernel in
//                           the chains-to-regions driver (chain2reg.hip), where it can also apply mem_test_and_remove_exact
//                           (bwamem.c:438-443) first, and on a caller's vectors behind bmh_pestat_device (api.hip).
//                           No LDS, no cross-lane operation.
#include "bmh_ctx.h"
#include "bmh_device.h"
#include "../host/pestat_core.h"

namespace bmh {

static_assert(sizeof(bmh_alnreg_t) == 64, "pestat_collect_kernel moves a region as four uint4");

// mem_test_and_remove_exact on read r's slice; returns the count it leaves
__device__ __forceinline__ unsigned long long pestat_drop_exact(bmh_alnreg_t *a, unsigned long long n, int l_seq, int match, unsigned long long *cnt_r,
                                                                unsigned long long *gone)
{
	if (!bmh_ps_is_exact(a, (size_t)n, l_seq, match)) return n;
	uint4 *v = (uint4 *)a; // ascending, so a record is read before it is overwritten
	for (unsigned long long q = 0; q < (n - 1) * 4; ++q) v[q] = v[q + 4];
	*cnt_r = n - 1, ++*gone;
	return n - 1;
}

// Lane p owns reads 2p and 2p + 1 of n_reads (the last lane of an odd batch owns one read: it has no pair, only the drop-exact step).
// cand may be null (drop-exact alone), len and removed may be null without drop_exact.
__global__ __launch_bounds__(64) void pestat_collect_kernel(bmh_alnreg_t *reg, const unsigned long long *__restrict__ off, unsigned long long *cnt,
                                                            const int *__restrict__ len, int n_reads, unsigned long long total, bmh_sam_opt_t o,
                                                            int64_t l_pac, int match, int drop_exact, uint32_t *__restrict__ cand,
                                                            unsigned long long *removed, int *err)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	const size_t r0 = (size_t)p << 1, r1 = r0 + 1;
	if (r0 >= (size_t)n_reads) return;
	const bool pair = r1 < (size_t)n_reads;
	unsigned long long n0 = cnt[r0], n1 = pair ? cnt[r1] : 0;
	const unsigned long long at0 = off[r0], at1 = pair ? off[r1] : 0;
	if (n0 > 0x7fffffffull || at0 > total || n0 > total - at0 || n1 > 0x7fffffffull || at1 > total || n1 > total - at1) {
		atomicCAS(err, 0, BMH_E_ARG);
		return;
	}
	if (drop_exact) {
		unsigned long long gone = 0;
		n0 = pestat_drop_exact(reg + at0, n0, len[r0], match, &cnt[r0], &gone);
		if (pair) n1 = pestat_drop_exact(reg + at1, n1, len[r1], match, &cnt[r1], &gone);
		if (gone) atomicAdd(removed, gone);
	}
	if (pair && cand) cand[p] = bmh_ps_candidate(&o, l_pac, reg + at0, (size_t)n0, reg + at1, (size_t)n1);
}

int launch_pestat_collect(bmh_ctx *ctx, bmh_alnreg_t *d_reg, const unsigned long long *d_off, unsigned long long *d_cnt, const int *d_len,
                          int n_reads, unsigned long long total, const bmh_sam_opt_t &o, int64_t l_pac, int match, bool drop_exact, uint32_t *d_cand,
                          unsigned long long *d_removed, int *d_err)
{
	const int lanes = (n_reads + 1) / 2;
	if (lanes <= 0 || (!d_cand && !drop_exact)) return BMH_OK;
	if (ctx->timing) {
		if (!ctx->ev_pestat[0]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_pestat[0]));
		if (!ctx->ev_pestat[1]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_pestat[1]));
		BMH_HIP(ctx, hipEventRecord(ctx->ev_pestat[0], ctx->stream));
	}
	hipLaunchKernelGGL(pestat_collect_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, ctx->stream, d_reg, d_off, d_cnt, d_len, n_reads, total, o, l_pac,
	                   match, drop_exact ? 1 : 0, d_cand, d_removed, d_err);
	BMH_HIP(ctx, hipGetLastError());
	if (ctx->timing) BMH_HIP(ctx, hipEventRecord(ctx->ev_pestat[1], ctx->stream));
	return BMH_OK;
}

} // namespace bmh
