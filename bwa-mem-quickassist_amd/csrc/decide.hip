// decide.hip -- pass A of phase 2 on the device: primary marking, pairing, the tail of mem_sam_pe, the selection of mem_reg2sam_se
// and mem_approx_mapq_se of every region (reference bwamem.c:445-475, :1023-1062, bwamem_pair.c:177-331), behind
// bmh_decide_device (api.hip).  The rules are the text of host/postproc_core.h, which gcc compiles for bmh_decide_batch: the two
// give the same bytes.
//   decide_kernel   one lane per read (single-end) or per pair, 64-lane blocks.  The lane sorts its regions in place in the arena
//                   (the 64-byte records themselves move, as in region_dedup_kernel), keeps the z[] list of the marking and the
//                   v[] keys of the pairing in two scratch arrays addressed by the same offsets as the regions, and its range
//                   stack in its own 34 entries.  Outputs go to the regions' offsets.
// log and erfc do not run here: the lane reads log(k) and mem_pair's insert-size term from tables the host made with its libm
// (postproc_core.h says why), and the core's multiply-add pairs are compiled without contraction.
#include "decide.h"

namespace bmh {

// bmh_sort_stack_len(n) <= 34 entries for n < 2^32
constexpr int kDecideStk = 34;

__global__ __launch_bounds__(64) void decide_kernel(DecideArgs A)
{
	const int u = blockIdx.x * blockDim.x + threadIdx.x;
	if (u >= (A.pe ? A.n >> 1 : A.n)) return;
	bmh_sort_stk_t stk[kDecideStk];
	const bmh_sam_opt_t *o = &A.hdr->opt;
	if (!A.pe) {
		const unsigned long long o0 = A.roff[u], o1 = A.roff[u + 1];
		if (o0 > o1 || o1 > A.total || o1 - o0 > 0x7fffffffull) { atomicCAS(A.err, 0, BMH_E_ARG); return; }
		bmh_pp_unit_se(o, &A.tab, A.id0 + u, (int)(o1 - o0), A.reg + o0, A.z + o0, stk, A.reg_mapq + o0, &A.n_want[u], A.want_k + o0);
		return;
	}
	const unsigned long long o0 = A.roff[2 * u], o1 = A.roff[2 * u + 1], o2 = A.roff[2 * u + 2];
	if (o0 > o1 || o1 > o2 || o2 > A.total || o2 - o0 > 0x7fffffffull) { atomicCAS(A.err, 0, BMH_E_ARG); return; }
	const int n[2] = {(int)(o1 - o0), (int)(o2 - o1)};
	bmh_alnreg_t *const a[2] = {A.reg + o0, A.reg + o1};
	int *const z[2] = {A.z + o0, A.z + o1};
	int32_t *const mq[2] = {A.reg_mapq + o0, A.reg_mapq + o1};
	int32_t *const wk[2] = {A.want_k + o0, A.want_k + o1};
	bmh_pp_unit_pe(o, A.l_pac, A.hdr->pes, &A.tab, (uint64_t)(A.id0 >> 1) + (uint64_t)u, n, a, z, A.v + o0, stk, &A.pd[u], mq, &A.n_want[2 * u], wk);
}

int launch_decide(bmh_ctx *ctx, const DecideArgs &A)
{
	const int units = A.pe ? A.n >> 1 : A.n;
	if (units <= 0) return BMH_OK;
	if (ctx->timing) {
		if (!ctx->ev_decide[0]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_decide[0]));
		if (!ctx->ev_decide[1]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_decide[1]));
		BMH_HIP(ctx, hipEventRecord(ctx->ev_decide[0], ctx->stream));
	}
	hipLaunchKernelGGL(decide_kernel, dim3((unsigned)((units + 63) / 64)), dim3(64), 0, ctx->stream, A);
	BMH_HIP(ctx, hipGetLastError());
	if (ctx->timing) BMH_HIP(ctx, hipEventRecord(ctx->ev_decide[1], ctx->stream));
	return BMH_OK;
}

} // namespace bmh
