// wave_ticket.h -- the in-launch hand-off of table_plan_kernel (chain2reg.hip) and mt_filter_kernel (matesw.hip): every block is one
// wave, lane 0 of each publishes the wave's part of W 64-bit words and draws a ticket, and the wave that draws the last one reads
// every block's part.  Packing the fields into words and merging the parts stay with the caller.
//
// The parts cross compute units and dies inside one launch, where no cache of one unit is refreshed by another's stores.  So they
// are written through with agent-scope stores and released by the fence before the ticket, and read with agent-scope loads behind
// the acquire that follows the ticket -- never from a cache line this unit may hold.  The s_waitcnt stands between the fence and
// the ticket's atomic, in that order: the part has left this wave before the ticket is drawn, whatever the toolchain makes of the
// fence's own wait (the in-launch reduction recipe of the CDNA programming guide, its guideline on inter-workgroup communication:
// keep the second wait, fence first, always).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmh {

// Every lane of the block's one wave calls it; lane 0's w is what is published, at part[STRIDE * blockIdx.x].  *ticket: zeroed by the
// host ahead of the launch.  True in every lane of the last wave to arrive, which may then read the parts with wave_ticket_word.
template <int W, int STRIDE>
__device__ __forceinline__ bool wave_ticket_publish(long long *part, const long long (&w)[W], uint32_t *ticket)
{
	static_assert(W <= STRIDE, "a part lies inside its stride");
	uint32_t drawn = 0;
	if (threadIdx.x == 0) {
		long long *dst = part + STRIDE * (size_t)blockIdx.x;
#pragma unroll
		for (int i = 0; i < W; ++i) __hip_atomic_store(dst + i, w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__threadfence();
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		drawn = atomicAdd(ticket, 1u);
	}
	drawn = (uint32_t)__shfl((int)drawn, 0);
	if (drawn != gridDim.x - 1) return false;
	__threadfence();
	return true;
}

// word i of block b's part, for the last wave
template <int STRIDE>
__device__ __forceinline__ long long wave_ticket_word(const long long *part, unsigned b, int i)
{
	return __hip_atomic_load(part + STRIDE * (size_t)b + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace bmh
