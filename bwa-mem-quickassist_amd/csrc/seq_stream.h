// seq_stream.h -- the lane kernels' refill of their per-row sequence stream: N dwords = the 4N positions [p0, p0 + 4N) of a task's
// sequence, a position outside [0, len) reading as base 4 (host/seqstream_core.h has the addresses and the assembly, and the test).
//
// A kernel ISSUES a batch -- every load of it unconditional, from an address clamped into the sequence, no branch between two of
// them: loads under a test of their own are compiled into a basic block and an `s_waitcnt vmcnt` each, one dependent round trip per
// load, and on gfx950 that counter also holds the direction-word stores in flight -- then FINISHES it once, after the one wait: the
// bytes that were not asked for are shifted out and replaced.  Several sequences' batches may be issued before the first is finished.
// A sequence shorter than a dword (rare: 1..3 bases) has its own bytes loaded instead, under one test for the batch.
#ifndef BMH_SEQ_STREAM_H
#define BMH_SEQ_STREAM_H

#include <stdint.h>

#include "../host/seqstream_core.h"

namespace bmh {

// the lowest address of a sequence whose position 0 is pool[off]: reversed ones run downwards from there
__device__ __forceinline__ uint64_t seq_lo(uint64_t off, int len, bool rev) { return rev ? off - (uint64_t)(len > 0 ? len - 1 : 0) : off; }

// d[0..N) <- what seq_finish() needs for positions [p0, p0 + 4N) of the sequence at lo; a lane with !on loads nothing
template <int N>
__device__ __forceinline__ void seq_issue(uint32_t (&d)[N], const uint8_t *__restrict__ pool, uint64_t lo, int len, int p0, bool rev, bool on)
{
	const uint8_t *s = pool + lo;
#pragma unroll
	for (int v = 0; v < N; ++v) d[v] = 0;
	if (on && len >= 4) {
#pragma unroll
		for (int v = 0; v < N; ++v) __builtin_memcpy(&d[v], s + bmh_seqs_dword_at(bmh_seqs_mem_pos(p0 + 4 * v, len, rev), len), 4);
	} else if (on && len > 0) {
		const uint32_t b0 = s[0], b1 = s[bmh_seqs_small_at(1, len)], b2 = s[bmh_seqs_small_at(2, len)];
#pragma unroll
		for (int v = 0; v < N; ++v) d[v] = b0 | b1 << 8 | b2 << 16;
	}
}

// d[v] <- the bytes of positions [p0 + 4v, p0 + 4v + 4), with the arguments seq_issue() had
template <int N>
__device__ __forceinline__ void seq_finish(uint32_t (&d)[N], int len, int p0, bool rev, bool on)
{
	len = on ? len : 0;
#pragma unroll
	for (int v = 0; v < N; ++v) {
		const int m = bmh_seqs_mem_pos(p0 + 4 * v, len, rev);
		d[v] = bmh_seqs_assemble(d[v], bmh_seqs_dword_at(m, len), m, len, rev);
	}
}

// ---- the global lane kernels' stream (global_lane.hip, global_narrow.hip): rows [r0, r0 + ROWS) of a lane, one byte per row at
// strm[row * 64 + lane]: low nibble the target base t[r], high nibble the query base q[r + qsh] that enters the window's top slot
// after row r.  B dwords of each sequence per batch: ROWS / (4 B) batches, one wait each.
template <int ROWS, int B>
__device__ __forceinline__ void glb_fill_stream(uint8_t *strm, int lane, const uint8_t *__restrict__ pool, uint64_t t_off, int tlen,
                                                uint64_t q_off, int qlen, int r0, int qsh, bool on)
{
	static_assert(ROWS % (4 * B) == 0, "whole batches");
	// what the batches derive from the two lengths is made here, once per refill: hoisted out of the caller's row loop by the compiler,
	// it is a dozen registers held, or spilled, across that loop
	asm volatile("" : "+v"(tlen), "+v"(qlen));
#pragma unroll 1
	for (int rb = 0; rb < ROWS; rb += 4 * B) {
		uint32_t t[B], q[B];
		seq_issue<B>(t, pool, t_off, tlen, r0 + rb, false, on);
		seq_issue<B>(q, pool, q_off, qlen, r0 + rb + qsh, false, on);
		seq_finish<B>(t, tlen, r0 + rb, false, on);
		seq_finish<B>(q, qlen, r0 + rb + qsh, false, on);
#pragma unroll
		for (int v = 0; v < B; ++v) {
			const uint32_t m4 = (t[v] & 0x0f0f0f0fu) | (q[v] & 0x0f0f0f0fu) << 4;
#pragma unroll
			for (int k = 0; k < 4; ++k) strm[(rb + 4 * v + k) * 64 + lane] = (uint8_t)(m4 >> (8 * k));
		}
	}
}

} // namespace bmh

#endif
