/*
 * seqstream_core.h -- where the lane kernels' sequence stream reads a task's bases and how it puts them together, as ONE text for the
 * device (csrc/seq_stream.h, hipcc) and for a C test program (tests/seqstream_core_main.c, gcc).
 *
 * A sequence is `len` bytes of the pool; position k is byte lo + k of a forward sequence and byte lo + len-1 - k of a reversed one
 * (lo is its lowest address: off, or off - (len-1) for the reversed forms of BMH_F_QREV / BMH_F_TREV).  A consumer asks for the four
 * positions [p, p+4) as one dword, byte k = position p + k, where a position outside [0, len) reads as base 4; p may be negative
 * (the query window left of column 0) or at and past len (the rows after the sequence's end).
 *
 *   len >= 4: ONE unaligned dword, from an address clamped into the sequence: bmh_seqs_dword_at() gives its byte index a in
 *             [0, len-4], bmh_seqs_assemble() shifts what was loaded to where it was asked for and sets the rest to 4.
 *   len <  4: the sequence's own one to three bytes, loaded once for any number of dwords (bmh_seqs_small_at(): byte indices clamped
 *             to len-1) and packed in memory order into a dword "loaded from index 0"; bmh_seqs_assemble() as above.  len == 0
 *             loads nothing, and whatever stands in for the dword is masked out.
 *
 * Neither reads a byte outside [lo, lo + len), so every load can be issued without a test of its own, a batch of them back to back
 * with one wait.  Plain C, no allocation; under hipcc __host__ __device__ and always inlined.
 */
#ifndef BMH_SEQSTREAM_CORE_H
#define BMH_SEQSTREAM_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define BMH_SQ_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_SQ_HD
#endif

#define BMH_SEQS_NONE 0x04040404u /* four times "no base" */

/* the first position in memory order of the four positions [p, p+4): p itself, or len-4-p where the sequence is stored reversed */
BMH_SQ_HD static inline int bmh_seqs_mem_pos(int p, int len, int rev) { return rev ? len - 4 - p : p; }

/* the byte index (from lo) of the dword that serves memory positions [m, m+4): clamped into [0, len-4]; 0 for len < 4 */
BMH_SQ_HD static inline int bmh_seqs_dword_at(int m, int len)
{
	const int hi = len > 4 ? len - 4 : 0;
	return m < 0 ? 0 : (m > hi ? hi : m);
}

/* 0 < len < 4: the byte index (from lo) of byte k = 0, 1, 2 of the packed dword */
BMH_SQ_HD static inline int bmh_seqs_small_at(int k, int len) { return k < len ? k : len - 1; }

/* dword d holds the bytes from index a = bmh_seqs_dword_at(m, len) on; the bytes of positions [p, p+4), m = bmh_seqs_mem_pos(p, len, rev) */
BMH_SQ_HD static inline uint32_t bmh_seqs_assemble(uint32_t d, int a, int m, int len, int rev)
{
	int sh = m - a; /* memory position m + k is byte k + sh of d */
	/* bytes [klo, khi) of the result are positions of the sequence: 0 <= m + k < len */
	const int klo = m >= 0 ? 0 : (m < -4 ? 4 : -m), khi = len - m >= 4 ? 4 : (len - m < 0 ? 0 : len - m);
	const uint32_t keep = khi > klo ? (0xffffffffu >> (8 * (4 - (khi - klo)))) << (8 * klo) : 0u;
	uint32_t v;
	sh = sh < -3 ? -3 : (sh > 3 ? 3 : sh); /* (beyond that nothing is kept) */
	v = sh >= 0 ? d >> (8 * sh) : d << (8 * -sh);
	v = (v & keep) | (BMH_SEQS_NONE & ~keep);
	if (rev) v = v >> 24 | (v >> 8 & 0xff00u) | (v << 8 & 0xff0000u) | v << 24;
	return v;
}

#endif
