/*
 * seqstream_core_main.c -- stand-alone check of host/seqstream_core.h for a plain and a sanitizer build: the dwords the lane kernels'
 * stream refill (csrc/seq_stream.h) puts together, against a byte-by-byte restatement.  Every sequence ends where its heap block ends
 * (the block is `align` + len bytes, the sequence its last len: every start alignment 0..15, and alignment 0 is a block of exactly
 * len), so a build under -fsanitize=address,undefined sees a read past the end; and load() itself refuses any index outside
 * [0, len) before it reads, which also covers the bytes in front of an unaligned start.
 *
 * Covered: len 0..200; forward and reversed; every dword position p in [-72, 288) -- which holds the rows [r0, r0 + 64) of
 * r0 = 0, 64, 128, 192, the same shifted by the query shifts 1..16, and the query windows that start up to 64 columns left of
 * column 0.  Prints "ok <dwords checked> <loads>"; exit status 1 on a wrong dword, 2 on a load outside the sequence.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/seqstream_core.h"

static unsigned long long n_loads;

static uint32_t load(const uint8_t *seq, int len, int at, int bytes)
{
	uint32_t d = 0;
	if (at < 0 || at + bytes > len) {
		fprintf(stderr, "load of %d bytes at %d outside a sequence of %d\n", bytes, at, len);
		exit(2);
	}
	memcpy(&d, seq + at, (size_t)bytes);
	++n_loads;
	return d;
}

/* what seq_issue() + seq_finish() of csrc/seq_stream.h do for one dword */
static uint32_t by_core(const uint8_t *seq, int len, int p, int rev)
{
	const int m = bmh_seqs_mem_pos(p, len, rev), a = bmh_seqs_dword_at(m, len);
	uint32_t d = 0;
	if (len >= 4) d = load(seq, len, a, 4);
	else if (len > 0) d = load(seq, len, 0, 1) | load(seq, len, bmh_seqs_small_at(1, len), 1) << 8 | load(seq, len, bmh_seqs_small_at(2, len), 1) << 16;
	return bmh_seqs_assemble(d, a, m, len, rev);
}

/* the restatement: position k is seq[k], or seq[len-1-k] of a reversed sequence; outside [0, len) base 4 */
static uint32_t by_bytes(const uint8_t *seq, int len, int p, int rev)
{
	uint32_t v = 0;
	int k;
	for (k = 0; k < 4; ++k) {
		const int q = p + k;
		const uint32_t b = q >= 0 && q < len ? seq[rev ? len - 1 - q : q] : 4u;
		v |= b << (8 * k);
	}
	return v;
}

int main(void)
{
	unsigned long long n = 0;
	uint32_t rng = 12345u;
	int len, align, rev, p, r0i, qsh, k;
	for (len = 0; len <= 200; ++len)
		for (align = 0; align < 16; ++align) {
			uint8_t *blk = (uint8_t *)malloc((size_t)(align + len) ? (size_t)(align + len) : 1u); /* (malloc: 16-byte aligned) */
			uint8_t *seq = blk + align;
			if (!blk) return 3;
			for (k = 0; k < align + len; ++k) {
				rng = rng * 1664525u + 1013904223u;
				blk[k] = (uint8_t)(rng >> 24); /* any byte value: the core must carry all eight bits */
			}
			for (rev = 0; rev < 2; ++rev) {
				for (p = -72; p < 288; ++p) {
					const uint32_t got = by_core(seq, len, p, rev), want = by_bytes(seq, len, p, rev);
					if (got != want) {
						fprintf(stderr, "len %d align %d rev %d p %d: %08x, expected %08x\n", len, align, rev, p, got, want);
						return 1;
					}
					++n;
				}
				/* the refill's own walk, spelled out: 16 dwords per 64 rows, target unshifted (qsh 0) and query shifted by 1..16 */
				for (r0i = 0; r0i < 4; ++r0i)
					for (qsh = 0; qsh <= 16; ++qsh)
						for (k = 0; k < 16; ++k) {
							const int q = 64 * r0i + qsh + 4 * k;
							if (by_core(seq, len, q, rev) != by_bytes(seq, len, q, rev)) {
								fprintf(stderr, "len %d align %d rev %d r0 %d qsh %d dword %d\n", len, align, rev, 64 * r0i, qsh, k);
								return 1;
							}
							++n;
						}
			}
			free(blk);
		}
	printf("ok %llu %llu\n", n, n_loads);
	return 0;
}
