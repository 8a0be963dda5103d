/*
 * regfinish_core.h -- how a region record is finished once its tries have run, as ONE text for gcc and hipcc: the long round of
 * bmh_region_cigar_batch_long (csrc/region_long.hip, one lane per region) and the stand-alone program of the tests
 * (tests/regfinish_core_main.c).  Restated from region_finish_kernel (csrc/region_cigar.hip), which keeps its own text.
 *   bmh_rf_replay   mem_reg2aln's band loop over the tries' results     reference bwa-0.7.8/bwamem.c:1194-1201
 *   bmh_rf_nm_md    NM and MD of a CIGAR over the oriented copies       bwa.c:134-164
 * The MD bytes go through a sink that counts every byte and stores only those below its size: with size 0 (and no buffer) it is
 * the size pass, with the size the size pass gave it is the write pass.  No NUL is written.  The walk also never reads past
 * the two sequences: an operation that would run past ql or tl ends it with -1 (a CIGAR that does not belong to the pair).
 * Nothing is allocated.  Under hipcc every routine is __host__ __device__ and always inlined.
 */
#ifndef BMH_REGFINISH_CORE_H
#define BMH_REGFINISH_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bwamem_hip.h"

#ifdef __HIPCC__
#define BMH_RF_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_RF_HD
#endif

typedef struct bmh_rf_replay {
	int32_t fin; /* index of the task the loop ends on */
	int32_t tries, score, n_cigar;
} bmh_rf_replay_t;

/* ---- bwamem.c:1194-1201 over the precomputed tries task[0..2] (task[0] >= 0; equal bands share an index); a = opt->a */
BMH_RF_HD static inline void bmh_rf_replay(const int32_t task[3], int truesc, int a, const bmh_glb_result_t *gres, bmh_rf_replay_t *o)
{
	const int single = truesc == INT32_MIN;
	int last = -(1 << 30), tries = 0, t_;
	for (t_ = 0;; ++t_) {
		o->fin = task[t_];
		++tries;
		o->score = gres[o->fin].score;
		if (o->score == last) break; /* bwamem.c:1198 */
		last = o->score;
		if (single || !(tries < 3 && o->score < truesc - a)) break; /* bwamem.c:1201 */
	}
	o->tries = tries, o->n_cigar = gres[o->fin].n_cigar;
}

typedef struct bmh_rf_sink { /* kputc / kputw into s[0, cap); past cap only the length keeps counting */
	char *s;
	int64_t l, cap;
} bmh_rf_sink_t;

BMH_RF_HD static inline void bmh_rf_putc(bmh_rf_sink_t *k, char ch)
{
	if (k->l < k->cap) k->s[k->l] = ch;
	++k->l;
}

BMH_RF_HD static inline void bmh_rf_putw(bmh_rf_sink_t *k, int v) /* kputw (kstring.h:62-77), v >= 0 */
{
	char buf[12];
	int n = 0;
	if (v == 0) buf[n++] = '0';
	for (; v > 0; v /= 10) buf[n++] = (char)('0' + v % 10);
	while (n) bmh_rf_putc(k, buf[--n]);
}

/* ---- bwa.c:134-164: walk the CIGAR over the oriented copies q[0, ql) and t[0, tl); `run` = matches since the last MD token.
 * Returns NM, md->l = strlen(MD); -1 when the CIGAR runs past either sequence (md->l is then meaningless). */
BMH_RF_HD static inline int bmh_rf_nm_md(int n_cigar, const uint32_t *cigar, const uint8_t *q, int ql, const uint8_t *t, int tl, int rev,
                                         bmh_rf_sink_t *md)
{
	const char *letter = rev ? "TGCAN" : "ACGTN";
	int c, i, qpos = 0, tpos = 0, run = 0, mismatches = 0, gap_bases = 0;
	for (c = 0; c < n_cigar; ++c) {
		const int op = (int)(cigar[c] & 0xf), len = (int)(cigar[c] >> 4);
		switch (op) {
		case 0: /* M: a mismatch closes the run and names the reference base */
			if (len > ql - qpos || len > tl - tpos) return -1;
			for (i = 0; i < len; ++i) {
				const int tb = t[tpos + i];
				if (q[qpos + i] == tb) {
					++run;
					continue;
				}
				bmh_rf_putw(md, run), bmh_rf_putc(md, letter[tb < 4 ? tb : 4]);
				++mismatches, run = 0;
			}
			qpos += len, tpos += len;
			break;
		case 2: /* D: "^" + the deleted reference bases, unless it is the first or the last operation */
			if (len > tl - tpos) return -1;
			if (c > 0 && c < n_cigar - 1) {
				bmh_rf_putw(md, run), bmh_rf_putc(md, '^');
				for (i = 0; i < len; ++i) {
					const int tb = t[tpos + i];
					bmh_rf_putc(md, letter[tb < 4 ? tb : 4]);
				}
				run = 0, gap_bases += len;
			}
			tpos += len;
			break;
		case 1: /* I */
			if (len > ql - qpos) return -1;
			qpos += len, gap_bases += len;
			break;
		default: break;
		}
	}
	bmh_rf_putw(md, run);
	return mismatches + gap_bases;
}

#endif
