/*
 * extstop_core.h -- when a ksw_extend2 flank (reference bwa-0.7.8/ksw.c:379-476) may end before the reference's own loop does, as ONE
 * text for the device (csrc/extend_lane.hip, hipcc) and for a C test program (tests/extstop_core_main.c, gcc).  DESIGN.md §4.3 has the
 * argument; in short, with A = max(mat) and row i finished (its cells, the gscore update and the max update, the loop not broken):
 *
 *   U_i = max( max over beg <= j < end of H(i,j) + A (qlen-1-j),          every live cell, with one best match per column to its right
 *              max(h0 - o_del - e_del (i+1), 0) + A (qlen-beg) )          row i's own first-column value, which row i+1 reads diagonally
 *                                                                          at column beg even when beg > 0 (ksw.c:415,429)
 *
 *   stop after row i  iff  U_i <= max  and  U_i < gscore.
 *
 * No cell of a later row exceeds U_i, `max` changes only through m > max (strictly) and gscore through h1 >= gscore (a tie goes to the
 * later row, hence strictly below), so none of the six outputs can change; m == 0 and z-drop only end the loop sooner.  With
 * gscore == -1 the test never passes (U_i >= 0).  The rule holds only for A >= 0 and gap costs >= 0.
 *
 * Any bound at or above U_i is as valid.  The lane kernels take it per block of eight columns counted from the query's right end:
 * the row maximum over the live columns up to the block's end, plus A times the columns to the right of the block's FIRST column
 * (8r + 7 for block r from the right).  Only blocks up to which the lane has a live column count.
 *
 * The switch is the factor itself: A when the rule is on and applies, else BMH_EXTSTOP_OFF, with which no bound can stay at or
 * below a 16-bit score.  Plain C, no allocation; under hipcc __host__ __device__ and always inlined.
 */
#ifndef BMH_EXTSTOP_CORE_H
#define BMH_EXTSTOP_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define BMH_XS_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_XS_HD
#endif

#define BMH_EXTSTOP_OFF (1 << 20) /* times at least one column: above every score the kernels hold; times 128 columns: within int32 */

/* the largest entry of mat[25] (not floored at 0 as ksw.c:399-400 floors its own) */
BMH_XS_HD static inline int bmh_extstop_amax(const int8_t *mat)
{
	int k, a = mat[0];
	for (k = 1; k < 25; ++k) a = mat[k] > a ? mat[k] : a;
	return a;
}

/* does the rule apply to a scoring */
BMH_XS_HD static inline int bmh_extstop_applies(int amax, int o_del, int e_del, int o_ins, int e_ins)
{
	return amax >= 0 && o_del >= 0 && e_del >= 0 && o_ins >= 0 && e_ins >= 0;
}

/* the allowance per column a launch runs with */
BMH_XS_HD static inline int bmh_extstop_factor(int on, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins)
{
	const int amax = bmh_extstop_amax(mat);
	return on && bmh_extstop_applies(amax, o_del, e_del, o_ins, e_ins) ? amax : BMH_EXTSTOP_OFF;
}

/* first-column term: row i's first-column value `left` = max(h0 - o_del - e_del (i+1), 0), and the columns from beg on */
BMH_XS_HD static inline int bmh_extstop_first(int left, int factor, int cols_from_beg) { return left + factor * cols_from_beg; }

/* per-block term joined into u: m = the row maximum over the live columns up to the block's end, negative if there is none yet;
 * right = the columns to the right of the block's first column.  (For one cell: m = H(i,j), right = qlen-1-j.) */
BMH_XS_HD static inline int bmh_extstop_block(int u, int m, int factor, int right)
{
	const int t = m + factor * right;
	return m >= 0 && t > u ? t : u;
}

/* the test, with max and gscore as they stand after row i's updates */
BMH_XS_HD static inline int bmh_extstop_test(int u, int max, int gscore) { return u <= max && u < gscore; }

#endif
