/*
 * glbbin_core.h -- which bin of the global dispatcher a lane-kernel task goes to, and its sort key inside the bin, from the band
 * the task runs on (the band pass's w_eff, or its own w).  One source for glb_sort_hist_kernel (csrc/global_kernel.hip) and for the
 * stand-alone check tests/glbbin_core_main.c; tests/glbbin_ref.py restates it in Python.
 *
 *   bin 6: bands 0..3  -> global_narrow_kernel (level `exact` >= 3)      bin 7: bands 4..7 -> global_narrow_kernel (level 7)
 *   bin 5: bands <= 15 -> global_lane_kernel<32> (c32 on)                bin 0: <= 31 -> <64>    bin 3: <= 47 -> <96>    bin 1: <= 63 -> <128>
 *   bin 2: wider: the wave kernel
 *
 * The key has kGlbKeyBits bits.  Bins 0, 1, 3, 5: rows first (the lanes of a wave run until their longest target ends), then the band
 * in the bin's resolution.  Bins 6, 7: the band first, then rows -- a wave of global_narrow_kernel runs one row pass per distinct
 * band among its lanes, so only a wave where two bands meet in the sorted list runs more than one.
 */
#ifndef BMH_GLBBIN_CORE_H
#define BMH_GLBBIN_CORE_H

#ifdef __HIPCC__
#define BMH_GBIN_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_GBIN_HD
#endif

enum { kGlbKeyBits = 11, kGlbExactLow = 3, kGlbExactAll = 7 };

/* w >= 0: the band of a task the lane kernels may take (glb_lane_domain) */
BMH_GBIN_HD static inline int bmh_glb_lane_bin(int w, int c32, int exact)
{
	if (exact >= kGlbExactLow && w <= 3) return 6;
	if (exact >= kGlbExactAll && w <= 7) return 7;
	return c32 && w <= 15 ? 5 : w <= 31 ? 0 : w <= 47 ? 3 : (w <= 63 ? 1 : 2);
}

BMH_GBIN_HD static inline int bmh_glb_sort_key(int bin, int tlen, int w)
{
	const int rows = tlen >> 3, wc = w < 63 ? w : 63;
	if (bin == 2 || bin == 4) return 0;
	if (bin == 6 || bin == 7) return (w & 3) << 9 | (rows < 511 ? rows : 511);
	return (rows < 127 ? rows : 127) << 4 | (wc >> (bin == 5 ? 0 : bin == 0 ? 1 : 2) & 15);
}

#endif
