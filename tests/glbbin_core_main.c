/*
 * glbbin_core_main.c -- stand-alone check of host/glbbin_core.h for a plain and a sanitizer build:
 * tests/test_global_exact_cpu.py compiles it with gcc and runs it as a child process.
 *
 * Without arguments it prints, for every band w = 0..300, every switch setting (c32 0/1, exact 0/3/7) and a set of target lengths,
 * one line "w c32 exact tlen bin key", which the test compares with tests/glbbin_ref.py line by line.  It also checks what the
 * dispatcher relies on and exits 1 where that fails:
 *   the key fits kGlbKeyBits bits; with exact = 0 no task reaches bins 6 and 7 and the bin is the one of the rule before them;
 *   a bin 6 task has a band of 0..3 and a bin 7 task one of 4..7; inside bins 6 and 7 the key is band-major (a wider band never has
 *   a smaller key), and inside one band it does not fall with the rows.
 */
#include <stdio.h>

#include "../bwa-mem-quickassist_amd/host/glbbin_core.h"

static int old_bin(int w, int c32) { return c32 && w <= 15 ? 5 : w <= 31 ? 0 : w <= 47 ? 3 : (w <= 63 ? 1 : 2); }

int main(void)
{
	static const int tlens[] = {0, 1, 7, 8, 9, 63, 64, 150, 151, 152, 300, 511, 512, 1015, 1016, 1024, 4095, 4096, 65535};
	static const int exacts[] = {0, 3, 7};
	const int nt = (int)(sizeof(tlens) / sizeof(tlens[0]));
	int bad = 0, w, c32, e, t;
	for (w = 0; w <= 300; ++w)
		for (c32 = 0; c32 <= 1; ++c32)
			for (e = 0; e < 3; ++e) {
				const int bin = bmh_glb_lane_bin(w, c32, exacts[e]);
				int prev_key = -1;
				if (exacts[e] == 0 && (bin != old_bin(w, c32) || bin >= 6)) ++bad;
				if (bin == 6 && !(w <= 3 && exacts[e] >= 3)) ++bad;
				if (bin == 7 && !(w >= (exacts[e] >= 3 ? 4 : 0) && w <= 7 && exacts[e] == 7)) ++bad;
				if (bin != 6 && bin != 7 && bin != old_bin(w, c32)) ++bad;
				for (t = 0; t < nt; ++t) {
					const int key = bmh_glb_sort_key(bin, tlens[t], w);
					printf("%d %d %d %d %d %d\n", w, c32, exacts[e], tlens[t], bin, key);
					if (key < 0 || key >= 1 << kGlbKeyBits) ++bad;
					if ((bin == 6 || bin == 7) && key < prev_key) ++bad; /* rows do not lower the key */
					if ((bin == 6 || bin == 7) && w > 0 && bmh_glb_lane_bin(w - 1, c32, exacts[e]) == bin &&
					    bmh_glb_sort_key(bin, 65535, w - 1) >= bmh_glb_sort_key(bin, 0, w))
						++bad; /* band-major */
					prev_key = key;
				}
			}
	if (bad) fprintf(stderr, "%d property violations\n", bad);
	return bad != 0;
}
