/*
 * samcut_core.h -- a batch's SAM text cut into one string per read, as ONE text for its two callers: bmh_sam_batch (host/sam_post.c,
 * in libbwamem_hip.so) behind whichever route made the text, and the preload shim's single-end session (host/interpose.c, in
 * libbwamem_hip_dropin.so) behind bmh_reads_sam_device.  The two callers live in two libraries, so the routine is a static function
 * in a header and no symbol of either; tests/samcut_core_main.c builds it with gcc on its own.
 *   bmh_sam_cut   seqs[i].sam = a malloc'd, NUL-terminated copy of text[text_off[i] .. text_off[i + 1]) for i in [0, n).
 *                 BMH_OK, or BMH_E_NOMEM: all or nothing, the strings it made are freed and their seqs[i].sam set to NULL.
 *                 BMH_E_ARG for offsets that run backwards (no caller's do: they come from a scan over sizes), nothing is made.
 * A read without a line gets the empty string, never NULL: the host program prints seqs[i].sam as it is.
 */
#ifndef BMH_SAMCUT_CORE_H
#define BMH_SAMCUT_CORE_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bwamem_hip.h"

#ifndef BMH_SAMCUT_MALLOC /* (the stand-alone program counts and fails allocations through this) */
#define BMH_SAMCUT_MALLOC malloc
#endif

static int bmh_sam_cut(int n, bmh_seq_t *seqs, const char *text, const int64_t *text_off)
{
	int i;
	for (i = 0; i < n; ++i)
		if (text_off[i + 1] < text_off[i]) return BMH_E_ARG;
	for (i = 0; i < n; ++i) {
		const size_t len = (size_t)(text_off[i + 1] - text_off[i]);
		char *s = (char *)BMH_SAMCUT_MALLOC(len + 1);
		if (!s) { /* all or nothing */
			while (--i >= 0) free(seqs[i].sam), seqs[i].sam = 0;
			return BMH_E_NOMEM;
		}
		memcpy(s, text + text_off[i], len), s[len] = 0;
		seqs[i].sam = s;
	}
	return BMH_OK;
}

#endif
