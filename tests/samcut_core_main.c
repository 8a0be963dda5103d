/* host/samcut_core.h on its own: bmh_sam_cut over a text and offsets the program makes from its arguments, every block of its exact size.
 *   samcut_core_main <n> <seed> <fail_at>
 * n reads whose line lengths come from a small generator (every fourth read has no line at all), cut into strings and checked byte
 * for byte; fail_at >= 0 makes the fail_at-th allocation of the cut fail, and the program checks that no read keeps a string (the sanitizer's leak check sees the rest).
 * Prints "reads N bytes B strings S rc R". */
#include <stdio.h>

static long g_allocs, g_fail_at = -1;
static void *counted_malloc(size_t n);
#define BMH_SAMCUT_MALLOC counted_malloc
#include "../bwa-mem-quickassist_amd/host/samcut_core.h"

static void *counted_malloc(size_t n)
{
	return g_allocs++ == g_fail_at ? 0 : malloc(n);
}

int main(int argc, char **argv)
{
	const int n = argc > 1 ? atoi(argv[1]) : 0;
	uint32_t x = argc > 2 ? (uint32_t)atoi(argv[2]) * 2654435761u + 1u : 1u;
	bmh_seq_t *seqs = (bmh_seq_t *)calloc((size_t)n + 1, sizeof(bmh_seq_t));
	int64_t *off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)n + 1));
	char *text;
	int64_t k;
	int i, rc, strings = 0;
	g_fail_at = argc > 3 ? atol(argv[3]) : -1;
	if (!seqs || !off) return 2;
	for (i = 0, off[0] = 0; i < n; ++i) {
		x = x * 1664525u + 1013904223u;
		off[i + 1] = off[i] + ((i & 3) == 3 ? 0 : 1 + (int64_t)((x >> 8) % 700));
	}
	if (!(text = (char *)malloc((size_t)off[n] ? (size_t)off[n] : 1))) return 2; /* exactly the text: no terminator behind it */
	for (k = 0; k < off[n]; ++k) text[k] = (char)('!' + (k * 7 + (k >> 5)) % 90);
	rc = bmh_sam_cut(n, seqs, text, off);
	if (rc == BMH_OK) {
		for (i = 0; i < n; ++i) {
			const size_t len = (size_t)(off[i + 1] - off[i]);
			if (!seqs[i].sam || strlen(seqs[i].sam) != len || memcmp(seqs[i].sam, text + off[i], len) != 0) {
				printf("read %d: its string is not its slice of the text\n", i);
				return 1;
			}
			++strings, free(seqs[i].sam);
		}
	} else {
		for (i = 0; i < n; ++i)
			if (seqs[i].sam) {
				printf("read %d keeps a string behind a failed cut\n", i);
				return 1;
			}
	}
	if (g_allocs != (rc == BMH_OK ? n : g_fail_at + 1)) { /* one allocation per read, and none behind the one that failed */
		printf("%ld allocations\n", g_allocs);
		return 1;
	}
	if (n >= 2 && off[1] > 0) { /* offsets that run backwards are refused before anything is made */
		const int64_t back[3] = {off[1], 0, off[2]};
		seqs[0].sam = seqs[1].sam = 0;
		if (bmh_sam_cut(2, seqs, text, back) != BMH_E_ARG || seqs[0].sam || seqs[1].sam) {
			printf("offsets that run backwards were not refused\n");
			return 1;
		}
	}
	printf("reads %d bytes %lld strings %d rc %d\n", n, (long long)off[n], strings, rc);
	free(text), free(off), free(seqs);
	return 0;
}
