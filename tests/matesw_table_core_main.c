/*
 * matesw_table_core_main.c -- host/matesw_table_core.h as a stand-alone program, for a plain build and one under AddressSanitizer: what
 * mt_filter_kernel decides about every pair of a region table -- candidate counts, busy, slice capacities, the reads' refusals -- with
 * every vector in a heap block of exactly its size, so that a read one record past a vector is an error the sanitizer reports.  An empty
 * vector has no block at all: the rules must not look at it.
 *
 *   matesw_table_core_main FILE
 *
 * FILE (little endian, written by tests/test_matesw_table_core_cpu.py):
 *   int32 magic 0x4d545442, int32 n_pairs, int64 l_pac, bmh_pestat_t[4] (32 bytes each), bmh_matesw_opt_t (16), bmh_mt_rule_t (24),
 *   per pair {int32 n0, n1; int64 l_seq0, l_seq1} (24 bytes), then the regions of all vectors, 64 bytes each
 * Prints one line per pair:  p nb0 nb1 busy cap0 cap1 refuse0 refuse1
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/matesw_table_core.h"

typedef struct {
	int32_t n[2];
	int64_t l_seq[2];
} pair_head_t;

static int fail(const char *why)
{
	fprintf(stderr, "matesw_table_core_main: %s\n", why);
	return 2;
}

int main(int argc, char **argv)
{
	int32_t head[2];
	int64_t l_pac;
	bmh_pestat_t pes[4];
	bmh_matesw_opt_t o;
	bmh_mt_rule_t rule;
	pair_head_t *ph = 0;
	FILE *f;
	int p, n, i;
	if (argc != 2) return fail("usage: matesw_table_core_main FILE");
	if (sizeof(bmh_pestat_t) != 32 || sizeof(o) != 16 || sizeof(rule) != 24 || sizeof(pair_head_t) != 24 || sizeof(bmh_alnreg_t) != 64 ||
	    sizeof(bmh_mt_pair_t) != 40)
		return fail("record sizes");
	if (!(f = fopen(argv[1], "rb"))) return fail("cannot open the case file");
	if (fread(head, 4, 2, f) != 2 || head[0] != 0x4d545442 || fread(&l_pac, 8, 1, f) != 1 || fread(pes, sizeof(pes), 1, f) != 1 ||
	    fread(&o, sizeof(o), 1, f) != 1 || fread(&rule, sizeof(rule), 1, f) != 1)
		return fail("bad header");
	n = head[1];
	if (n < 0) return fail("bad pair count");
	ph = (pair_head_t *)malloc(sizeof(pair_head_t) * (size_t)(n + 1));
	if (!ph || fread(ph, sizeof(pair_head_t), (size_t)n, f) != (size_t)n) return fail("bad pair heads");
	for (p = 0; p < n; ++p) {
		bmh_alnreg_t *a[2] = {0, 0};
		bmh_mt_pair_t m;
		for (i = 0; i < 2; ++i) {
			const size_t k = (size_t)ph[p].n[i];
			if (ph[p].n[i] < 0) return fail("bad count");
			if (!k) continue;
			a[i] = (bmh_alnreg_t *)malloc(k * sizeof(bmh_alnreg_t));
			if (!a[i] || fread(a[i], sizeof(bmh_alnreg_t), k, f) != k) return fail("bad regions");
		}
		bmh_mt_pair(l_pac, pes, &o, &rule, a[0], ph[p].n[0], a[1], ph[p].n[1], ph[p].l_seq[0], ph[p].l_seq[1], &m);
		printf("%d %d %d %d %lld %lld %d %d\n", p, (int)m.nb[0], (int)m.nb[1], (int)m.busy, (long long)m.cap[0], (long long)m.cap[1], (int)m.refuse[0],
		       (int)m.refuse[1]);
		free(a[0]), free(a[1]);
	}
	fclose(f);
	free(ph);
	return 0;
}
