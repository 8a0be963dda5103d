/*
 * regfinish_core_main.c -- stand-alone check of host/regfinish_core.h for a plain and a sanitizer build:
 * tests/test_region_long_cpu.py compiles it with gcc, links the oracle (liborc.so) and runs it as a child process.
 *
 * Per region it does what the long round of bmh_region_cigar_batch_long does behind the tries: the plan of host/regplan_core.h,
 * oriented copies from the 2-bit reference, one orc_global per planned task (in place of the global kernels), bmh_rf_replay over
 * their results, then bmh_rf_nm_md twice -- the size pass into a sink without a buffer, the write pass into a heap block of
 * exactly the size the size pass gave.  Both oriented sequences, the task results, the final CIGAR and the MD live in heap blocks
 * of exactly their sizes, so an access past any of them is the sanitizer's to report.
 *
 * Input file (little endian, written by the test):
 *   bmh_params_t, int64 l_pac, int32 pac_bytes, pac, int32 n_regions,
 *   per region: int32 ql, its base codes (read orientation), int64 rb, int64 re, int32 truesc, int32 reg_w
 * Output: per region one line
 *   "region K: bands B0 B1 B2 score S n_cigar N tries T fin F NM M md_len L sized Z cigar <hex words, comma separated> md <MD or ->"
 * (fin: the index of the try the loop ends on, -1 in the no-gap case; sized: the size pass's length).  Exit status 0: every size
 * pass gave the length and NM of its write pass, and no walk left its sequences.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/regfinish_core.h"
#include "../bwa-mem-quickassist_amd/host/regplan_core.h"
#include "../oracle/ksw_oracle.h"

static int rd(void *p, size_t sz, size_t n, FILE *f) { return n == 0 || fread(p, sz, n, f) == n; }

static int base_at(const uint8_t *pac, int64_t l_pac, int64_t pos) /* the doubled coordinate, bntseq.c:355-376 */
{
	if (pos >= l_pac) return 3 - base_at(pac, l_pac, (l_pac << 1) - 1 - pos);
	return pac[pos >> 2] >> ((~pos & 3) << 1) & 3;
}

static void *exact(size_t n) /* a block of exactly n bytes (n == 0: one that must not be touched) */
{
	void *p = malloc(n ? n : 1);
	if (!p) exit(2);
	return p;
}

int main(int argc, char **argv)
{
	bmh_params_t p;
	bmh_rp_opt_t po;
	orc_scoring_t sc;
	int64_t l_pac;
	int32_t pac_bytes, n_regions, k;
	uint8_t *pac;
	FILE *f;
	int bad = 0;
	if (argc != 2 || !(f = fopen(argv[1], "rb"))) return 2;
	if (!rd(&p, sizeof(p), 1, f) || !rd(&l_pac, 8, 1, f) || !rd(&pac_bytes, 4, 1, f)) return 2;
	pac = (uint8_t *)exact((size_t)pac_bytes);
	if (!rd(pac, 1, (size_t)pac_bytes, f) || !rd(&n_regions, 4, 1, f)) return 2;
	po.a = p.a, po.mat0 = p.mat[0], po.o_del = p.o_del, po.e_del = p.e_del, po.o_ins = p.o_ins, po.e_ins = p.e_ins, po.w = p.w;
	sc.o_del = p.o_del, sc.e_del = p.e_del, sc.o_ins = p.o_ins, sc.e_ins = p.e_ins, sc.zdrop = 0, sc.m = 5, sc.mat = p.mat;
	for (k = 0; k < n_regions; ++k) {
		int32_t ql, tl, truesc, reg_w, i, t;
		int64_t rb, re;
		uint8_t *read, *q, *tg;
		bmh_rp_plan_t pl;
		bmh_glb_result_t *gres;
		uint32_t **tcig, *words;
		int32_t task[3];
		bmh_rf_replay_t rp;
		bmh_rf_sink_t sink;
		char *md;
		int rev, nm0, nm1;
		int64_t sized;
		if (!rd(&ql, 4, 1, f)) return 2;
		read = (uint8_t *)exact((size_t)ql);
		if (!rd(read, 1, (size_t)ql, f) || !rd(&rb, 8, 1, f) || !rd(&re, 8, 1, f) || !rd(&truesc, 4, 1, f) || !rd(&reg_w, 4, 1, f)) return 2;
		tl = (int32_t)(re - rb), rev = rb >= l_pac;
		q = (uint8_t *)exact((size_t)ql), tg = (uint8_t *)exact((size_t)tl);
		for (i = 0; i < ql; ++i) q[i] = rev ? read[ql - 1 - i] : read[i]; /* bwa.c:100-107 */
		for (i = 0; i < tl; ++i) tg[i] = (uint8_t)base_at(pac, l_pac, rev ? re - 1 - i : rb + i);
		bmh_rp_plan(&po, ql, tl, truesc, reg_w, &pl);
		gres = (bmh_glb_result_t *)exact(sizeof(*gres) * (size_t)pl.n_tasks);
		tcig = (uint32_t **)exact(sizeof(*tcig) * (size_t)pl.n_tasks);
		for (t = 0; t < 3; ++t) {
			task[t] = pl.slot[t];
			if (pl.slot[t] < 0 || (t > 0 && pl.slot[t] == pl.slot[t - 1])) continue;
			gres[pl.slot[t]].score = orc_global(&sc, ql, q, tl, tg, pl.band[t], &gres[pl.slot[t]].n_cigar, &tcig[pl.slot[t]]);
		}
		if (pl.n_tasks == 0) { /* no gap, no DP: one match run (bwa.c:108-114) */
			int s = 0;
			for (i = 0; i < ql; ++i) s += p.mat[tg[i] * 5 + q[i]];
			rp.fin = -1, rp.score = s, rp.n_cigar = 1, rp.tries = (truesc != INT32_MIN && s < truesc - p.a) ? 2 : 1;
			words = (uint32_t *)exact(4);
			words[0] = (uint32_t)ql << 4;
		} else {
			bmh_rf_replay(task, truesc, p.a, gres, &rp);
			words = (uint32_t *)exact(4 * (size_t)rp.n_cigar);
			memcpy(words, tcig[rp.fin], 4 * (size_t)rp.n_cigar);
		}
		sink.s = 0, sink.l = 0, sink.cap = 0; /* the size pass */
		nm0 = bmh_rf_nm_md(rp.n_cigar, words, q, ql, tg, tl, rev, &sink);
		sized = sink.l;
		md = (char *)exact((size_t)(sized > 0 ? sized : 0));
		sink.s = md, sink.l = 0, sink.cap = sized; /* the write pass */
		nm1 = bmh_rf_nm_md(rp.n_cigar, words, q, ql, tg, tl, rev, &sink);
		if (nm0 < 0 || nm1 != nm0 || sink.l != sized) ++bad;
		/* (fin is printed as the index of the try the loop ended on, tries - 1, not of the task) */
		printf("region %d: bands %d %d %d score %d n_cigar %d tries %d fin %d NM %d md_len %lld sized %lld cigar ", (int)k, pl.band[0], pl.band[1],
		       pl.band[2], rp.score, rp.n_cigar, rp.tries, rp.fin < 0 ? -1 : rp.tries - 1, nm1, (long long)sink.l, (long long)sized);
		for (i = 0; i < rp.n_cigar; ++i) printf("%s%x", i ? "," : "", words[i]);
		printf(" md ");
		if (sized > 0) fwrite(md, 1, (size_t)sized, stdout);
		else printf("-");
		printf("\n");
		for (t = 0; t < pl.n_tasks; ++t) free(tcig[t]);
		free(read), free(q), free(tg), free(gres), free(tcig), free(words), free(md);
	}
	free(pac);
	fclose(f);
	printf("%d regions, %d differ\n", (int)n_regions, bad);
	return bad ? 1 : 0;
}
