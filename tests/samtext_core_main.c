/* samtext_core_main.c -- host/samtext_core.h driven as the kernels of csrc/samtext.hip drive it, over a dumped slice with every array
 * in a heap block of exactly its size, so that a build under -fsanitize=address,undefined sees any access past what the core was
 * promised.  For every read: the counting sink, then the writing sink into a block of EXACTLY the counted size -- counted, written and
 * the host call's size (and bytes) must agree -- then a block one byte short, which the sink must refuse without touching the byte
 * behind it.  A size / emit disagreement here would be an out-of-bounds store on the device.
 * The dump (tests/test_samtext_cpu.py writes it), little-endian:
 *   int64 n, pe, opt_flag, l_pac, n_seqs, total, n_w, cig_words, md_bytes, names_bytes, l_rg, pool_bytes
 *   bmh_refspan_t[n_seqs], uint64 name_off[n_seqs + 1], names, bmh_pestat_t[4], int64 roff[n + 1], int64 first[n + 1], int32 n_want[n],
 *   int32 want_k[total], int32 reg_mapq[total], bmh_pairdec_t[n / 2], bmh_alnreg_t[total], bmh_wanted_res_t[n_w], uint32 cig[cig_words],
 *   md, rg_id, uint64 poff[n + 1], the read pool (per read int32 l_name, l_seq, has_qual, l_comment, then the bytes), int64 text_off[n + 1],
 *   the host call's text
 * Prints "ok <reads> <lines> <bytes>". */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/samtext_core.h"

static void die(const char *what, long long i)
{
	fprintf(stderr, "%s (read %lld)\n", what, i);
	exit(1);
}
static void *block(FILE *f, size_t bytes) /* exactly `bytes` from the dump */
{
	void *p = malloc(bytes ? bytes : 1);
	if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) die("short input", -1);
	return p;
}

static bmh_st_read_t view(const uint8_t *pool, const uint64_t *poff, int i)
{
	const int32_t *h = (const int32_t *)(pool + poff[i]);
	const char *b = (const char *)(h + 4);
	bmh_st_read_t v;
	v.name = b, v.l_name = h[0], b += h[0];
	v.seq = (const uint8_t *)b, v.l_seq = h[1], b += h[1];
	v.qual = h[2] ? b : 0, b += h[2] ? h[1] : 0;
	v.comment = h[3] >= 0 ? b : 0, v.l_comment = h[3] >= 0 ? h[3] : 0, v.rsv_ = 0;
	return v;
}

int main(int argc, char **argv)
{
	FILE *f;
	int64_t hd[12], n, pe, total, n_w, i, lines = 0;
	bmh_refspan_t *ref;
	bmh_rp_refv_t rv;
	bmh_st_env_t E;
	uint64_t *noff, *poff;
	char *names, *md, *rg, *text;
	bmh_pestat_t *pes;
	int64_t *roff, *first, *toff;
	int32_t *n_want, *want_k, *reg_mapq;
	bmh_pairdec_t *pd;
	bmh_alnreg_t *reg;
	bmh_wanted_res_t *wr;
	uint32_t *cig;
	uint8_t *pool;
	bmh_st_aln_t *alns;
	bmh_st_plan_t *plan;
	if (argc != 2 || !(f = fopen(argv[1], "rb"))) return 2;
	if (fread(hd, 8, 12, f) != 12) die("short input", -1);
	n = hd[0], pe = hd[1], total = hd[5], n_w = hd[6];
	ref = (bmh_refspan_t *)block(f, sizeof(*ref) * (size_t)hd[4]);
	noff = (uint64_t *)block(f, 8 * ((size_t)hd[4] + 1)), names = (char *)block(f, (size_t)hd[9]);
	pes = (bmh_pestat_t *)block(f, 4 * sizeof(*pes));
	roff = (int64_t *)block(f, 8 * ((size_t)n + 1)), first = (int64_t *)block(f, 8 * ((size_t)n + 1));
	n_want = (int32_t *)block(f, 4 * (size_t)n), want_k = (int32_t *)block(f, 4 * (size_t)total), reg_mapq = (int32_t *)block(f, 4 * (size_t)total);
	pd = (bmh_pairdec_t *)block(f, pe ? sizeof(*pd) * (size_t)(n >> 1) : 0);
	reg = (bmh_alnreg_t *)block(f, sizeof(*reg) * (size_t)total), wr = (bmh_wanted_res_t *)block(f, sizeof(*wr) * (size_t)n_w);
	cig = (uint32_t *)block(f, 4 * (size_t)hd[7]), md = (char *)block(f, (size_t)hd[8]), rg = (char *)block(f, (size_t)hd[10]);
	poff = (uint64_t *)block(f, 8 * ((size_t)n + 1)), pool = (uint8_t *)block(f, (size_t)hd[11]);
	toff = (int64_t *)block(f, 8 * ((size_t)n + 1)), text = (char *)block(f, (size_t)toff[n]);
	alns = (bmh_st_aln_t *)malloc(n_w ? sizeof(*alns) * (size_t)n_w : 1), plan = (bmh_st_plan_t *)malloc(n ? sizeof(*plan) * (size_t)n : 1);
	if (!alns || !plan) return 3;
	rv.off0 = &ref[0].offset, rv.len0 = &ref[0].len, rv.stride = sizeof(*ref), rv.n_seqs = (int32_t)hd[4], rv.l_pac = hd[3];
	E.names.pool = names, E.names.off = noff, E.names.n_seqs = (int32_t)hd[4], E.names.rsv_ = 0;
	E.cig = cig, E.md = md, E.rg_id = rg, E.l_rg = (int32_t)hd[10], E.rsv_ = 0;
	(void)n_want;
	for (i = 0; i < n; ++i) { /* the records, as samtext_size_kernel makes them */
		const bmh_st_read_t v = view(pool, poff, (int)i);
		int64_t q;
		for (q = first[i]; q < first[i + 1]; ++q) {
			const int k = want_k[roff[i] + (q - first[i])];
			if (bmh_st_record(&rv, &wr[q], &reg[roff[i] + k], reg_mapq[roff[i] + k], v.l_seq, cig, &alns[q])) die("a record was refused", i);
		}
	}
	for (i = 0; i < n; i += pe ? 2 : 1) {
		const int32_t *const wk[2] = {want_k + roff[i], pe ? want_k + roff[i + 1] : 0};
		const bmh_alnreg_t *const ra[2] = {reg + roff[i], pe ? reg + roff[i + 1] : 0};
		bmh_st_unit((int)hd[2], hd[3], pes, (int)pe, pe ? &pd[i >> 1] : 0, first + i, wk, ra, alns, plan + i);
	}
	for (i = 0; i < n; ++i) {
		const bmh_st_read_t v = view(pool, poff, (int)i);
		const int n_rec = (int)(first[i + 1] - first[i]);
		bmh_st_sink_t c = {0, 0, 0, 0, 0}, w, s;
		char *exact, *shorter;
		lines += bmh_st_read_text(&E, &c, &v, &plan[i], n_rec, alns + first[i]);
		if (c.err) die("the counting sink reports an error", i);
		if (c.l != toff[i + 1] - toff[i]) die("the counted size is not the host call's", i);
		if (!(exact = (char *)malloc(c.l ? (size_t)c.l : 1))) return 3;
		w.s = exact, w.l = 0, w.cap = c.l, w.err = 0, w.rsv_ = 0;
		bmh_st_read_text(&E, &w, &v, &plan[i], n_rec, alns + first[i]);
		if (w.err || w.l != c.l) die("the written size is not the counted size", i);
		if (memcmp(exact, text + toff[i], (size_t)c.l) != 0) die("the written bytes are not the host call's", i);
		free(exact);
		if (!(shorter = (char *)malloc((size_t)c.l))) return 3; /* (every read prints at least one line: c.l > 0) */
		shorter[c.l - 1] = 0x5a;
		s.s = shorter, s.l = 0, s.cap = c.l - 1, s.err = 0, s.rsv_ = 0;
		bmh_st_read_text(&E, &s, &v, &plan[i], n_rec, alns + first[i]);
		if (!s.err) die("a slice one byte short was not refused", i);
		if (shorter[c.l - 1] != 0x5a) die("the sink wrote past its end", i);
		if (c.l > 1 && memcmp(shorter, text + toff[i], 1) != 0) die("the short slice does not start with the text", i);
		free(shorter);
	}
	printf("ok %" PRId64 " %" PRId64 " %" PRId64 "\n", n, lines, toff[n]);
	free(ref), free(noff), free(names), free(pes), free(roff), free(first), free(n_want), free(want_k), free(reg_mapq), free(pd), free(reg), free(wr);
	free(cig), free(md), free(rg), free(poff), free(pool), free(toff), free(text), free(alns), free(plan);
	fclose(f);
	return 0;
}
