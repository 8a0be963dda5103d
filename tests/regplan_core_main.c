/* regplan_core_main.c -- host/regplan_core.h driven as the planning kernels of csrc/wanted.hip drive it, one routine at a time, with
 * the sequence table and every CIGAR in a heap block of exactly its size, so that a build under -fsanitize=address,undefined sees any
 * access past what the core was promised and any signed overflow in its arithmetic.
 * Input (tests/test_wanted_cpu.py writes it), one case per line:
 *   R n_seqs l_pac off len ...                          the sequence table the following P and X lines use
 *   P pos_f                                          -> "P rid"
 *   X rb re                                          -> "X verdict cb ce"        (cb ce as 0 0 unless the verdict is 1)
 *   C qb qe rb re cb ce n_cigar word ...             -> "C verdict qb qe rb re"
 *   B ql tl truesc reg_w a mat0 o_del e_del o_ins e_ins w -> "B w2 band*3 slot*3 n_tasks cap" and the emitted record and tasks in hex */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/regplan_core.h"

static void hex(const void *p, size_t n)
{
	const unsigned char *b = (const unsigned char *)p;
	size_t i;
	for (i = 0; i < n; ++i) printf("%02x", b[i]);
}
static void *block(size_t bytes) /* exactly `bytes`, filled with 0xff */
{
	void *p = malloc(bytes ? bytes : 1);
	if (!p) exit(3);
	memset(p, 0xff, bytes);
	return p;
}
static void need(int ok) { if (!ok) { fprintf(stderr, "short input\n"); exit(2); } }

int main(int argc, char **argv)
{
	FILE *f;
	bmh_refspan_t *ref = 0;
	bmh_rp_refv_t rv;
	char op[4];
	memset(&rv, 0, sizeof(rv));
	if (argc != 2 || !(f = fopen(argv[1], "r"))) return 2;
	while (fscanf(f, "%3s", op) == 1) {
		if (op[0] == 'R') {
			int n, i;
			int64_t l_pac;
			need(fscanf(f, "%d %" SCNd64, &n, &l_pac) == 2 && n > 0);
			free(ref);
			ref = (bmh_refspan_t *)block(sizeof(*ref) * (size_t)n);
			for (i = 0; i < n; ++i) need(fscanf(f, "%" SCNd64 " %d", &ref[i].offset, &ref[i].len) == 2);
			rv.off0 = &ref[0].offset, rv.len0 = &ref[0].len, rv.stride = sizeof(*ref), rv.n_seqs = n, rv.l_pac = l_pac;
		} else if (op[0] == 'P') {
			int64_t pos;
			need(ref && fscanf(f, "%" SCNd64, &pos) == 1);
			printf("P %d\n", bmh_rp_pos2rid(&rv, pos));
		} else if (op[0] == 'X') {
			int64_t rb, re, cb = 0, ce = 0;
			int v;
			need(ref && fscanf(f, "%" SCNd64 " %" SCNd64, &rb, &re) == 2);
			v = bmh_rp_xref_test(&rv, rb, re, &cb, &ce);
			if (v != 1) cb = ce = 0;
			printf("X %d %" PRId64 " %" PRId64 "\n", v, cb, ce);
		} else if (op[0] == 'C') {
			int32_t qb, qe;
			int64_t rb, re, cb, ce;
			int n, i, v;
			uint32_t *cig;
			need(fscanf(f, "%d %d %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %d", &qb, &qe, &rb, &re, &cb, &ce, &n) == 7 && n >= 0);
			cig = (uint32_t *)block(4 * (size_t)n);
			for (i = 0; i < n; ++i) need(fscanf(f, "%" SCNu32, &cig[i]) == 1);
			v = bmh_rp_xref_cut(n, cig, cb, ce, &qb, &qe, &rb, &re);
			printf("C %d %d %d %" PRId64 " %" PRId64 "\n", v, qb, qe, rb, re);
			free(cig);
		} else if (op[0] == 'B') {
			bmh_rp_opt_t o;
			bmh_rp_plan_t pl;
			int ql, tl, truesc, reg_w;
			bmh_region_req_t *q = (bmh_region_req_t *)block(sizeof(*q));
			bmh_glb_task_t *t;
			need(fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d", &ql, &tl, &truesc, &reg_w, &o.a, &o.mat0, &o.o_del, &o.e_del, &o.o_ins, &o.e_ins, &o.w) == 11);
			bmh_rp_plan(&o, ql, tl, truesc, reg_w, &pl);
			printf("B %d %d %d %d %d %d %d %d %u ", bmh_rp_first_band(&o, ql, tl, truesc, reg_w), pl.band[0], pl.band[1], pl.band[2], pl.slot[0], pl.slot[1],
			       pl.slot[2], pl.n_tasks, pl.cap);
			t = (bmh_glb_task_t *)block(sizeof(*t) * (size_t)pl.n_tasks); /* exactly the tasks the plan counts */
			bmh_rp_emit(&pl, 1000, 77, 5000, ql, tl, truesc, 10, 240, q, t);
			hex(q, sizeof(*q)), printf(" "), hex(t, sizeof(*t) * (size_t)pl.n_tasks), printf("\n");
			free(q), free(t);
		} else need(0);
	}
	free(ref);
	fclose(f);
	return 0;
}
