/* decide_core_main.c -- host/postproc_core.h driven as the device kernel of csrc/decide.hip drives it, one unit (read or pair) at a
 * time, with every vector, z[] list, v[] key array, range stack and output in a heap block of exactly its size, so that a build
 * under -fsanitize=address,undefined sees any access past what the core was promised.
 * Input (tests/test_decide_cpu.py writes it): int32 cases; per case bmh_sam_opt_t, bmh_pestat_t[4], int64 l_pac, int64 id0, int32 n,
 * int32 0, then n times { int32 count, count bmh_alnreg_t }.
 * Output: per case "case <i>", then per read "R <i> <hex of its regions>", "M <i> <hex of reg_mapq>", "W <i> <n_want> <hex of want_k>"
 * and per pair "P <p> <hex of bmh_pairdec_t>". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bwa-mem-quickassist_amd/host/postproc_core.h"

static void hex(const void *p, size_t n)
{
	const unsigned char *b = (const unsigned char *)p;
	size_t i;
	for (i = 0; i < n; ++i) printf("%02x", b[i]);
}
static void *block(size_t bytes) /* exactly `bytes`, filled with 0xff */
{
	void *p = malloc(bytes);
	if (!p) exit(3);
	memset(p, 0xff, bytes);
	return p;
}
static void need(int ok) { if (!ok) { fprintf(stderr, "short input\n"); exit(2); } }

int main(int argc, char **argv)
{
	FILE *f;
	int32_t n_cases, c;
	if (argc != 2 || !(f = fopen(argv[1], "rb"))) return 2;
	need(fread(&n_cases, 4, 1, f) == 1);
	for (c = 0; c < n_cases; ++c) {
		bmh_sam_opt_t o;
		bmh_pestat_t pes[4];
		int64_t l_pac, id0;
		int32_t n, pad, i, r;
		bmh_alnreg_t **a;
		int32_t *cnt;
		need(fread(&o, sizeof(o), 1, f) == 1 && fread(pes, sizeof(pes), 1, f) == 1 && fread(&l_pac, 8, 1, f) == 1 && fread(&id0, 8, 1, f) == 1);
		need(fread(&n, 4, 1, f) == 1 && fread(&pad, 4, 1, f) == 1);
		a = (bmh_alnreg_t **)block(sizeof(*a) * (size_t)(n + 1)), cnt = (int32_t *)block(4 * (size_t)(n + 1));
		for (i = 0; i < n; ++i) {
			need(fread(&cnt[i], 4, 1, f) == 1);
			a[i] = (bmh_alnreg_t *)block(sizeof(bmh_alnreg_t) * (size_t)cnt[i]);
			need(fread(a[i], sizeof(bmh_alnreg_t), (size_t)cnt[i], f) == (size_t)cnt[i]);
		}
		printf("case %d\n", c);
		for (i = 0; i < n; i += (o.flag & BMH_MEM_F_PE) ? 2 : 1) {
			const int pe = (o.flag & BMH_MEM_F_PE) != 0, nr = pe ? 2 : 1;
			const int nn[2] = {cnt[i], pe ? cnt[i + 1] : 0};
			bmh_alnreg_t *const aa[2] = {a[i], pe ? a[i + 1] : 0};
			int *const z[2] = {(int *)block(sizeof(int) * (size_t)nn[0]), (int *)block(sizeof(int) * (size_t)nn[1])};
			int32_t *const mq[2] = {(int32_t *)block(4 * (size_t)nn[0]), (int32_t *)block(4 * (size_t)nn[1])};
			int32_t *const wk[2] = {(int32_t *)block(4 * (size_t)nn[0]), (int32_t *)block(4 * (size_t)nn[1])};
			bmh_pair64_t *v = (bmh_pair64_t *)block(sizeof(bmh_pair64_t) * (size_t)(nn[0] + nn[1]));
			bmh_sort_stk_t *stk = (bmh_sort_stk_t *)block(sizeof(bmh_sort_stk_t) * bmh_sort_stack_len((size_t)(nn[0] + nn[1])));
			bmh_pairdec_t *d = (bmh_pairdec_t *)block(sizeof(*d));
			int32_t nw[2] = {-1, -1};
			if (pe) bmh_pp_unit_pe(&o, l_pac, pes, 0, (uint64_t)(id0 >> 1) + (uint64_t)(i >> 1), nn, aa, z, v, stk, d, mq, nw, wk);
			else bmh_pp_unit_se(&o, 0, id0 + i, nn[0], aa[0], z[0], stk, mq[0], &nw[0], wk[0]);
			for (r = 0; r < nr; ++r) {
				printf("R %d ", i + r), hex(aa[r], sizeof(bmh_alnreg_t) * (size_t)nn[r]), printf("\n");
				printf("M %d ", i + r), hex(mq[r], 4 * (size_t)nn[r]), printf("\n");
				printf("W %d %d ", i + r, nw[r]), hex(wk[r], 4 * (size_t)nn[r]), printf("\n");
			}
			if (pe) printf("P %d ", i >> 1), hex(d, sizeof(*d)), printf("\n");
			for (r = 0; r < 2; ++r) free(z[r]), free(mq[r]), free(wk[r]);
			free(v), free(stk), free(d);
		}
		for (i = 0; i < n; ++i) free(a[i]);
		free(a), free(cnt);
	}
	fclose(f);
	return 0;
}
