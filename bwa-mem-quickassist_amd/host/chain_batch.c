/*
 * chain_batch.c -- seeds to chains on the host (plain C, above the C-ABI): the rest of SURVEY.md §8(f) row 3.
 *
 * For a batch of reads whose FM-index queries were answered by bmh_smem_batch / bmh_sa_batch, bmh_chain_reads runs
 * smem_next2's rounds, mem_insert_seed, mem_chain and mem_chain_flt (reference bwa-0.7.8/bwamem.c:118-380) read by read.
 * The chainer itself is host/chain_core.h, the same text the device's chain_kernel runs (csrc/chain.hip); this file is
 * its host driver: one arena for the whole call, grown to the largest read's bounds, and the kept chains handed back in
 * mem_chain's return form.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/bwamem_hip.h"
#include "chain_core.h"

/* The suffix-array entries chaining will ask for (bwamem.c:218-225): every occurrence of every interval that is long
 * and rare enough -- taken over ALL intervals the batch returned, a superset of the merged lists that are walked.
 * sa_off[k] = index of interval k's first entry in the key list (and later in the position list), or UINT64_MAX for an
 * interval that is never looked up; keys (nullable: count only) receives x[0] + j for j < x[2].  Returns the key count. */
uint64_t bmh_chain_sa_keys(const bmh_chain_opt_t *o, uint64_t n_intv, const bmh_smem_intv_t *intv, uint64_t *sa_off, uint64_t *keys)
{
	uint64_t k, n = 0;
	for (k = 0; k < n_intv; ++k) {
		const bmh_smem_intv_t *p = &intv[k];
		if (bmh_cc_seeds_qualify(o, p)) {
			uint64_t j;
			if (sa_off) sa_off[k] = n;
			if (keys)
				for (j = 0; j < p->x[2]; ++j) keys[n + j] = p->x[0] + j;
			n += p->x[2];
		} else if (sa_off) sa_off[k] = UINT64_MAX;
	}
	return n;
}

/* Grows the call's arena (and the compact buffers bmh_cc_gather fills) to hold a read of seed bound s. */
static int arena_fit(bmh_cc_arena_t *A, void **mem, uint32_t **cn, bmh_seed_t **cs, unsigned long long s)
{
	const unsigned long long nodes = bmh_cc_node_bound(s);
	size_t sz;
	char *p;
	if (s <= A->seed_cap && nodes <= A->node_cap) return BMH_OK;
	sz = nodes * sizeof(bmh_cc_node_t) + BMH_CC_STK * (sizeof(bmh_sort_stk_t) + sizeof(bmh_cc_pair_t)) +
	     s * (2 * sizeof(bmh_seed_t) + sizeof(bmh_cc_pair_t) + sizeof(bmh_cc_chn_t) + sizeof(bmh_cc_flt_t) + 2 * sizeof(uint32_t));
	free(*mem);
	if (!(*mem = p = (char *)malloc(sz))) {
		memset(A, 0, sizeof(*A));
		return BMH_E_NOMEM;
	}
	/* 8-byte records first */
	A->node = (bmh_cc_node_t *)p, p += nodes * sizeof(bmh_cc_node_t);
	A->sstk = (bmh_sort_stk_t *)p, p += BMH_CC_STK * sizeof(bmh_sort_stk_t);
	A->walk = (bmh_cc_pair_t *)p, p += BMH_CC_STK * sizeof(bmh_cc_pair_t);
	A->seed = (bmh_seed_t *)p, p += s * sizeof(bmh_seed_t);
	*cs = (bmh_seed_t *)p, p += s * sizeof(bmh_seed_t);
	A->ord = (bmh_cc_pair_t *)p, p += s * sizeof(bmh_cc_pair_t);
	A->chn = (bmh_cc_chn_t *)p, p += s * sizeof(bmh_cc_chn_t);
	A->flt = (bmh_cc_flt_t *)p, p += s * sizeof(bmh_cc_flt_t);
	A->next = (int32_t *)p, p += s * sizeof(int32_t);
	*cn = (uint32_t *)p;
	A->seed_cap = s, A->node_cap = nodes;
	return BMH_OK;
}

int bmh_chain_reads(const bmh_chain_opt_t *o, int64_t l_pac, int n_reads, const bmh_read_t *reads, const uint32_t *call_off,
                    const bmh_smem_call_t *calls, const uint64_t *intv_off, const bmh_smem_intv_t *intv, const uint64_t *sa_off,
                    const uint64_t *sa_pos, bmh_chain_v *chains)
{
	bmh_cc_arena_t A;
	bmh_cc_tables_t t;
	void *mem = 0;
	uint32_t *cn = 0;
	bmh_seed_t *cs = 0;
	int r, rc = BMH_OK;
	if (!o || n_reads < 0 || (n_reads > 0 && (!reads || !call_off || !calls || !intv_off || !intv || !sa_off || !sa_pos || !chains))) return BMH_E_ARG;
	for (r = 0; r < n_reads; ++r) chains[r].n = chains[r].m = 0, chains[r].a = 0;
	if (n_reads == 0) return BMH_OK;
	memset(&A, 0, sizeof(A));
	t.coff = call_off, t.calls = calls, t.ioff = intv_off, t.intv = intv, t.sa_off = sa_off, t.sa_pos = sa_pos;
	t.n_calls = call_off[n_reads], t.n_intv = intv_off[n_reads], t.n_pos = UINT64_MAX;
	for (r = 0; r < n_reads; ++r) {
		bmh_cc_counts_t cnt;
		unsigned long long s;
		if ((rc = bmh_cc_seed_bound(o, &t, r, reads[r].l_seq, &s)) || (rc = arena_fit(&A, &mem, &cn, &cs, s)) ||
		    (rc = bmh_cc_chain_read(o, l_pac, &t, r, reads[r].l_seq, &A, &cnt)))
			break;
		bmh_cc_gather(&A, cnt.kept, cn, cs);
		if ((rc = bmh_cc_emit(cnt.n_keys, cnt.kept, cn, cs, &chains[r]))) break;
	}
	free(mem);
	if (rc) bmh_cc_release(n_reads, chains);
	return rc;
}
