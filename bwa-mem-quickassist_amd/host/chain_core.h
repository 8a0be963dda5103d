/*
 * chain_core.h -- seeds to chains for one read: the one text of the chainer, compiled by gcc for bmh_chain_reads
 * (host/chain_batch.c) and by hipcc for the device's chain_kernel (csrc/chain.hip, one lane per read).
 *   smem_next2         reference bwa-0.7.8/bwamem.c:118-157  the rounds: a main call, merged in order with its re-seeding call (KEEP_SUB)
 *   mem_insert_seed    bwamem.c:208-243   every occurrence of every long, rare seed into klib's B-tree of chains (test_and_merge :186-206)
 *   mem_chain          bwamem.c:283-306   the in-order read-out
 *   mem_chain_flt      bwamem.c:319-380   (mem_chain_weight :245-263)
 * Two details decide the ORDER of the chains, which the extension stage and finally the SAM output depend on, and both are
 * reproduced literally:
 *   * chains with EQUAL keys: klib's B-tree (kbtree.h) puts a new key behind the first equal key of the leaf its descent ends
 *     in, and `kb_intervalp` returns the first equal key of the first node on its way down that has one -- both depend on how
 *     the tree has split so far.  So the tree is simulated node for node: nodes of 2t-1 = 15 keys (t from kb_init with
 *     KB_DEFAULT_SIZE = 512 bytes and 24-byte keys, kbtree.h:54-66), pre-emptive splitting on the way down (kbtree.h:176-212),
 *     the two-sided binary search of __kb_getp_aux (kbtree.h:122-135).
 *   * chains of EQUAL weight: mem_chain_flt orders them with klib's unstable introsort (sort_exact.h).
 * Nothing is allocated inside: the caller hands over an arena slice sized from the read's seed bound S_r (the positions of its
 * long and rare intervals).  Its chains are at most S_r, its nodes at most S_r/7 + 1 (every node but the root holds >= t-1 = 7
 * keys; one more slot is kept).  Nodes are addressed by 32-bit index; a chain keeps its first seed, its last seed and a linked
 * list of its seeds.  Every write is checked against the slice and every table read against the table (a caller's tables may
 * be inconsistent).  Under hipcc every routine is __host__ __device__ and always inlined; the C subset used (no references,
 * no vector types, no std::) is what lets gcc compile the same text.
 */
#ifndef BMH_CHAIN_CORE_H
#define BMH_CHAIN_CORE_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bwamem_hip.h"
#include "sort_exact.h"

#ifdef __HIPCC__
#define BMH_CC_HD __host__ __device__ __attribute__((always_inline))
#else
#define BMH_CC_HD
#endif

/* The filter's two (float)·(float) products.  Both builds round one IEEE single-precision product that a comparison then
 * reads: no addition follows that could be contracted into an FMA, and x86-64 evaluates float in float (FLT_EVAL_METHOD 0).
 * __fmul_rn only pins that rounding on the device, so both forms give the reference's result. */
#ifdef __HIP_DEVICE_COMPILE__
#define BMH_CC_FMUL(a, b) __fmul_rn((float)(a), (float)(b))
#else
#define BMH_CC_FMUL(a, b) ((float)(a) * (float)(b))
#endif

enum {
	BMH_CC_T = 8,                /* kb_init(chn, 512): t = ((512-4-8)/(8+24)+1)>>1 = 8 */
	BMH_CC_MAX = 2 * BMH_CC_T - 1, /* keys per node */
	BMH_CC_STK = 40              /* per read: entries of the walk stack (tree height <= 12 below 2^32 keys) and of the sort stack */
};
#define BMH_CC_MAX_SEEDS_PER_READ (1ull << 31)

typedef struct { /* one B-tree node, 256 bytes */
	int64_t pos[BMH_CC_MAX];
	int32_t cid[BMH_CC_MAX];
	int32_t child[BMH_CC_MAX + 1];
	int32_t n, internal;
} bmh_cc_node_t;
typedef char bmh_cc_node_layout[sizeof(bmh_cc_node_t) == 256 ? 1 : -1];

typedef struct { /* a chain: its first and last seed (indices into the read's seed slice), the seed count */
	int32_t first, last, n, rsv;
} bmh_cc_chn_t;

typedef struct { /* flt_aux_t of mem_chain_flt with indices for pointers; cid = the chain the record stands for */
	int32_t beg, end, w, cid, p, p2;
} bmh_cc_flt_t;

typedef struct __attribute__((aligned(8))) {
	int32_t x, y;
} bmh_cc_pair_t;

typedef struct { /* one read's slices */
	bmh_seed_t *seed;
	int32_t *next;
	bmh_cc_chn_t *chn;
	bmh_cc_flt_t *flt;
	bmh_cc_pair_t *ord;  /* after the filter: (chain, seed count) of the kept chains, best first */
	bmh_cc_node_t *node;
	bmh_cc_pair_t *walk; /* BMH_CC_STK entries */
	bmh_sort_stk_t *sstk; /* BMH_CC_STK entries */
	unsigned long long seed_cap, node_cap;
} bmh_cc_arena_t;

typedef struct { /* a batch's seeding tables (bmh_smem_batch's output form) and their sizes */
	const uint32_t *coff;
	const bmh_smem_call_t *calls;
	const uint64_t *ioff;
	const bmh_smem_intv_t *intv;
	const uint64_t *sa_off, *sa_pos;
	uint64_t n_calls, n_intv, n_pos; /* n_pos = UINT64_MAX: sa_pos is unbounded */
} bmh_cc_tables_t;

typedef struct { /* what bmh_cc_chain_read reports */
	uint32_t n_keys;          /* chains before the filter */
	uint32_t kept;            /* chains after it */
	unsigned long long seeds; /* seeds of the kept chains */
	int n_equal;              /* B-tree look-ups that met an equal key */
} bmh_cc_counts_t;

BMH_CC_HD static inline int bmh_cc_min(int a, int b) { return a < b ? a : b; }
BMH_CC_HD static inline int bmh_cc_max(int a, int b) { return a > b ? a : b; }
BMH_CC_HD static inline int bmh_cc_key_cmp(int64_t a, int64_t b) { return (b < a) - (a < b); } /* chain_cmp, bwamem.c:183 */

BMH_CC_HD static inline int bmh_cc_iv_len(const bmh_smem_intv_t *p) { return (int)((uint32_t)p->info - (uint32_t)(p->info >> 32)); }
/* a seed interval mem_insert_seed keeps: long and rare */
BMH_CC_HD static inline int bmh_cc_seeds_qualify(const bmh_chain_opt_t *o, const bmh_smem_intv_t *p)
{
	return bmh_cc_iv_len(p) >= o->min_seed_len && p->x[2] <= (uint64_t)o->max_occ;
}

/* S_r of read r (of length len): the positions of its long and rare intervals; 0 for a read too short to chain.
 * BMH_E_ARG (and *s = 0) when its interval range lies outside the table or S_r does not fit 31 bits. */
BMH_CC_HD static inline int bmh_cc_seed_bound(const bmh_chain_opt_t *o, const bmh_cc_tables_t *in, int r, int len, unsigned long long *s)
{
	uint64_t lo, hi, k;
	unsigned long long n = 0;
	*s = 0;
	if (len < o->min_seed_len) return 0;
	lo = in->ioff[r], hi = in->ioff[r + 1];
	if (lo > hi || hi > in->n_intv) return BMH_E_ARG;
	for (k = lo; k < hi; ++k)
		if (bmh_cc_seeds_qualify(o, &in->intv[k])) n += in->intv[k].x[2];
	if (n >= BMH_CC_MAX_SEEDS_PER_READ) return BMH_E_ARG;
	*s = n;
	return 0;
}
BMH_CC_HD static inline unsigned long long bmh_cc_node_bound(unsigned long long s) { return s ? s / 7 + 2 : 0; }

/* ---- the B-tree of chains ------------------------------------------------------------------------------------------ */
/* __kb_getp_aux, kbtree.h:122-135: the first key equal to k (*r = 0), else the last key below it (possibly -1; *r != 0) */
BMH_CC_HD static inline int bmh_cc_bt_find(const bmh_cc_node_t *x, int64_t k, int *r)
{
	int begin = 0, end = x->n;
	if (x->n == 0) return -1;
	while (begin < end) {
		const int mid = (begin + end) >> 1;
		if (bmh_cc_key_cmp(x->pos[mid], k) < 0) begin = mid + 1;
		else end = mid;
	}
	if (begin == x->n) {
		*r = 1;
		return x->n - 1;
	}
	if ((*r = bmh_cc_key_cmp(k, x->pos[begin])) < 0) --begin;
	return begin;
}

typedef struct {
	int root, n_keys, n_nodes;
} bmh_cc_tree_t;

BMH_CC_HD static inline int bmh_cc_bt_node(const bmh_cc_arena_t *A, bmh_cc_tree_t *b)
{
	bmh_cc_node_t *x;
	if ((unsigned long long)b->n_nodes >= A->node_cap) return -1;
	x = &A->node[b->n_nodes];
	x->n = 0, x->internal = 0;
	return b->n_nodes++;
}

/* kb_intervalp (kbtree.h:153-169), lower bound only: the chain at or below k (-1: none); *eq += 1 when that is an equal key */
BMH_CC_HD static inline int bmh_cc_bt_lower(const bmh_cc_arena_t *A, const bmh_cc_tree_t *b, int64_t k, int *eq)
{
	int xi = b->root, lower = -1;
	while (xi >= 0) {
		const bmh_cc_node_t *x = &A->node[xi];
		int r = 0;
		const int i = bmh_cc_bt_find(x, k, &r);
		if (i >= 0 && r == 0) {
			++*eq;
			return x->cid[i];
		}
		if (i >= 0) lower = x->cid[i];
		if (!x->internal) return lower;
		xi = x->child[i + 1];
	}
	return lower;
}

/* __kb_split, kbtree.h:176-192: child y = x->child[i] is full; its upper half moves to a new right sibling.  0: no node left */
BMH_CC_HD static inline int bmh_cc_bt_split(const bmh_cc_arena_t *A, bmh_cc_tree_t *b, int xi, int i, int yi)
{
	const int zi = bmh_cc_bt_node(A, b);
	bmh_cc_node_t *x, *y, *z;
	int k;
	if (zi < 0) return 0;
	x = &A->node[xi], y = &A->node[yi], z = &A->node[zi];
	z->internal = y->internal, z->n = BMH_CC_T - 1;
	for (k = 0; k < BMH_CC_T - 1; ++k) z->pos[k] = y->pos[BMH_CC_T + k], z->cid[k] = y->cid[BMH_CC_T + k];
	if (y->internal)
		for (k = 0; k < BMH_CC_T; ++k) z->child[k] = y->child[BMH_CC_T + k];
	y->n = BMH_CC_T - 1;
	for (k = x->n; k >= i + 1; --k) x->child[k + 1] = x->child[k];
	x->child[i + 1] = zi;
	for (k = x->n - 1; k >= i; --k) x->pos[k + 1] = x->pos[k], x->cid[k + 1] = x->cid[k];
	x->pos[i] = y->pos[BMH_CC_T - 1], x->cid[i] = y->cid[BMH_CC_T - 1];
	++x->n;
	return 1;
}

/* kb_putp / __kb_putp_aux, kbtree.h:193-227 (iterative: the recursion there is a plain descent).  0: no node left */
BMH_CC_HD static inline int bmh_cc_bt_put(const bmh_cc_arena_t *A, bmh_cc_tree_t *b, int64_t pos, int cid)
{
	bmh_cc_node_t *x;
	int xi, r, i, k;
	if (b->root < 0 && (b->root = bmh_cc_bt_node(A, b)) < 0) return 0;
	xi = b->root;
	++b->n_keys;
	if (A->node[xi].n == BMH_CC_MAX) { /* grow at the root */
		const int si = bmh_cc_bt_node(A, b);
		bmh_cc_node_t *s;
		if (si < 0) return 0;
		s = &A->node[si];
		s->internal = 1, s->n = 0, s->child[0] = xi;
		b->root = si;
		if (!bmh_cc_bt_split(A, b, si, 0, xi)) return 0;
		xi = si;
	}
	while (A->node[xi].internal) {
		x = &A->node[xi];
		i = bmh_cc_bt_find(x, pos, &r) + 1;
		if (A->node[x->child[i]].n == BMH_CC_MAX) {
			if (!bmh_cc_bt_split(A, b, xi, i, x->child[i])) return 0;
			if (bmh_cc_key_cmp(pos, x->pos[i]) > 0) ++i;
		}
		xi = x->child[i];
	}
	x = &A->node[xi];
	i = bmh_cc_bt_find(x, pos, &r);
	for (k = x->n - 1; k >= i + 1; --k) x->pos[k + 1] = x->pos[k], x->cid[k + 1] = x->cid[k];
	x->pos[i + 1] = pos, x->cid[i + 1] = cid;
	++x->n;
	return 1;
}

/* ---- bwamem.c:186-206: seed si (already in the read's seed slice) joins chain ci or not */
BMH_CC_HD static inline int bmh_cc_test_and_merge(const bmh_chain_opt_t *o, int64_t l_pac, const bmh_cc_arena_t *A, int ci, int si)
{
	bmh_cc_chn_t *c = &A->chn[ci];
	const bmh_seed_t f = A->seed[c->first], last = A->seed[c->last], p = A->seed[si];
	const int64_t qend = (int64_t)last.qbeg + last.len, rend = last.rbeg + last.len;
	int64_t x, y;
	if (p.qbeg >= f.qbeg && (int64_t)p.qbeg + p.len <= qend && p.rbeg >= f.rbeg && p.rbeg + p.len <= rend) return 1; /* contained */
	if ((last.rbeg < l_pac || f.rbeg < l_pac) && p.rbeg >= l_pac) return 0; /* other strand */
	x = (int64_t)p.qbeg - last.qbeg; /* never negative */
	y = p.rbeg - last.rbeg;
	if (y >= 0 && x - y <= o->w && y - x <= o->w && x - last.len < o->max_chain_gap && y - last.len < o->max_chain_gap) { /* grow */
		A->next[c->last] = si, A->next[si] = -1;
		c->last = si, ++c->n;
		return 1;
	}
	return 0; /* a new chain */
}

/* ---- bwamem.c:245-263 */
BMH_CC_HD static inline int bmh_cc_chain_weight(const bmh_cc_arena_t *A, const bmh_cc_chn_t *c)
{
	int64_t end = 0;
	int w = 0, tmp, s, j;
	for (s = c->first, j = 0; j < c->n; ++j, s = A->next[s]) {
		const bmh_seed_t sd = A->seed[s];
		if (sd.qbeg >= end) w += sd.len;
		else if ((int64_t)sd.qbeg + sd.len > end) w += (int)(sd.qbeg + sd.len - end);
		end = end > (int64_t)sd.qbeg + sd.len ? end : (int64_t)sd.qbeg + sd.len;
	}
	tmp = w;
	end = 0;
	for (s = c->first, j = 0; j < c->n; ++j, s = A->next[s]) { /* (the reference adds the second pass onto w and advances `end` on the QUERY, :256-261) */
		const bmh_seed_t sd = A->seed[s];
		if (sd.rbeg >= end) w += sd.len;
		else if (sd.rbeg + sd.len > end) w += (int)(sd.rbeg + sd.len - end);
		end = end > (int64_t)sd.qbeg + sd.len ? end : (int64_t)sd.qbeg + sd.len;
	}
	return w < tmp ? w : tmp;
}

/* flt_lt of mem_chain_flt: the heavier chain first.  hipcc takes it as a callable the sort inlines, gcc as a function. */
BMH_CC_HD static inline int bmh_cc_heavier(const void *a, const void *b) { return ((const bmh_cc_flt_t *)a)->w > ((const bmh_cc_flt_t *)b)->w; }
#ifdef __HIPCC__
struct bmh_cc_flt_lt {
	BMH_CC_HD int operator()(const void *a, const void *b) const { return bmh_cc_heavier(a, b); }
};
#define BMH_CC_FLT_LT bmh_cc_flt_lt()
#else
#define BMH_CC_FLT_LT bmh_cc_heavier
#endif

/* ---- one read: smem_next2's rounds, mem_insert_seed, the in-order walk and mem_chain_flt.  The kept chains stay in the
 * arena, best first, as ord[k] = (chain, seed count) for k < kept.  0, or BMH_E_ARG: inconsistent tables or a slice too small. */
BMH_CC_HD static inline int bmh_cc_chain_read(const bmh_chain_opt_t *o, int64_t l_pac, const bmh_cc_tables_t *in, int r, int len,
                                              const bmh_cc_arena_t *A, bmh_cc_counts_t *cnt)
{
	uint32_t c, c_lo, c_hi;
	uint64_t i_lo, i_hi, n_iv;
	const bmh_smem_intv_t *iv;
	bmh_cc_tree_t bt;
	int split_len, n_seeds = 0, n_eq = 0, n_chn, n, kept, i;
	unsigned long long n_out_seeds = 0;
	cnt->n_keys = 0, cnt->kept = 0, cnt->seeds = 0, cnt->n_equal = 0;
	if (len < o->min_seed_len) return 0; /* bwamem.c:291 */
	c_lo = in->coff[r], c_hi = in->coff[r + 1], i_lo = in->ioff[r], i_hi = in->ioff[r + 1];
	if (c_lo > c_hi || c_hi > in->n_calls || i_lo > i_hi || i_hi > in->n_intv) return BMH_E_ARG;
	iv = in->intv + i_lo, n_iv = i_hi - i_lo;
	split_len = bmh_cc_min(o->split_len, len); /* bwamem.c:213 */
	bt.root = -1, bt.n_keys = 0, bt.n_nodes = 0;
	c = c_lo;
	while (c < c_hi) { /* one smem_next2 round per main bwt_smem1 call */
		const bmh_smem_call_t mc = in->calls[c++];
		const bmh_smem_intv_t *m, *s = 0;
		int max = 0, max_i = 0, sn = 0, j = 0;
		if (mc.n < 0 || (uint64_t)mc.first + (uint64_t)mc.n > n_iv) return BMH_E_ARG;
		m = iv + mc.first;
		for (i = 0; i < mc.n; ++i) /* the longest match, bwamem.c:130-134 */
			if (max < bmh_cc_iv_len(&m[i])) max = bmh_cc_iv_len(&m[i]), max_i = i;
		if (mc.n > 0 && split_len > 0 && max >= split_len && m[max_i].x[2] <= (uint64_t)o->split_width) {
			/* long and rare: its middle was searched again with a higher occurrence floor (bwamem.c:135-155); that call is the
			 * next record */
			bmh_smem_call_t sc;
			if (c >= c_hi) return BMH_E_ARG;
			sc = in->calls[c++];
			if (sc.x != (int)(((uint32_t)m[max_i].info + (uint32_t)(m[max_i].info >> 32)) >> 1) || sc.min_intv != (int)(m[max_i].x[2] + 1) ||
			    sc.n < 0 || (uint64_t)sc.first + (uint64_t)sc.n > n_iv)
				return BMH_E_ARG; /* the call list does not follow smem_next2's order */
			s = iv + sc.first, sn = sc.n;
		}
		/* the round's intervals: the main call's, or its ordered merge by (start, len - end) with the re-seeding call's
		 * (KEEP_SUB), produced one at a time */
		i = 0;
		for (;;) {
			const bmh_smem_intv_t *p;
			bmh_smem_intv_t P;
			uint64_t so, kk;
			int slen;
			if (!s) {
				if (i >= mc.n) break;
				p = &m[i++];
			} else {
				int take_m;
				if (i < mc.n && j < sn) {
					const int64_t xi = (int64_t)(m[i].info >> 32 << 32 | (uint64_t)(uint32_t)(len - (int)(uint32_t)m[i].info));
					const int64_t xj = (int64_t)(s[j].info >> 32 << 32 | (uint64_t)(uint32_t)(len - (int)(uint32_t)s[j].info));
					take_m = xi < xj;
				} else if (i < mc.n) take_m = 1;
				else if (j < sn) take_m = 0;
				else break;
				if (take_m) p = &m[i++];
				else {
					const bmh_smem_intv_t *q = &s[j++];
					if (!(bmh_cc_iv_len(q) >= max >> 1 && (int)(uint32_t)q->info > mc.x)) continue; /* KEEP_SUB */
					p = q;
				}
			}
			/* mem_insert_seed's loop body, bwamem.c:216-240 */
			P = *p;
			slen = bmh_cc_iv_len(&P);
			if (!bmh_cc_seeds_qualify(o, &P)) continue;
			so = in->sa_off[i_lo + (uint64_t)(p - iv)];
			if (so == UINT64_MAX || so > in->n_pos || P.x[2] > in->n_pos - so) return BMH_E_ARG; /* the table must cover the interval */
			for (kk = 0; kk < P.x[2]; ++kk) {
				bmh_seed_t sd;
				int si, lower;
				sd.rbeg = (int64_t)in->sa_pos[so + kk];
				sd.qbeg = (int32_t)(P.info >> 32), sd.len = slen;
				if (sd.rbeg < l_pac && l_pac < sd.rbeg + sd.len) continue; /* bridges the strands */
				if ((unsigned long long)n_seeds >= A->seed_cap) return BMH_E_ARG;
				si = n_seeds++;
				A->seed[si] = sd, A->next[si] = -1;
				lower = bt.n_keys ? bmh_cc_bt_lower(A, &bt, sd.rbeg, &n_eq) : -1;
				if (lower < 0 || !bmh_cc_test_and_merge(o, l_pac, A, lower, si)) { /* a new chain (chains are numbered in creation order) */
					const int ci = bt.n_keys;
					A->chn[ci].first = si, A->chn[ci].last = si, A->chn[ci].n = 1, A->chn[ci].rsv = 0;
					if (!bmh_cc_bt_put(A, &bt, sd.rbeg, ci)) return BMH_E_ARG;
				}
			}
		}
	}
	n_chn = bt.n_keys;
	cnt->n_keys = (uint32_t)n_chn, cnt->n_equal = n_eq;
	if (n_chn == 0) return 0;
	{ /* the in-order walk (__kb_traverse): child 0, key 0, child 1, ... key n-1, child n.  Stack entry (node, i): the next key
	   * of the node is i and everything left of it has been emitted. */
		int top = -1, k = 0, x;
		for (x = bt.root;; x = A->node[x].child[0]) {
			if (top + 1 >= BMH_CC_STK) return BMH_E_ARG;
			++top, A->walk[top].x = x, A->walk[top].y = 0;
			if (!A->node[x].internal) break;
		}
		while (top >= 0) {
			const bmh_cc_pair_t e = A->walk[top];
			const bmh_cc_node_t *nd = &A->node[e.x];
			if (e.y >= nd->n) {
				--top;
				continue;
			}
			A->flt[k++].cid = nd->cid[e.y];
			A->walk[top].y = e.y + 1;
			if (nd->internal)
				for (x = nd->child[e.y + 1];; x = A->node[x].child[0]) {
					if (top + 1 >= BMH_CC_STK) return BMH_E_ARG;
					++top, A->walk[top].x = x, A->walk[top].y = 0;
					if (!A->node[x].internal) break;
				}
		}
	}
	n = n_chn;
	if (n_chn > 1) { /* mem_chain_flt, bwamem.c:319-380 */
		int jj;
		for (i = 0; i < n_chn; ++i) {
			bmh_cc_flt_t *f = &A->flt[i];
			const bmh_cc_chn_t ch = A->chn[f->cid];
			const bmh_seed_t last = A->seed[ch.last];
			f->beg = A->seed[ch.first].qbeg, f->end = last.qbeg + last.len, f->w = bmh_cc_chain_weight(A, &ch), f->p = 0, f->p2 = -1;
		}
		bmh_sort_exact_stk(A->flt, (size_t)n_chn, sizeof(bmh_cc_flt_t), BMH_CC_FLT_LT, A->sstk);
		for (i = 0; i < n_chn; ++i) A->ord[i].x = A->flt[i].cid, A->ord[i].y = 0, A->flt[i].p = i; /* best chain first */
		for (i = 1, n = 1; i < n_chn; ++i) {
			const bmh_cc_flt_t ai = A->flt[i];
			for (jj = 0; jj < n; ++jj) {
				bmh_cc_flt_t *aj = &A->flt[jj];
				const int b_max = bmh_cc_max(aj->beg, ai.beg), e_min = bmh_cc_min(aj->end, ai.end);
				if (e_min > b_max) { /* overlap on the query */
					const int min_l = bmh_cc_min(ai.end - ai.beg, aj->end - aj->beg);
					if ((float)(e_min - b_max) >= BMH_CC_FMUL(min_l, o->mask_level)) { /* significant */
						if (aj->p2 < 0) aj->p2 = ai.p;
						if ((float)ai.w < BMH_CC_FMUL(aj->w, o->chain_drop_ratio) && aj->w - ai.w >= o->min_seed_len << 1) break;
					}
				}
			}
			if (jj == n) A->flt[n++] = ai; /* not shadowed by a better chain */
		}
		for (i = 0; i < n; ++i) { /* kept: the survivors and, for each, the first chain it shadows */
			A->ord[A->flt[i].p].y = 1;
			if (A->flt[i].p2 >= 0) A->ord[A->flt[i].p2].y = 1;
		}
	} else A->ord[0].x = A->flt[0].cid, A->ord[0].y = 1;
	/* the kept chains, best first: ord[k] = (chain, seed count), compacted in place (k <= i) */
	kept = 0;
	for (i = 0; i < n_chn; ++i) {
		const bmh_cc_pair_t e = A->ord[i];
		if (!e.y) continue;
		A->ord[kept].x = e.x, A->ord[kept].y = A->chn[e.x].n;
		++kept;
		n_out_seeds += (unsigned long long)A->chn[e.x].n;
	}
	cnt->kept = (uint32_t)kept, cnt->seeds = n_out_seeds;
	return 0;
}

/* The kept chains of a read in compact form: out_n[k] = seed count of the k-th, their seeds back to back in out_seed. */
BMH_CC_HD static inline void bmh_cc_gather(const bmh_cc_arena_t *A, uint32_t kept, uint32_t *out_n, bmh_seed_t *out_seed)
{
	uint32_t k;
	int s, j;
	for (k = 0; k < kept; ++k) {
		const bmh_cc_pair_t e = A->ord[k];
		out_n[k] = (uint32_t)e.y;
		for (s = A->chn[e.x].first, j = 0; j < e.y; ++j, s = A->next[s]) *out_seed++ = A->seed[s];
	}
}

/* ---- host side: compact form -> mem_chain's return form ---------------------------------------------------------- */
/* Frees every read's chains and leaves each {0, 0, NULL}. */
static inline void bmh_cc_release(int n_reads, bmh_chain_v *chains)
{
	int r;
	size_t k;
	for (r = 0; r < n_reads; ++r) {
		for (k = 0; k < chains[r].n; ++k) free(chains[r].a[k].seeds);
		free(chains[r].a);
		chains[r].n = chains[r].m = 0, chains[r].a = 0;
	}
}

/* One read's kept chains into *v (empty on entry): a[] sized for its n_keys chains before the filter, seed arrays of
 * capacity 4, 8, 16, ... as test_and_merge grows them.  BMH_E_NOMEM: *v holds the chains made so far (bmh_cc_release). */
static inline int bmh_cc_emit(uint32_t n_keys, uint32_t kept, const uint32_t *cn, const bmh_seed_t *sd, bmh_chain_v *v)
{
	uint32_t k;
	if (!n_keys) return 0;
	if (!(v->a = (bmh_chain_t *)malloc(sizeof(bmh_chain_t) * n_keys))) return BMH_E_NOMEM;
	v->m = n_keys;
	for (k = 0; k < kept; ++k) {
		bmh_chain_t *c = &v->a[k];
		c->n = (int)cn[k];
		for (c->m = 4; c->m < c->n; c->m <<= 1) {}
		if (!(c->seeds = (bmh_seed_t *)malloc(sizeof(bmh_seed_t) * (size_t)c->m))) return BMH_E_NOMEM;
		memcpy(c->seeds, sd, sizeof(bmh_seed_t) * (size_t)c->n);
		c->pos = c->seeds[0].rbeg;
		sd += c->n;
		v->n = k + 1;
	}
	return 0;
}

#endif
