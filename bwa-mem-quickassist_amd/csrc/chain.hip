// chain.hip -- seeds to chains on the device (last slice): what host/chain_batch.c's bmh_chain_reads does,
// one lane per read, over the per-read seeding tables as bmh_seed_batch holds them on the device (smem_order_* + sa_of_intervals_kernel).
//   smem_next2         reference bwa-0.7.8/bwamem.c:118-157  the rounds: a main call, merged in order with its re-seeding call (KEEP_SUB)
//   mem_insert_seed    bwamem.c:208-243   every occurrence of every long, rare seed into klib's B-tree of chains (test_and_merge :186-206)
//   mem_chain          bwamem.c:283-306   the in-order read-out
//   mem_chain_flt      bwamem.c:319-380   (mem_chain_weight :245-263)
// Equal keys decide the output order (see host/chain_batch.c), so the B-tree is simulated node for node: same node size (t = 8, 15
// keys), pre-emptive splits, two-sided binary search, first equal key of the first node on the way down.  Its nodes live in a per-read
// arena slice and are addressed by 32-bit index; a chain keeps its first seed, its last seed and a linked list of its seeds.  The
// equal-weight order of mem_chain_flt comes from host/sort_exact.h itself, compiled for the device.
// Sizes are known before the launch: a read's seeds are at most the positions of its long and rare intervals (S_r), its chains at most
// S_r, its nodes at most S_r/7 + 1 (every node but the root holds >= t-1 = 7 keys).  Each read gets arena slices from the prefix sums of
// those bounds, and every write is checked against its slice anyway (a caller's tables may be inconsistent): no overflow, no retry.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bmh_ctx.h"
#include "bmh_device.h"
#include "../host/sort_exact.h"

namespace bmh {

namespace {

constexpr int kT = 8, kMax = 2 * kT - 1; // kb_init(chn, 512): t = 8, nodes of 15 keys
constexpr int kStk = 40;                 // per read: entries of the walk stack (tree height <= 12 below 2^32 keys) and of the sort stack
constexpr unsigned long long kMaxSeedsPerRead = 1ull << 31;

struct Node { // one B-tree node, 256 bytes
	int64_t pos[kMax];
	int32_t cid[kMax];
	int32_t child[kMax + 1];
	int32_t n, internal;
};
static_assert(sizeof(Node) == 256, "node layout");

struct Chn { // a chain: its first and last seed (indices into the read's seed slice), the seed count
	int32_t first, last, n, rsv;
};

struct Flt { // flt_aux_t of mem_chain_flt with indices for pointers; cid = the chain the record stands for
	int32_t beg, end, w, cid, p, p2;
};

struct FltLt { // flt_lt of chain_batch.c: the heavier chain first
	__device__ __forceinline__ int operator()(const void *a, const void *b) const { return ((const Flt *)a)->w > ((const Flt *)b)->w; }
};

__device__ __forceinline__ int key_cmp(int64_t a, int64_t b) { return (b < a) - (a < b); }

// __kb_getp_aux, kbtree.h:122-135
__device__ __forceinline__ int bt_find(const Node *x, int64_t k, int *r)
{
	int begin = 0, end = x->n;
	if (x->n == 0) return -1;
	while (begin < end) {
		const int mid = (begin + end) >> 1;
		if (key_cmp(x->pos[mid], k) < 0) begin = mid + 1;
		else end = mid;
	}
	if (begin == x->n) {
		*r = 1;
		return x->n - 1;
	}
	if ((*r = key_cmp(k, x->pos[begin])) < 0) --begin;
	return begin;
}

struct Arena { // one read's slices
	bmh_seed_t *seed;
	int32_t *next;
	Chn *chn;
	Flt *flt;
	int2 *ord;
	Node *node;
	int2 *walk;
	bmh_sort_stk_t *sstk;
	unsigned long long seed_cap, node_cap;
};

struct Tree {
	int root, n_keys, n_nodes;
};

__device__ __forceinline__ int bt_node(const Arena &A, Tree &b)
{
	if ((unsigned long long)b.n_nodes >= A.node_cap) return -1;
	Node *x = &A.node[b.n_nodes];
	x->n = 0, x->internal = 0;
	return b.n_nodes++;
}

// kb_intervalp, lower bound only: the chain at or below k (-1: none); *eq += 1 when that is an equal key
__device__ int bt_lower(const Arena &A, const Tree &b, int64_t k, int *eq)
{
	int xi = b.root, lower = -1;
	while (xi >= 0) {
		const Node *x = &A.node[xi];
		int r = 0;
		const int i = bt_find(x, k, &r);
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

// __kb_split, kbtree.h:176-192
__device__ bool bt_split(const Arena &A, Tree &b, int xi, int i, int yi)
{
	const int zi = bt_node(A, b);
	if (zi < 0) return false;
	Node *x = &A.node[xi], *y = &A.node[yi], *z = &A.node[zi];
	z->internal = y->internal, z->n = kT - 1;
	for (int k = 0; k < kT - 1; ++k) z->pos[k] = y->pos[kT + k], z->cid[k] = y->cid[kT + k];
	if (y->internal)
		for (int k = 0; k < kT; ++k) z->child[k] = y->child[kT + k];
	y->n = kT - 1;
	for (int k = x->n; k >= i + 1; --k) x->child[k + 1] = x->child[k];
	x->child[i + 1] = zi;
	for (int k = x->n - 1; k >= i; --k) x->pos[k + 1] = x->pos[k], x->cid[k + 1] = x->cid[k];
	x->pos[i] = y->pos[kT - 1], x->cid[i] = y->cid[kT - 1];
	++x->n;
	return true;
}

// kb_putp / __kb_putp_aux, kbtree.h:193-227
__device__ bool bt_put(const Arena &A, Tree &b, int64_t pos, int cid)
{
	if (b.root < 0 && (b.root = bt_node(A, b)) < 0) return false;
	int xi = b.root;
	++b.n_keys;
	if (A.node[xi].n == kMax) { // grow at the root
		const int si = bt_node(A, b);
		if (si < 0) return false;
		Node *s = &A.node[si];
		s->internal = 1, s->n = 0, s->child[0] = xi;
		b.root = si;
		if (!bt_split(A, b, si, 0, xi)) return false;
		xi = si;
	}
	while (A.node[xi].internal) {
		Node *x = &A.node[xi];
		int r, i = bt_find(x, pos, &r) + 1;
		if (A.node[x->child[i]].n == kMax) {
			if (!bt_split(A, b, xi, i, x->child[i])) return false;
			if (key_cmp(pos, x->pos[i]) > 0) ++i;
		}
		xi = x->child[i];
	}
	Node *x = &A.node[xi];
	int r;
	const int i = bt_find(x, pos, &r);
	for (int k = x->n - 1; k >= i + 1; --k) x->pos[k + 1] = x->pos[k], x->cid[k + 1] = x->cid[k];
	x->pos[i + 1] = pos, x->cid[i + 1] = cid;
	++x->n;
	return true;
}

// bwamem.c:186-206; seed s (already in the read's seed slice) joins chain c or not
__device__ __forceinline__ bool test_and_merge(const bmh_chain_opt_t &o, int64_t l_pac, const Arena &A, int ci, int si)
{
	Chn &c = A.chn[ci];
	const bmh_seed_t f = A.seed[c.first], last = A.seed[c.last], p = A.seed[si];
	const int64_t qend = (int64_t)last.qbeg + last.len, rend = last.rbeg + last.len;
	if (p.qbeg >= f.qbeg && (int64_t)p.qbeg + p.len <= qend && p.rbeg >= f.rbeg && p.rbeg + p.len <= rend) return true; // contained
	if ((last.rbeg < l_pac || f.rbeg < l_pac) && p.rbeg >= l_pac) return false; // other strand
	const int64_t x = (int64_t)p.qbeg - last.qbeg, y = p.rbeg - last.rbeg;
	if (y >= 0 && x - y <= o.w && y - x <= o.w && x - last.len < o.max_chain_gap && y - last.len < o.max_chain_gap) { // grow
		A.next[c.last] = si, A.next[si] = -1;
		c.last = si, ++c.n;
		return true;
	}
	return false;
}

// bwamem.c:245-263, with the second pass advancing `end` on the query as the reference does
__device__ int chain_weight(const Arena &A, const Chn &c)
{
	int64_t end = 0;
	int w = 0;
	for (int s = c.first, j = 0; j < c.n; ++j, s = A.next[s]) {
		const bmh_seed_t sd = A.seed[s];
		if (sd.qbeg >= end) w += sd.len;
		else if ((int64_t)sd.qbeg + sd.len > end) w += (int)(sd.qbeg + sd.len - end);
		end = max(end, (int64_t)sd.qbeg + sd.len);
	}
	const int tmp = w;
	end = 0;
	for (int s = c.first, j = 0; j < c.n; ++j, s = A.next[s]) {
		const bmh_seed_t sd = A.seed[s];
		if (sd.rbeg >= end) w += sd.len;
		else if (sd.rbeg + sd.len > end) w += (int)(sd.rbeg + sd.len - end);
		end = max(end, (int64_t)sd.qbeg + sd.len);
	}
	return min(w, tmp);
}

__device__ __forceinline__ int iv_len(const bmh_smem_intv_t &p) { return (int)((uint32_t)p.info - (uint32_t)(p.info >> 32)); }

__device__ __forceinline__ bool seeds_qualify(const bmh_chain_opt_t &o, const bmh_smem_intv_t &p)
{
	return iv_len(p) >= o.min_seed_len && p.x[2] <= (uint64_t)o.max_occ;
}

} // namespace

// Per read: the seed bound S_r (positions of its long and rare intervals) and the node bound.  Inconsistent offsets raise the flag.
__global__ void chain_size_kernel(bmh_chain_opt_t o, int n_reads, const int *__restrict__ len, const uint64_t *__restrict__ ioff,
                                  const bmh_smem_intv_t *__restrict__ intv, uint64_t n_intv, unsigned long long *__restrict__ seeds,
                                  unsigned long long *__restrict__ nodes, int *__restrict__ err)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads) return;
	unsigned long long s = 0;
	if (len[r] >= o.min_seed_len) {
		const uint64_t lo = ioff[r], hi = ioff[r + 1];
		if (lo > hi || hi > n_intv) atomicOr(err, 1);
		else
			for (uint64_t k = lo; k < hi; ++k)
				if (seeds_qualify(o, intv[k])) s += intv[k].x[2];
		if (s >= kMaxSeedsPerRead) atomicOr(err, 1), s = 0;
	}
	seeds[r] = s, nodes[r] = s ? s / 7 + 2 : 0;
}

// exclusive sums of two count arrays, n + 1 outputs each (the last one is the total); one block of 1024 threads
__global__ __launch_bounds__(1024) void chain_scan2(const unsigned long long *__restrict__ a, const unsigned long long *__restrict__ b, int n,
                                                    unsigned long long *__restrict__ pa, unsigned long long *__restrict__ pb)
{
	__shared__ unsigned long long sa[1024], sb[1024];
	const int t = threadIdx.x, per = (n + 1023) / 1024, lo = min(t * per, n), hi = min(lo + per, n);
	unsigned long long xa = 0, xb = 0;
	for (int k = lo; k < hi; ++k) xa += a[k], xb += b[k];
	sa[t] = xa, sb[t] = xb;
	__syncthreads();
	for (int d = 1; d < 1024; d <<= 1) {
		const unsigned long long ya = t >= d ? sa[t - d] : 0, yb = t >= d ? sb[t - d] : 0;
		__syncthreads();
		sa[t] += ya, sb[t] += yb;
		__syncthreads();
	}
	unsigned long long ca = sa[t] - xa, cb = sb[t] - xb;
	for (int k = lo; k < hi; ++k) {
		pa[k] = ca, pb[k] = cb;
		ca += a[k], cb += b[k];
	}
	if (t == 1023) pa[n] = sa[1023], pb[n] = sb[1023];
}

struct ChainIn { // the per-read seeding tables on the device (bmh_seed_batch's output form)
	int n_reads;
	const int *len;
	const uint32_t *coff;
	const bmh_smem_call_t *calls;
	const uint64_t *ioff;
	const bmh_smem_intv_t *intv;
	const uint64_t *sa_off, *sa_pos;
	uint64_t n_calls, n_intv, n_pos;
};

struct ChainWs { // arena and outputs
	bmh_seed_t *seed;
	int32_t *next;
	Chn *chn;
	Flt *flt;
	int2 *ord;
	Node *node;
	int2 *walk;
	bmh_sort_stk_t *sstk;
	const unsigned long long *seed_base, *node_base; // exclusive sums of the per-read bounds
	unsigned long long seed_cap, node_cap;          // slots allocated
	unsigned long long *n_chn, *n_seed;              // out per read: chains and seeds after the filter
	uint32_t *n_keys;                                // out per read: chains before it
	int *err;
	unsigned long long *n_equal; // look-ups that met an equal key, summed over the batch
};

// One lane per read: smem_next2's rounds, mem_insert_seed, the in-order walk and mem_chain_flt, in the order of bmh_chain_reads.
// The surviving chains stay in the read's slice, best first, as ord[k] = (chain, seed count); chain_place_kernel gathers their seeds.
__global__ __launch_bounds__(64) void chain_kernel(bmh_chain_opt_t o, int64_t l_pac, ChainIn in, ChainWs ws)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= in.n_reads) return;
	ws.n_chn[r] = 0, ws.n_seed[r] = 0, ws.n_keys[r] = 0;
	const int len = in.len[r];
	if (len < o.min_seed_len) return; // bwamem.c:291
	const unsigned long long s0 = ws.seed_base[r], s_cap = ws.seed_base[r + 1] - s0, n0 = ws.node_base[r];
	if (ws.seed_base[r + 1] > ws.seed_cap || ws.node_base[r + 1] > ws.node_cap) { atomicOr(ws.err, 1); return; }
	Arena A{ws.seed + s0, ws.next + s0, ws.chn + s0, ws.flt + s0, ws.ord + s0, ws.node + n0, ws.walk + (size_t)r * kStk,
	        ws.sstk + (size_t)r * kStk, s_cap, ws.node_base[r + 1] - n0};
	const uint32_t c_lo = in.coff[r], c_hi = in.coff[r + 1];
	const uint64_t i_lo = in.ioff[r], i_hi = in.ioff[r + 1];
	if (c_lo > c_hi || c_hi > in.n_calls || i_lo > i_hi || i_hi > in.n_intv) { atomicOr(ws.err, 1); return; }
	const bmh_smem_intv_t *iv = in.intv + i_lo;
	const uint64_t n_iv = i_hi - i_lo;
	const int split_len = min(o.split_len, len); // bwamem.c:213
	Tree bt{-1, 0, 0};
	int n_seeds = 0, n_eq = 0;
	uint32_t c = c_lo;
	while (c < c_hi) { // one smem_next2 round per main bwt_smem1 call
		const bmh_smem_call_t mc = in.calls[c++];
		if (mc.n < 0 || (uint64_t)mc.first + (uint64_t)mc.n > n_iv) { atomicOr(ws.err, 1); return; }
		const bmh_smem_intv_t *m = iv + mc.first;
		int max = 0, max_i = 0;
		for (int i = 0; i < mc.n; ++i) // the longest match, bwamem.c:130-134
			if (max < iv_len(m[i])) max = iv_len(m[i]), max_i = i;
		const bmh_smem_intv_t *s = nullptr;
		int sn = 0;
		if (mc.n > 0 && split_len > 0 && max >= split_len && m[max_i].x[2] <= (uint64_t)o.split_width) { // re-seeded: the next record
			if (c >= c_hi) { atomicOr(ws.err, 1); return; }
			const bmh_smem_call_t sc = in.calls[c++];
			if (sc.x != (int)(((uint32_t)m[max_i].info + (uint32_t)(m[max_i].info >> 32)) >> 1) || sc.min_intv != (int)(m[max_i].x[2] + 1) ||
			    sc.n < 0 || (uint64_t)sc.first + (uint64_t)sc.n > n_iv) {
				atomicOr(ws.err, 1); // the call list does not follow smem_next2's order
				return;
			}
			s = iv + sc.first, sn = sc.n;
		}
		// the round's intervals: the main call's, or its ordered merge by (start, len - end) with the re-seeding call's (KEEP_SUB),
		// produced one at a time in the order bmh_chain_reads lists them
		int i = 0, j = 0;
		for (;;) {
			const bmh_smem_intv_t *p;
			if (!s) {
				if (i >= mc.n) break;
				p = &m[i++];
			} else {
				bool take_m;
				if (i < mc.n && j < sn) {
					const int64_t xi = (int64_t)(m[i].info >> 32 << 32 | (uint64_t)(uint32_t)(len - (int)(uint32_t)m[i].info));
					const int64_t xj = (int64_t)(s[j].info >> 32 << 32 | (uint64_t)(uint32_t)(len - (int)(uint32_t)s[j].info));
					take_m = xi < xj;
				} else if (i < mc.n) take_m = true;
				else if (j < sn) take_m = false;
				else break;
				if (take_m) p = &m[i++];
				else {
					const bmh_smem_intv_t &q = s[j++];
					if (!(iv_len(q) >= max >> 1 && (int)(uint32_t)q.info > mc.x)) continue; // KEEP_SUB
					p = &q;
				}
			}
			// mem_insert_seed's loop body, bwamem.c:216-240
			const bmh_smem_intv_t P = *p;
			const int slen = iv_len(P);
			if (slen < o.min_seed_len || P.x[2] > (uint64_t)o.max_occ) continue;
			const uint64_t so = in.sa_off[i_lo + (uint64_t)(p - iv)];
			if (so == ~0ull || so > in.n_pos || P.x[2] > in.n_pos - so) { atomicOr(ws.err, 1); return; } // the table must cover the interval
			for (uint64_t kk = 0; kk < P.x[2]; ++kk) {
				bmh_seed_t sd;
				sd.rbeg = (int64_t)in.sa_pos[so + kk];
				sd.qbeg = (int32_t)(P.info >> 32), sd.len = slen;
				if (sd.rbeg < l_pac && l_pac < sd.rbeg + sd.len) continue; // bridges the strands
				if ((unsigned long long)n_seeds >= A.seed_cap) { atomicOr(ws.err, 1); return; }
				const int si = n_seeds++;
				A.seed[si] = sd, A.next[si] = -1;
				const int lower = bt.n_keys ? bt_lower(A, bt, sd.rbeg, &n_eq) : -1;
				if (lower < 0 || !test_and_merge(o, l_pac, A, lower, si)) { // a new chain (chains are numbered in creation order)
					const int ci = bt.n_keys;
					A.chn[ci] = Chn{si, si, 1, 0};
					if (!bt_put(A, bt, sd.rbeg, ci)) { atomicOr(ws.err, 1); return; }
				}
			}
		}
	}
	const int n_chn = bt.n_keys;
	ws.n_keys[r] = (uint32_t)n_chn;
	if (n_eq) atomicAdd(ws.n_equal, (unsigned long long)n_eq);
	if (n_chn == 0) return;
	{ // the in-order walk (__kb_traverse): child 0, key 0, child 1, ... key n-1, child n.  Stack entry (node, i): the next key of the
	  // node is i and everything left of it has been emitted.
		int top = -1, k = 0;
		for (int x = bt.root;; x = A.node[x].child[0]) {
			if (top + 1 >= kStk) { atomicOr(ws.err, 1); return; }
			A.walk[++top] = make_int2(x, 0);
			if (!A.node[x].internal) break;
		}
		while (top >= 0) {
			const int2 e = A.walk[top];
			const Node *x = &A.node[e.x];
			if (e.y >= x->n) {
				--top;
				continue;
			}
			A.flt[k++].cid = x->cid[e.y];
			A.walk[top].y = e.y + 1;
			if (x->internal)
				for (int y = x->child[e.y + 1];; y = A.node[y].child[0]) {
					if (top + 1 >= kStk) { atomicOr(ws.err, 1); return; }
					A.walk[++top] = make_int2(y, 0);
					if (!A.node[y].internal) break;
				}
		}
	}
	int n = n_chn;
	if (n_chn > 1) { // mem_chain_flt, bwamem.c:319-380
		for (int i = 0; i < n_chn; ++i) {
			Flt &f = A.flt[i];
			const Chn ch = A.chn[f.cid];
			const bmh_seed_t last = A.seed[ch.last];
			f.beg = A.seed[ch.first].qbeg, f.end = last.qbeg + last.len, f.w = chain_weight(A, ch), f.p = 0, f.p2 = -1;
		}
		bmh_sort_exact_stk(A.flt, (size_t)n_chn, sizeof(Flt), FltLt(), A.sstk);
		for (int i = 0; i < n_chn; ++i) A.ord[i] = make_int2(A.flt[i].cid, 0), A.flt[i].p = i; // best chain first
		int i, jj;
		for (i = 1, n = 1; i < n_chn; ++i) {
			const Flt ai = A.flt[i];
			for (jj = 0; jj < n; ++jj) {
				Flt &aj = A.flt[jj];
				const int b_max = max(aj.beg, ai.beg), e_min = min(aj.end, ai.end);
				if (e_min > b_max) { // overlap on the query
					const int min_l = min(ai.end - ai.beg, aj.end - aj.beg);
					if ((float)(e_min - b_max) >= __fmul_rn((float)min_l, o.mask_level)) { // significant
						if (aj.p2 < 0) aj.p2 = ai.p;
						if ((float)ai.w < __fmul_rn((float)aj.w, o.chain_drop_ratio) && aj.w - ai.w >= o.min_seed_len << 1) break;
					}
				}
			}
			if (jj == n) A.flt[n++] = ai; // not shadowed by a better chain
		}
		for (int q = 0; q < n; ++q) { // kept: the survivors and, for each, the first chain it shadows
			A.ord[A.flt[q].p].y = 1;
			if (A.flt[q].p2 >= 0) A.ord[A.flt[q].p2].y = 1;
		}
	} else A.ord[0] = make_int2(A.flt[0].cid, 1);
	// the kept chains, best first: ord[k] = (chain, seed count), compacted in place (k <= i)
	int kept = 0;
	unsigned long long n_out_seeds = 0;
	for (int i = 0; i < n_chn; ++i) {
		const int2 e = A.ord[i];
		if (!e.y) continue;
		const Chn ch = A.chn[e.x];
		A.ord[kept++] = make_int2(e.x, ch.n);
		n_out_seeds += (unsigned long long)ch.n;
	}
	ws.n_chn[r] = (unsigned long long)kept, ws.n_seed[r] = n_out_seeds;
}

// count -> scan -> place: one lane per read copies its surviving chains (seed counts) and their seeds, in chain order, to the compact
// output.  coff / soff: exclusive sums of n_chn / n_seed.
__global__ void chain_place_kernel(int n_reads, ChainWs ws, const unsigned long long *__restrict__ coff, const unsigned long long *__restrict__ soff,
                                   uint32_t *__restrict__ out_n, bmh_seed_t *__restrict__ out_seed, unsigned long long out_chn_cap,
                                   unsigned long long out_seed_cap)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads) return;
	const unsigned long long nc = ws.n_chn[r];
	if (!nc) return;
	const unsigned long long s0 = ws.seed_base[r];
	const int2 *ord = ws.ord + s0;
	const Chn *chn = ws.chn + s0;
	const bmh_seed_t *seed = ws.seed + s0;
	const int32_t *next = ws.next + s0;
	unsigned long long c = coff[r], at = soff[r];
	if (coff[r + 1] > out_chn_cap || soff[r + 1] > out_seed_cap) { atomicOr(ws.err, 1); return; }
	for (unsigned long long k = 0; k < nc; ++k) {
		const int2 e = ord[k];
		out_n[c++] = (uint32_t)e.y;
		for (int s = chn[e.x].first, j = 0; j < e.y; ++j, s = next[s]) out_seed[at++] = seed[s];
	}
}

} // namespace bmh

using namespace bmh;

namespace {

// device tables -> chains on the host (the rest of both entry points)
// seed_bound: the batch's sum of the per-read seed bounds (positions of the long and rare intervals) -- the arena's size
int chain_device(bmh_ctx *ctx, const bmh_chain_opt_t *o, int64_t l_pac, const ChainIn &in, uint64_t seed_bound, bmh_chain_v *chains)
{
	const int n = in.n_reads;
	const unsigned long long seed_cap = std::max<unsigned long long>(seed_bound, 1);
	const unsigned long long node_cap = seed_cap / 7 + 2 * (unsigned long long)n + 2;
	const size_t nr1 = (size_t)n + 1;
	auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
	// layout of d_chain: header (error flag) | per-read counts and sums | arena | compact output
	size_t o_ = 256;
	const size_t o_sb = o_; o_ += al(nr1 * 8);           // seed bound per read
	const size_t o_nb = o_; o_ += al(nr1 * 8);           // node bound per read
	const size_t o_sbase = o_; o_ += al(nr1 * 8);        // ... their exclusive sums
	const size_t o_nbase = o_; o_ += al(nr1 * 8);
	const size_t o_nchn = o_; o_ += al(nr1 * 8);         // out: chains / seeds after the filter, chains before
	const size_t o_nseed = o_; o_ += al(nr1 * 8);
	const size_t o_nkeys = o_; o_ += al(nr1 * 4);
	const size_t o_coff = o_; o_ += al(nr1 * 8);         // ... the sums of the first two
	const size_t o_soff = o_; o_ += al(nr1 * 8);
	const size_t o_seed = o_; o_ += al(seed_cap * sizeof(bmh_seed_t));
	const size_t o_next = o_; o_ += al(seed_cap * 4);
	const size_t o_chn = o_; o_ += al(seed_cap * sizeof(Chn));
	const size_t o_flt = o_; o_ += al(seed_cap * sizeof(Flt));
	const size_t o_ord = o_; o_ += al(seed_cap * sizeof(int2));
	const size_t o_node = o_; o_ += al(node_cap * sizeof(Node));
	const size_t o_walk = o_; o_ += al((size_t)n * kStk * sizeof(int2));
	const size_t o_sstk = o_; o_ += al((size_t)n * kStk * sizeof(bmh_sort_stk_t));
	const size_t o_outn = o_; o_ += al(seed_cap * 4);
	const size_t o_outs = o_; o_ += al(seed_cap * sizeof(bmh_seed_t));
	int rc;
	if ((rc = ensure(ctx, ctx->d_chain, o_))) return rc;
	uint8_t *d = (uint8_t *)ctx->d_chain.p;
	int *d_err = (int *)d;
	BMH_HIP(ctx, hipMemsetAsync(d, 0, 256, ctx->stream)); // the error flag starts clean on every call
	const unsigned rb = (unsigned)((n + 63) / 64);
	hipLaunchKernelGGL(chain_size_kernel, dim3(rb), dim3(64), 0, ctx->stream, *o, n, in.len, in.ioff, in.intv, in.n_intv,
	                   (unsigned long long *)(d + o_sb), (unsigned long long *)(d + o_nb), d_err);
	hipLaunchKernelGGL(chain_scan2, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long *)(d + o_sb), (const unsigned long long *)(d + o_nb), n,
	                   (unsigned long long *)(d + o_sbase), (unsigned long long *)(d + o_nbase));
	BMH_HIP(ctx, hipGetLastError());
	ChainWs ws{(bmh_seed_t *)(d + o_seed), (int32_t *)(d + o_next), (Chn *)(d + o_chn), (Flt *)(d + o_flt), (int2 *)(d + o_ord), (Node *)(d + o_node),
	           (int2 *)(d + o_walk), (bmh_sort_stk_t *)(d + o_sstk), (const unsigned long long *)(d + o_sbase), (const unsigned long long *)(d + o_nbase),
	           seed_cap, node_cap, (unsigned long long *)(d + o_nchn), (unsigned long long *)(d + o_nseed), (uint32_t *)(d + o_nkeys), d_err,
	           (unsigned long long *)(d + 8)};
	if (ctx->timing) {
		if (!ctx->ev_chain[0]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_chain[0]));
		if (!ctx->ev_chain[1]) BMH_HIP(ctx, hipEventCreate(&ctx->ev_chain[1]));
		BMH_HIP(ctx, hipEventRecord(ctx->ev_chain[0], ctx->stream));
	}
	hipLaunchKernelGGL(chain_kernel, dim3(rb), dim3(64), 0, ctx->stream, *o, l_pac, in, ws);
	BMH_HIP(ctx, hipGetLastError());
	if (ctx->timing) BMH_HIP(ctx, hipEventRecord(ctx->ev_chain[1], ctx->stream));
	hipLaunchKernelGGL(chain_scan2, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long *)(d + o_nchn), (const unsigned long long *)(d + o_nseed), n,
	                   (unsigned long long *)(d + o_coff), (unsigned long long *)(d + o_soff));
	hipLaunchKernelGGL(chain_place_kernel, dim3(rb), dim3(64), 0, ctx->stream, n, ws, (const unsigned long long *)(d + o_coff),
	                   (const unsigned long long *)(d + o_soff), (uint32_t *)(d + o_outn), (bmh_seed_t *)(d + o_outs), seed_cap, seed_cap);
	BMH_HIP(ctx, hipGetLastError());
	// the flag, the equal-key count and the two totals, then everything else at its size
	if ((rc = ensure_host(ctx, ctx->h_down, 64))) return rc;
	uint8_t *h = (uint8_t *)ctx->h_down.p;
	BMH_HIP(ctx, hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, hipMemcpyAsync(h + 16, d + o_coff + (size_t)n * 8, 8, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, hipMemcpyAsync(h + 24, d + o_soff + (size_t)n * 8, 8, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	int err;
	unsigned long long tc, ts, n_equal;
	memcpy(&err, h, 4), memcpy(&n_equal, h + 8, 8), memcpy(&tc, h + 16, 8), memcpy(&ts, h + 24, 8);
	if (err) {
		ctx->last_error = "chaining: the seeding tables are inconsistent (call list out of smem_next2's order, or an interval without its positions)";
		return BMH_E_ARG;
	}
	const size_t b_off = al(nr1 * 8), b_keys = al(nr1 * 4), b_n = al(tc * 4), b_s = tc ? ts * sizeof(bmh_seed_t) : 0;
	if ((rc = ensure_host(ctx, ctx->h_down, 2 * b_off + b_keys + b_n + b_s + 64))) return rc;
	h = (uint8_t *)ctx->h_down.p;
	BMH_HIP(ctx, hipMemcpyAsync(h, d + o_coff, nr1 * 8, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, hipMemcpyAsync(h + b_off, d + o_soff, nr1 * 8, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, hipMemcpyAsync(h + 2 * b_off, d + o_nkeys, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	if (tc) BMH_HIP(ctx, hipMemcpyAsync(h + 2 * b_off + b_keys, d + o_outn, tc * 4, hipMemcpyDeviceToHost, ctx->stream));
	if (b_s) BMH_HIP(ctx, hipMemcpyAsync(h + 2 * b_off + b_keys + b_n, d + o_outs, b_s, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	const unsigned long long *coff = (const unsigned long long *)h, *soff = (const unsigned long long *)(h + b_off);
	const uint32_t *nkeys = (const uint32_t *)(h + 2 * b_off), *cn = (const uint32_t *)(h + 2 * b_off + b_keys);
	const bmh_seed_t *sd = (const bmh_seed_t *)(h + 2 * b_off + b_keys + b_n);
	long long before = 0;
	for (int r = 0; r < n; ++r) { // mem_chain's return form: a[] sized for every chain before the filter, seed arrays grown 4, 8, 16 ...
		const unsigned long long c0 = coff[r], c1 = coff[r + 1];
		unsigned long long at = soff[r];
		before += nkeys[r];
		chains[r].n = chains[r].m = 0, chains[r].a = nullptr;
		if (!nkeys[r]) continue;
		chains[r].a = (bmh_chain_t *)malloc(sizeof(bmh_chain_t) * nkeys[r]);
		if (!chains[r].a) goto nomem;
		chains[r].m = nkeys[r], chains[r].n = (size_t)(c1 - c0);
		for (unsigned long long k = c0; k < c1; ++k) {
			bmh_chain_t &c = chains[r].a[k - c0];
			c.n = (int)cn[k];
			for (c.m = 4; c.m < c.n; c.m <<= 1) {}
			c.seeds = (bmh_seed_t *)malloc(sizeof(bmh_seed_t) * (size_t)c.m);
			if (!c.seeds) {
				chains[r].n = (size_t)(k - c0);
				goto nomem;
			}
			memcpy(c.seeds, sd + at, sizeof(bmh_seed_t) * (size_t)c.n);
			c.pos = c.seeds[0].rbeg;
			at += (unsigned long long)c.n;
		}
	}
	ctx->cstats.reads = n, ctx->cstats.chains_in = before, ctx->cstats.chains_out = (int64_t)tc, ctx->cstats.seeds = (int64_t)ts;
	ctx->cstats.equal_keys = (int64_t)n_equal;
	ctx->cstats.kernel_ms = -1.f;
	if (ctx->timing) BMH_HIP(ctx, hipEventElapsedTime(&ctx->cstats.kernel_ms, ctx->ev_chain[0], ctx->ev_chain[1]));
	return BMH_OK;
nomem:
	for (int r = 0; r < n; ++r) {
		for (size_t k = 0; k < chains[r].n; ++k) free(chains[r].a[k].seeds);
		free(chains[r].a);
		chains[r].n = chains[r].m = 0, chains[r].a = nullptr;
	}
	ctx->last_error = "chaining: out of host memory for the chains";
	return BMH_E_NOMEM;
}

int seed_chain_cb(bmh_ctx *ctx, const DevSeedTables &t, void *user)
{
	const auto *u = (const std::pair<const bmh_chain_opt_t *, std::pair<int64_t, bmh_chain_v *>> *)user;
	const ChainIn in{t.n_reads, t.len, t.coff, t.calls, t.ioff, t.intv, t.sa_off, t.sa_pos, t.n_calls, t.n_intv, t.n_pos};
	return chain_device(ctx, u->first, u->second.first, in, t.n_pos, u->second.second); // (sa_of_intervals_kernel used the same two filters)
}

bool chain_opt_ok(const bmh_chain_opt_t *o) { return o && o->min_seed_len >= 0 && o->max_occ >= 0; }

} // namespace

extern "C" {

int bmh_chain_batch(bmh_ctx_t *ctx, const bmh_chain_opt_t *o, int64_t l_pac, int n_reads, const bmh_read_t *reads, const uint32_t *call_off,
                    const bmh_smem_call_t *calls, const uint64_t *intv_off, const bmh_smem_intv_t *intv, const uint64_t *sa_off,
                    const uint64_t *sa_pos, uint64_t n_pos, bmh_chain_v *chains)
{
	if (!ctx || !chain_opt_ok(o) || n_reads < 0 || l_pac < 0 ||
	    (n_reads > 0 && (!reads || !call_off || !intv_off || !chains || (call_off[n_reads] && !calls) || (intv_off[n_reads] && (!intv || !sa_off)) ||
	                     (n_pos && !sa_pos))))
		return BMH_E_ARG;
	for (int r = 0; r < n_reads; ++r) chains[r].n = chains[r].m = 0, chains[r].a = nullptr;
	if (n_reads == 0) return BMH_OK;
	const uint64_t n_calls = call_off[n_reads], n_intv = intv_off[n_reads];
	for (int r = 0; r < n_reads; ++r)
		if (reads[r].l_seq < 0 || call_off[r] > call_off[r + 1] || intv_off[r] > intv_off[r + 1]) return BMH_E_ARG;
	// the seed bound of the batch (what the size kernel sums per read)
	uint64_t n_seed = 0;
	for (uint64_t k = 0; k < n_intv; ++k) {
		const bmh_smem_intv_t &p = intv[k];
		if ((int)((uint32_t)p.info - (uint32_t)(p.info >> 32)) >= o->min_seed_len && p.x[2] <= (uint64_t)o->max_occ) n_seed += p.x[2];
	}
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	int rc;
	// upload: lengths | call offsets | calls | interval offsets | intervals | sa_off | sa_pos, one pinned image, one copy
	auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
	const size_t nr1 = (size_t)n_reads + 1;
	const size_t o_len = 0, o_coff = al(nr1 * 4), o_calls = o_coff + al(nr1 * 4), o_ioff = o_calls + al(n_calls * sizeof(bmh_smem_call_t)),
	             o_intv = o_ioff + al(nr1 * 8), o_so = o_intv + al(n_intv * sizeof(bmh_smem_intv_t)), o_pos = o_so + al(n_intv * 8),
	             total = o_pos + al(n_pos * 8) + 256;
	if ((rc = ensure_host(ctx, ctx->h_up, total)) || (rc = ensure(ctx, ctx->d_scratch, total))) return rc;
	uint8_t *h = (uint8_t *)ctx->h_up.p;
	for (int r = 0; r < n_reads; ++r) ((int *)(h + o_len))[r] = reads[r].l_seq;
	memcpy(h + o_coff, call_off, nr1 * 4);
	if (n_calls) memcpy(h + o_calls, calls, n_calls * sizeof(bmh_smem_call_t));
	memcpy(h + o_ioff, intv_off, nr1 * 8);
	if (n_intv) memcpy(h + o_intv, intv, n_intv * sizeof(bmh_smem_intv_t)), memcpy(h + o_so, sa_off, n_intv * 8);
	if (n_pos) memcpy(h + o_pos, sa_pos, n_pos * 8);
	uint8_t *d = (uint8_t *)ctx->d_scratch.p;
	BMH_HIP(ctx, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, ctx->stream));
	ChainIn in{n_reads, (const int *)(d + o_len), (const uint32_t *)(d + o_coff), (const bmh_smem_call_t *)(d + o_calls), (const uint64_t *)(d + o_ioff),
	           (const bmh_smem_intv_t *)(d + o_intv), (const uint64_t *)(d + o_so), (const uint64_t *)(d + o_pos), n_calls, n_intv, n_pos};
	return chain_device(ctx, o, l_pac, in, n_seed, chains);
}

int bmh_seed_chain_batch(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                         bmh_chain_v *chains)
{
	if (!ctx || !so || !chain_opt_ok(co) || n_reads < 0 || l_pac < 0 || (n_reads > 0 && (!reads || !chains))) return BMH_E_ARG;
	if (so->min_seed_len != co->min_seed_len || so->split_len != co->split_len || so->split_width != co->split_width || so->min_emit_len < 0 ||
	    so->min_emit_len > co->min_seed_len) {
		ctx->last_error = "bmh_seed_chain_batch: min_seed_len / split_len / split_width must agree and min_emit_len <= min_seed_len";
		return BMH_E_ARG;
	}
	for (int r = 0; r < n_reads; ++r) chains[r].n = chains[r].m = 0, chains[r].a = nullptr;
	std::pair<const bmh_chain_opt_t *, std::pair<int64_t, bmh_chain_v *>> u{co, {l_pac, chains}};
	return seed_tables_device(ctx, so, co->max_occ, n_reads, reads, seed_chain_cb, &u);
}

int bmh_chain_stats(bmh_ctx_t *ctx, bmh_chain_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->cstats;
	return BMH_OK;
}

} // extern "C"
