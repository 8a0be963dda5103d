/*
 * samtext_core.h -- pass C of phase 2, from the wanted regions' alignments to SAM text, as ONE text for its two forms: the host call
 * bmh_sam_text_batch (host/sam_post.c, gcc) and the kernels behind bmh_sam_text_device (csrc/samtext.hip, hipcc).
 *   bmh_st_record     mem_reg2aln's second half   reference bwa-0.7.8/bwamem.c:1203-1235 (depos, the deletion squeeze, clips, rid, pos)
 *   bmh_st_unit       the tail of mem_sam_pe      bwamem_pair.c:311-324 (the mate records, the proper-pair test of the two top hits)
 *                     and mem_reg2sam_se          bwamem.c:1049-1083 (flags, XS of secondaries, the mapQ cap, the unmapped record)
 *   bmh_st_line       mem_aln2sam                 bwamem.c:904-1017, over the column emitters below
 *   bmh_st_read_text  every line of one read
 * Nothing is allocated.  Under hipcc every routine is __host__ __device__ and always inlined; the C subset used is what lets gcc compile
 * the same text.  Integers only: no sort, no floating point.
 *
 * The text goes into a SINK that either counts (s == NULL) or writes.  The callers run bmh_st_read_text twice per read over the same
 * records, first counting, then writing into a slice of exactly the counted size, so the two passes cannot disagree.  The writing sink
 * carries the size of its slice: a write that would pass it is not made and sets err; l advances either way.  No path writes outside
 * [s, s + cap).
 *
 * A record carries no pointer: its CIGAR is clip5 / n_core words at cig_off of the slice's CIGAR pool / clip3 (bmh_st_op reads operation
 * k of that list, so no clipped copy of the CIGAR exists anywhere), its MD string is md_len bytes at md_off of the MD pool.
 */
#ifndef BMH_SAMTEXT_CORE_H
#define BMH_SAMTEXT_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bwamem_hip.h"
#include "postproc_core.h"
#include "regplan_core.h"

#define BMH_ST_HD BMH_PP_HD

/* ---- the sink */
typedef struct bmh_st_sink {
	char *s;        /* NULL: count only */
	int64_t l, cap; /* bytes so far; the slice's size (unused when counting) */
	int32_t err;    /* a write was refused, or a record named something that does not exist */
	int32_t rsv_;
} bmh_st_sink_t;

BMH_ST_HD static inline void bmh_st_c(bmh_st_sink_t *t, char c)
{
	if (t->s) {
		if (t->l < t->cap) t->s[t->l] = c;
		else t->err = 1;
	}
	++t->l;
}
BMH_ST_HD static inline void bmh_st_n(bmh_st_sink_t *t, const char *p, int64_t n)
{
	if (n <= 0) return;
	if (t->s) {
		if (n <= t->cap - t->l) __builtin_memcpy(t->s + t->l, p, (size_t)n);
		else t->err = 1;
	}
	t->l += n;
}
/* kputw / kputl (kstring.h:62-111) without their buffer: count the digits, then write them backwards where they belong */
BMH_ST_HD static inline void bmh_st_l(bmh_st_sink_t *t, int64_t c)
{
	uint64_t x = c < 0 ? (uint64_t)0 - (uint64_t)c : (uint64_t)c, y;
	int len = 1 + (c < 0);
	for (y = x; y >= 10; y /= 10) ++len;
	if (t->s) {
		if (len <= t->cap - t->l) {
			char *e = t->s + t->l + len;
			do *--e = (char)('0' + (int)(x % 10)), x /= 10;
			while (x);
			if (c < 0) *--e = '-';
		} else t->err = 1;
	}
	t->l += len;
}

/* ---- what the composer reads */
typedef struct bmh_st_read { /* a read: name and comment without their NULs, comment / qual NULL where there is none */
	const char *name, *comment, *qual;
	const uint8_t *seq; /* base codes */
	int32_t l_name, l_comment, l_seq, rsv_;
} bmh_st_read_t;
typedef struct bmh_st_names { /* the reference sequences' names: name i is pool[off[i] .. off[i+1]) */
	const char *pool;
	const uint64_t *off;
	int32_t n_seqs, rsv_;
} bmh_st_names_t;
typedef struct bmh_st_aln { /* mem_aln_t (bwamem.h:72-82), 64 bytes */
	int64_t pos;
	int32_t rid, flag, is_rev, mapq, NM, n_cigar, score, sub;
	int32_t clip5, clip3, n_core; /* n_cigar = (clip5 != 0) + n_core + (clip3 != 0) */
	uint32_t cig_off, md_off, md_len;
} bmh_st_aln_t;
typedef struct bmh_st_plan { /* what one read prints: `one` alone (a paired decision's hit, or the unmapped record), else its records */
	bmh_st_aln_t one, mate;
	int32_t single, has_mate;
} bmh_st_plan_t;

BMH_ST_HD static inline void bmh_st_unmapped(bmh_st_aln_t *a) /* mem_reg2aln(..., 0), bwamem.c:1171-1175 */
{
	a->pos = -1, a->rid = -1, a->flag = 0x4, a->is_rev = 0, a->mapq = 0, a->NM = 0, a->n_cigar = 0, a->score = 0, a->sub = 0;
	a->clip5 = a->clip3 = a->n_core = 0, a->cig_off = a->md_off = a->md_len = 0;
}

BMH_ST_HD static inline uint32_t bmh_st_op(const bmh_st_aln_t *a, const uint32_t *cig, int k) /* operation k of the clipped CIGAR */
{
	if (a->clip5) {
		if (k == 0) return (uint32_t)a->clip5 << 4 | 3;
		--k;
	}
	return k < a->n_core ? cig[(size_t)a->cig_off + (size_t)k] : (uint32_t)a->clip3 << 4 | 3;
}

/* ---- the record rule, bwamem.c:1203-1235: wanted region x of a read of l_query bases, `ar` its region, mapq its mem_approx_mapq_se,
 * cig the CIGAR pool x addresses.  0, or BMH_E_ARG for a record outside its read or the reference (nothing the reference could print) */
BMH_ST_HD static inline int bmh_st_record(const bmh_rp_refv_t *rv, const bmh_wanted_res_t *x, const bmh_alnreg_t *ar, int mapq, int l_query,
                                           const uint32_t *cig, bmh_st_aln_t *a)
{
	const int64_t l_pac = rv->l_pac;
	const uint32_t *src = cig + x->cigar_off;
	int64_t pos = x->rb < l_pac ? x->rb : x->re - 1;
	int nc = x->n_cigar, is_rev, off = 0;
	if (nc < 0 || x->qb < 0 || x->qb > x->qe || x->qe > l_query) return BMH_E_ARG;
	is_rev = pos >= l_pac; /* bns_depos, bntseq.h:83-86 */
	if (is_rev) pos = (l_pac << 1) - 1 - pos;
	a->mapq = ar->secondary < 0 ? mapq : 0;
	a->flag = ar->secondary >= 0 ? 0x100 : 0;
	a->NM = x->NM, a->md_off = x->md_off, a->md_len = x->md_len;
	a->is_rev = is_rev;
	if (nc > 0) { /* squeeze out a leading or trailing deletion */
		if ((src[0] & 0xf) == 2) pos += src[0] >> 4, off = 1, --nc;
		else if ((src[nc - 1] & 0xf) == 2) --nc;
	}
	a->clip5 = is_rev ? l_query - x->qe : x->qb, a->clip3 = is_rev ? x->qb : l_query - x->qe; /* soft clipping */
	a->cig_off = x->cigar_off + (uint32_t)off, a->n_core = nc;
	a->n_cigar = (a->clip5 != 0) + nc + (a->clip3 != 0);
	a->rid = pos < 0 ? -1 : bmh_rp_pos2rid(rv, pos);
	if (a->rid < 0 || a->rid >= rv->n_seqs) return BMH_E_ARG;
	a->pos = pos - bmh_rp_ref_off(rv, a->rid);
	a->score = ar->score, a->sub = ar->sub > ar->csub ? ar->sub : ar->csub;
	return 0;
}

/* ---- the per-unit rule: a read, or (pe) a pair with d its pair decision.
 *   f[r], f[r+1]   read r's records are alns[f[r] .. f[r+1]), in want order
 *   wk[r]          ... and the index of each in the read's region vector ra[r]
 * The mate copies are taken BEFORE the flag loop touches the records, as the reference takes them (bwamem_pair.c:311-312, :320-324 before
 * mem_reg2sam_se).  Leaves the records as mem_reg2sam_se prints them and plan[r] for each read. */
BMH_ST_HD static inline void bmh_st_unit(int opt_flag, int64_t l_pac, const bmh_pestat_t *pes, int pe, const bmh_pairdec_t *d, const int64_t *f,
                                         const int32_t *const wk[2], const bmh_alnreg_t *const ra[2], bmh_st_aln_t *alns, bmh_st_plan_t *plan)
{
	const int nr = pe ? 2 : 1;
	bmh_st_aln_t h[2];
	int r, extra = 0;
	if (pe) {
		extra = d->extra_flag;
		for (r = 0; r < 2; ++r) { /* the pair's two alignments, or each end's best hit */
			const int64_t f0 = f[r], f1 = f[r + 1];
			if (d->paired) {
				if (f1 > f0) h[r] = alns[f0], h[r].mapq = d->q_se[r];
				else bmh_st_unmapped(&h[r]);
				h[r].flag |= (r ? 0x80 : 0x40) | extra;
			} else if (f1 > f0 && wk[r][0] == 0) h[r] = alns[f0]; /* regs[].a[0] with score >= T */
			else bmh_st_unmapped(&h[r]);
		}
		if (d->paired) {
			for (r = 0; r < 2; ++r) plan[r].one = h[r], plan[r].mate = h[!r], plan[r].single = 1, plan[r].has_mate = 1;
			return;
		}
		if (!(opt_flag & BMH_MEM_F_NOPAIRING) && h[0].rid == h[1].rid && h[0].rid >= 0) { /* the two top hits make a proper pair? */
			int64_t dist;
			const int dd = bmh_pp_infer_dir(l_pac, ra[0][0].rb, ra[1][0].rb, &dist);
			if (!pes[dd].failed && dist >= pes[dd].low && dist <= pes[dd].high) extra |= 2;
		}
	}
	for (r = 0; r < nr; ++r) { /* mem_reg2sam_se, bwamem.c:1049-1083 */
		const int64_t f0 = f[r], f1 = f[r + 1];
		const int extra_flag = pe ? ((r ? 0x81 : 0x41) | extra) : 0;
		int64_t q;
		for (q = f0; q < f1; ++q) {
			const int k = wk[r][q - f0];
			const bmh_alnreg_t *p = &ra[r][k];
			bmh_st_aln_t *a = &alns[q];
			a->flag |= extra_flag;
			if (p->secondary >= 0) a->sub = -1;
			if (k && p->secondary < 0) a->flag |= (opt_flag & BMH_MEM_F_NO_MULTI) ? 0x10000 : 0x800; /* supplementary */
			if (k && a->mapq > alns[f0].mapq) a->mapq = alns[f0].mapq;
		}
		plan[r].has_mate = pe, plan[r].single = f1 == f0;
		if (pe) plan[r].mate = h[!r];
		else bmh_st_unmapped(&plan[r].mate);
		bmh_st_unmapped(&plan[r].one);
		plan[r].one.flag |= extra_flag;
	}
}

/* ---- One SAM line (what mem_aln2sam prints, bwamem.c:904-1017): the record and its mate are first RESOLVED into a small value (flag
 * bits, where an unmapped end is placed, clip lengths), then the column emitters write the eleven mandatory columns and the tags. */
typedef struct bmh_st_place {
	int mapped;         /* has a reference sequence to print (its own, or the mate's for an unmapped end) */
	int rid, rev, n_op; /* n_op = 0 when the end only borrows its mate's position */
	int64_t pos;
	const bmh_st_aln_t *a; /* whose CIGAR the n_op operations are */
} bmh_st_place_t;

typedef struct bmh_st_line {
	const bmh_st_names_t *names;
	const bmh_st_read_t *read;
	const bmh_st_aln_t *all; /* the read's records (for SA:Z) */
	int n_all, self;         /* ... and which one this line is */
	const bmh_st_aln_t *rec;
	const uint32_t *cig;
	const char *md, *rg_id;
	int l_rg, flag, has_mate;
	bmh_st_place_t me, mate;
} bmh_st_line_t;

BMH_ST_HD static inline bmh_st_place_t bmh_st_place_of(const bmh_st_aln_t *a)
{
	bmh_st_place_t p;
	p.mapped = a->rid >= 0, p.rid = a->rid, p.rev = a->is_rev, p.n_op = a->n_cigar, p.pos = a->pos, p.a = a;
	return p;
}
/* an unmapped end sits where its mapped mate is, without a CIGAR (bwamem.c:917-918) */
BMH_ST_HD static inline void bmh_st_borrow(bmh_st_place_t *dst, const bmh_st_place_t *src)
{
	dst->mapped = 1, dst->rid = src->rid, dst->pos = src->pos, dst->rev = src->rev, dst->n_op = 0;
}
BMH_ST_HD static inline int bmh_st_clip_len(const bmh_st_place_t *p, const uint32_t *cig, int at) /* length of a clip at CIGAR index `at`, else 0 */
{
	const uint32_t w = bmh_st_op(p->a, cig, at);
	const int op = (int)(w & 0xf);
	return op == 3 || op == 4 ? (int)(w >> 4) : 0;
}
BMH_ST_HD static inline int64_t bmh_st_far_end(const bmh_st_place_t *p, const uint32_t *cig) /* 5' end on the reference; get_rlen, bwamem.c:893-902 */
{
	int k, l = 0;
	if (!p->rev) return p->pos;
	for (k = 0; k < p->n_op; ++k) {
		const uint32_t w = bmh_st_op(p->a, cig, k);
		const int op = (int)(w & 0xf);
		if (op == 0 || op == 2) l += (int)(w >> 4);
	}
	return p->pos + (l - 1);
}
BMH_ST_HD static inline void bmh_st_name(bmh_st_sink_t *t, const bmh_st_names_t *nm, int rid)
{
	if (rid < 0 || rid >= nm->n_seqs) t->err = 1;
	else bmh_st_n(t, nm->pool + nm->off[rid], (int64_t)(nm->off[rid + 1] - nm->off[rid]));
}

/* bases or qualities of [from,to) in the orientation of the alignment; `code` maps a base code to its letter (NULL: copy bytes) */
BMH_ST_HD static inline void bmh_st_oriented(bmh_st_sink_t *t, const char *src, int from, int to, int rev, const char *code)
{
	const int n = to > from ? to - from : 0;
	int i;
	if (t->s) {
		if (n <= t->cap - t->l) {
			char *d = t->s + t->l;
			if (code) {
				for (i = 0; i < n; ++i) {
					const uint8_t c = (uint8_t)src[rev ? to - 1 - i : from + i];
					d[i] = code[c < 4 ? c : 4];
				}
			} else if (!rev) __builtin_memcpy(d, src + from, (size_t)n);
			else for (i = 0; i < n; ++i) d[i] = src[to - 1 - i];
		} else t->err = 1;
	}
	t->l += n;
}
enum { BMH_ST_CLIP_SOFT, BMH_ST_CLIP_HARD, BMH_ST_CLIP_ASIS }; /* clips of the first line are S, of a supplementary line H; SA:Z prints what is stored */
BMH_ST_HD static inline void bmh_st_ops(bmh_st_sink_t *t, const bmh_st_aln_t *a, const uint32_t *cig, int n, int clips)
{
	int i;
	for (i = 0; i < n; ++i) {
		const uint32_t w = bmh_st_op(a, cig, i);
		int c = (int)(w & 0xf);
		if (clips != BMH_ST_CLIP_ASIS && (c == 3 || c == 4)) c = clips == BMH_ST_CLIP_HARD ? 4 : 3;
		bmh_st_l(t, (int64_t)(w >> 4)), bmh_st_c(t, c < 5 ? "MIDSH"[c] : '?');
	}
}

BMH_ST_HD static inline void bmh_st_col_qname_flag(const bmh_st_line_t *L, bmh_st_sink_t *t)
{
	bmh_st_n(t, L->read->name, L->read->l_name), bmh_st_c(t, '\t');
	bmh_st_l(t, (L->flag & 0xffff) | (L->flag & 0x10000 ? 0x100 : 0)); /* -M: a supplementary hit is shown as secondary (bwamem.c:928) */
}
BMH_ST_HD static inline void bmh_st_col_rname_pos_mapq_cigar(const bmh_st_line_t *L, bmh_st_sink_t *t)
{
	if (!L->me.mapped) { bmh_st_n(t, "*\t0\t0\t*", 7); return; }
	bmh_st_name(t, L->names, L->me.rid), bmh_st_c(t, '\t');
	bmh_st_l(t, L->me.pos + 1), bmh_st_c(t, '\t');
	bmh_st_l(t, L->rec->mapq), bmh_st_c(t, '\t');
	if (L->me.n_op) bmh_st_ops(t, L->me.a, L->cig, L->me.n_op, L->self ? BMH_ST_CLIP_HARD : BMH_ST_CLIP_SOFT);
	else bmh_st_c(t, '*');
}
BMH_ST_HD static inline void bmh_st_col_mate(const bmh_st_line_t *L, bmh_st_sink_t *t)
{
	if (!L->has_mate || !L->mate.mapped) { bmh_st_n(t, "*\t0\t0", 5); return; }
	if (L->me.rid == L->mate.rid) bmh_st_c(t, '=');
	else bmh_st_name(t, L->names, L->mate.rid);
	bmh_st_c(t, '\t'), bmh_st_l(t, L->mate.pos + 1), bmh_st_c(t, '\t');
	if (L->me.rid == L->mate.rid && L->me.n_op && L->mate.n_op) { /* TLEN between the two 5' ends (bwamem.c:957-961) */
		const int64_t d = bmh_st_far_end(&L->me, L->cig) - bmh_st_far_end(&L->mate, L->cig);
		bmh_st_l(t, -(d + (d > 0) - (d < 0)));
	} else bmh_st_c(t, '0');
}
BMH_ST_HD static inline void bmh_st_col_seq_qual(const bmh_st_line_t *L, bmh_st_sink_t *t)
{
	int from = 0, to = L->read->l_seq;
	if (L->flag & 0x100) { bmh_st_n(t, "*\t*", 3); return; } /* none on secondary lines */
	if (L->self && L->me.n_op) { /* a supplementary line prints only what it aligns: its clips are hard (bwamem.c:971-976) */
		const int c5 = bmh_st_clip_len(&L->me, L->cig, 0), c3 = bmh_st_clip_len(&L->me, L->cig, L->me.n_op - 1);
		if (L->me.rev) from += c3, to -= c5;
		else from += c5, to -= c3;
		if (from < 0 || to > L->read->l_seq) { t->err = 1; return; } /* (clips longer than the read: no such bytes) */
	}
	bmh_st_oriented(t, (const char *)L->read->seq, from, to, L->me.rev, L->me.rev ? "TGCAN" : "ACGTN");
	bmh_st_c(t, '\t');
	if (L->read->qual) bmh_st_oriented(t, L->read->qual, from, to, L->me.rev, 0);
	else bmh_st_c(t, '*');
}
BMH_ST_HD static inline void bmh_st_col_tags(const bmh_st_line_t *L, bmh_st_sink_t *t)
{
	const bmh_st_aln_t *r = L->rec;
	int i, others = 0;
	if (L->me.n_op) bmh_st_n(t, "\tNM:i:", 6), bmh_st_l(t, r->NM), bmh_st_n(t, "\tMD:Z:", 6), bmh_st_n(t, L->md + r->md_off, (int64_t)r->md_len);
	if (r->score >= 0) bmh_st_n(t, "\tAS:i:", 6), bmh_st_l(t, r->score);
	if (r->sub >= 0) bmh_st_n(t, "\tXS:i:", 6), bmh_st_l(t, r->sub);
	if (L->l_rg > 0) bmh_st_n(t, "\tRG:Z:", 6), bmh_st_n(t, L->rg_id, L->l_rg);
	if (!(L->flag & 0x100)) { /* SA:Z lists the read's other non-secondary lines (bwamem.c:995-1013) */
		for (i = 0; i < L->n_all; ++i) others += i != L->self && !(L->all[i].flag & 0x100);
		if (others) bmh_st_n(t, "\tSA:Z:", 6);
		for (i = 0; others && i < L->n_all; ++i) {
			const bmh_st_aln_t *o = &L->all[i];
			if (i == L->self || (o->flag & 0x100) || o->rid < 0) continue;
			bmh_st_name(t, L->names, o->rid), bmh_st_c(t, ','), bmh_st_l(t, o->pos + 1), bmh_st_c(t, ',');
			bmh_st_c(t, o->is_rev ? '-' : '+'), bmh_st_c(t, ',');
			bmh_st_ops(t, o, L->cig, o->n_cigar, BMH_ST_CLIP_ASIS);
			bmh_st_c(t, ','), bmh_st_l(t, o->mapq), bmh_st_c(t, ','), bmh_st_l(t, o->NM), bmh_st_c(t, ';');
		}
	}
	if (L->read->comment) bmh_st_c(t, '\t'), bmh_st_n(t, L->read->comment, L->read->l_comment);
}

/* the slice-wide inputs of a line */
typedef struct bmh_st_env {
	bmh_st_names_t names;
	const uint32_t *cig; /* the CIGAR pool */
	const char *md;      /* the MD pool */
	const char *rg_id;   /* l_rg bytes, 0 = no read group */
	int32_t l_rg, rsv_;
} bmh_st_env_t;

BMH_ST_HD static inline void bmh_st_line(const bmh_st_env_t *E, bmh_st_sink_t *t, const bmh_st_read_t *s, int n, const bmh_st_aln_t *list, int which,
                                         const bmh_st_aln_t *mate)
{
	bmh_st_line_t L;
	L.names = &E->names, L.read = s, L.all = list, L.n_all = n, L.self = which, L.rec = &list[which], L.cig = E->cig, L.md = E->md;
	L.rg_id = E->rg_id, L.l_rg = E->l_rg;
	L.has_mate = mate != 0;
	L.me = bmh_st_place_of(L.rec);
	L.mate = L.me;
	L.flag = L.rec->flag | (mate ? 0x1 : 0) | (L.me.mapped ? 0 : 0x4);
	if (mate) {
		L.mate = bmh_st_place_of(mate);
		if (!L.mate.mapped) L.flag |= 0x8;
		if (!L.me.mapped && L.mate.mapped) bmh_st_borrow(&L.me, &L.mate);
		else if (!L.mate.mapped && L.me.mapped) bmh_st_borrow(&L.mate, &L.me);
		if (L.mate.rev) L.flag |= 0x20;
	}
	if (L.me.rev) L.flag |= 0x10;
	bmh_st_col_qname_flag(&L, t), bmh_st_c(t, '\t');
	bmh_st_col_rname_pos_mapq_cigar(&L, t), bmh_st_c(t, '\t');
	bmh_st_col_mate(&L, t), bmh_st_c(t, '\t');
	bmh_st_col_seq_qual(&L, t);
	bmh_st_col_tags(&L, t); /* (the tags bring their own separators) */
	bmh_st_c(t, '\n');
}

/* every line of one read: recs[0..n_rec) are its records as bmh_st_unit left them.  Returns the lines. */
BMH_ST_HD static inline int bmh_st_read_text(const bmh_st_env_t *E, bmh_st_sink_t *t, const bmh_st_read_t *s, const bmh_st_plan_t *plan, int n_rec,
                                             const bmh_st_aln_t *recs)
{
	const bmh_st_aln_t *mate = plan->has_mate ? &plan->mate : 0;
	int q;
	if (plan->single) {
		bmh_st_line(E, t, s, 1, &plan->one, 0, mate);
		return 1;
	}
	for (q = 0; q < n_rec; ++q) bmh_st_line(E, t, s, n_rec, recs, q, mate);
	return n_rec;
}

#endif
