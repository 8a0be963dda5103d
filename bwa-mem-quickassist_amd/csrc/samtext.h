// samtext.h -- what api.hip hands samtext.hip (bmh_sam_text_device): the records of one call's device block and the kernels' arguments.
#pragma once
#include "bmh_ctx.h"
#include "../host/samtext_core.h"

namespace bmh {

struct SamtextHdr { // the upload's parameter block
	int32_t opt_flag, pe, l_rg, rsv; // mem_opt_t.flag; reads come in pairs; bytes of rg_id
	bmh_pestat_t pes[4];
};
static_assert(sizeof(SamtextHdr) == 144, "the header states the upload's size");

// a read in the pool the host packs: this record, then name, base codes, qualities (has_qual) and comment (l_comment >= 0), the whole
// rounded up to 8 bytes
struct SamtextRead {
	int32_t l_name, l_seq, has_qual, l_comment; // l_comment -1: none
};
constexpr size_t samtext_read_bytes(size_t l_name, size_t l_seq, bool qual, long long l_comment)
{
	return (sizeof(SamtextRead) + l_name + l_seq * (qual ? 2 : 1) + (size_t)(l_comment > 0 ? l_comment : 0) + 7) & ~(size_t)7;
}

// the only thing the host reads between launches
struct SamtextStatus { // 16 bytes
	long long total; // bytes of text
	int32_t err, rsv; // the first error (also in the context's word)
};

struct SamtextArgs {
	// inputs
	const int64_t *roff, *first;    // n + 1 each: regions / wanted regions before read i
	const unsigned long long *poff; // n + 1: read i's record in rpool
	const SamtextHdr *hdr;
	const char *rg;                 // hdr->l_rg bytes
	const int32_t *n_want, *want_k, *reg_mapq; // n; total each, at roff
	const bmh_pairdec_t *pd;        // n / 2 (pe)
	const bmh_alnreg_t *reg;        // total
	const bmh_wanted_res_t *wr;     // n_w, in want order
	const uint32_t *cig;            // cig_words
	const char *md;                 // md_bytes
	const uint8_t *rpool;           // rpool_bytes
	unsigned long long total, n_w, cig_words, md_bytes, rpool_bytes;
	const bmh_refspan_t *ref;       // the resident sequence table ...
	const char *names;              // ... and the names: name i is names[name_off[i] .. name_off[i+1])
	const uint64_t *name_off;
	int32_t n_seqs, n, pe; // pe: reads 2p, 2p + 1 are mates (n even)
	int64_t l_pac;
	// work and outputs
	bmh_st_aln_t *alns;             // n_w: the records
	bmh_st_plan_t *plan;            // n
	unsigned long long *size;       // n: bytes of read i's lines
	unsigned long long *toff;       // n + 1: their exclusive sums = text_off
	SamtextStatus *status;
	char *text;                     // text_cap bytes (the emit kernel only)
	unsigned long long text_cap;
	int *err;
};

// the records, the per-unit rule, the sizes; then their scan.  Behind it alns[], plan[], toff[] and the status are complete.
int launch_samtext_size(bmh_ctx *ctx, const SamtextArgs &A);
// every read's lines into text[toff[i] .. toff[i+1])
int launch_samtext_emit(bmh_ctx *ctx, const SamtextArgs &A);

} // namespace bmh
