// samtext.h -- what api.hip hands samtext.hip (bmh_sam_text_device): the records of one call's device block and the kernels' arguments.
#pragma once
#include "bmh_ctx.h"
#include "wanted.h"
#include "../host/samtext_core.h"

namespace bmh {

struct SamtextHdr { // the upload's parameter block
	int32_t opt_flag, pe, l_rg, rsv; // mem_opt_t.flag; reads come in pairs; bytes of rg_id
	bmh_pestat_t pes[4];
};
static_assert(sizeof(SamtextHdr) == 144, "the header states the upload's size");

// a read in the pool the host packs: this record, then name, base codes, qualities (has_qual) and comment (l_comment >= 0), the whole
// rounded up to 8 bytes.  bases false: the record of a session whose bases are on the device already (SamtextArgs::bases) has none
struct SamtextRead {
	int32_t l_name, l_seq, has_qual, l_comment; // l_comment -1: none
};
constexpr size_t samtext_read_bytes(size_t l_name, size_t l_seq, bool qual, long long l_comment, bool bases = true)
{
	return (sizeof(SamtextRead) + l_name + l_seq * ((bases ? 1 : 0) + (qual ? 1 : 0)) + (size_t)(l_comment > 0 ? l_comment : 0) + 7) & ~(size_t)7;
}

// the only thing the host reads between launches
struct SamtextStatus { // 16 bytes
	long long total; // bytes of text
	int32_t err, rsv; // the first error (also in the context's word)
};

// What the fused session (bmh_phase2_text_device) keeps beside the status, zeroed before every size launch.  n_host: regions of the slice
// whose records are still the host's to make (phase2_text_bind_kernel counts them); lines: SAM lines of the slice (the size kernel's sum)
struct SamtextFused { // 16 bytes
	int32_t n_host, rsv;
	long long lines;
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
	// not NULL (bmh_pairs_sam_finish): the records hold no bases, read i's are bases[soff[i] .. soff[i] + l_seq) in a pool of bases_bytes
	const uint8_t *bases;
	const unsigned long long *soff; // n + 1
	unsigned long long bases_bytes;
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
	SamtextFused *fused;            // NULL in the stand-alone call.  Non-zero n_host: the size and scan kernels leave at once and raise nothing
};

// the records, the per-unit rule, the sizes; then their scan.  Behind it alns[], plan[], toff[] and the status are complete.
int launch_samtext_size(bmh_ctx *ctx, const SamtextArgs &A);
// every read's lines into text[toff[i] .. toff[i+1])
int launch_samtext_emit(bmh_ctx *ctx, const SamtextArgs &A);

// ---- what joins pass B's device arrays to pass C's input in the fused session (bmh_phase2_text_device, api.hip)

// Pass B's contiguous reads pool from the per-read pool of A (poff, rpool, rpool_bytes, n): read i's base codes to
// dst[seq_off[i] .. seq_off[i + 1]), one wave per read.  A record outside the pool (samtext_read_view's checks), or offsets that are not
// the read's length inside reads_bytes, copies nothing and raises A's error words.  In timing mode ctx->ev_gather are recorded around it.
int launch_reads_gather(bmh_ctx *ctx, const SamtextArgs &A, const unsigned long long *seq_off, uint8_t *dst, unsigned long long reads_bytes);

// a region flagged BMH_WANTED_HOST as the host needs it to redo it: where it stands in want order, whose it is, the sorted region and
// the coordinates as cut
struct Phase2TextHost { // 112 bytes
	int64_t j;
	int32_t read, k;
	bmh_alnreg_t reg;
	int64_t rb, re;
	int32_t qb, qe;
	uint32_t flags, rsv;
};

struct Phase2TextBindArgs {
	const WantedStatus *status;     // [1].n_w: the wanted regions
	bmh_wanted_res_t *wres;         // in want order; cigar_off / md_off: the slot number in, the slot's address out
	const WantRec *rec;             // read and k of wanted region j
	const unsigned long long *roff; // n + 1
	const bmh_alnreg_t *reg;        // the sorted regions, total of them
	unsigned long long total;
	int32_t n, cig_cap, md_cap;     // words / bytes per slot
	unsigned long long w_cap;       // entries list[] holds
	Phase2TextHost *list;
	SamtextFused *fused;            // n_host: entries appended (in no order the output may depend on)
	SamtextStatus *status_out;      // the error words
	int *err;
};
// one lane per wanted region, behind wanted_result_kernel
int launch_phase2_text_bind(bmh_ctx *ctx, const Phase2TextBindArgs &A, int64_t n_w);
// wres[at[t]] = recs[t] for t < m: the records the host has redone, at[t] < n_w checked
int launch_phase2_text_patch(bmh_ctx *ctx, bmh_wanted_res_t *wres, const bmh_wanted_res_t *recs, const int64_t *at, int64_t m, int64_t n_w,
                             SamtextStatus *status, int *err);

} // namespace bmh
