// decide.h -- what api.hip hands decide.hip (bmh_decide_device): the layout of one call's device block and the kernel's arguments.
#pragma once
#include "bmh_ctx.h"
#include "../host/postproc_core.h"

namespace bmh {

struct DecideHdr { // the upload's parameter block
	bmh_sam_opt_t opt;
	bmh_pestat_t pes[4]; // zeros for single-end reads
};

struct DecideArgs {
	const unsigned long long *roff; // n + 1: regions before read i
	const DecideHdr *hdr;
	bmh_pp_tab_t tab;               // device pointers: the context's log table, the call's pair table
	bmh_alnreg_t *reg;              // the arena: every read's regions at roff, sorted and marked in place
	unsigned long long total;       // its records
	int32_t *reg_mapq, *want_k;     // total each, at roff
	int32_t *n_want;                // n
	bmh_pairdec_t *pd;              // n / 2 (paired-end)
	int *z;                         // scratch, total: the marking's z[] at roff
	bmh_pair64_t *v;                // scratch, total (paired-end): a pair's keys at roff of its first read
	int64_t l_pac, id0;
	int n, pe;
	int *err;                       // BMH_E_ARG by atomicCAS from 0 for offsets outside the arena: nothing touched for that unit
};

// one lane per read or pair; in timing mode ctx->ev_decide are recorded around the kernel
int launch_decide(bmh_ctx *ctx, const DecideArgs &A);

} // namespace bmh
