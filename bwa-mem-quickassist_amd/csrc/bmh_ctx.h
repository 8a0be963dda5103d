// bmh_ctx.h -- host-side context shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/bwamem_hip.h"
#include "bmh_device.h"
#include "../host/regplan_core.h"

constexpr int kExtBinsMax = 6;

struct DevBuf { // grow-only device allocation
	void *p = nullptr;
	size_t cap = 0;
};

struct bmh_ctx {
	int device = 0;
	hipStream_t own_stream = nullptr, stream = nullptr;
	bool have_params = false;
	bool glb_params = false; // parameters are set, possibly with a zero gap extension: then have_params stays false and only the global calls run
	bmh_params_t params{};
	bmh::DevParams dev{};
	int qcap = 512; // query-length capacity used to size the LDS kernel's window state for *_device calls
	// device workspaces of the host-buffer entry points
	DevBuf d_pool, d_tasks, d_res, d_order, d_cigar, d_scratch;
	void *bwt_bind = nullptr; // FM-index binding (fmindex.hip), or null
	double smem_calls_per_base = 0.06, smem_intv_per_base = 0.35, smem_pos_per_base = 0.03; // high-water marks of bmh_smem_batch's / bmh_seed_batch's output density
	const uint8_t *h_pac = nullptr; // host identity of the shared device copy of the 2-bit reference (bmh_ctx_set_pac)
	DevBuf d_swrm;  // per-wave row maxima of the register Smith-Waterman kernels
	DevBuf d_sw;    // row / row-maximum slabs of the local Smith-Waterman kernels
	DevBuf d_zslab; // direction words of the lane-per-task global kernels, one slab per resident wave
	int glb_mode = 0; // 0 lane-per-task global kernels, 1 one wave per task only (env BMH_GLB_MODE=wave)
	int sw_mode = 0;  // 0 register kernels where they fit, 1 slab kernel only (env BMH_SW_MODE=generic)
	int glb_fast = 1;   // unmasked body for blocks inside every lane's band (env BMH_GL_FAST=0 turns it off)
	int glb_narrow = 1; // lane kernels run each task on the band its result needs (host/glbband_core.h; env BMH_GLB_NARROW=0 turns it off)
	int glb_c32 = 1;    // bands up to 15 run on the 32-slot instantiation, four waves per SIMD (env BMH_GLB_C32=0: on the 64-slot one)
	int glb_exact = 7;  // bands of 0..3 (level 3) and of 4..7 (level 7) run on global_narrow_kernel, each row on exactly its 2w+1 cells
	                    // (global_narrow.hip; env BMH_GLB_EXACT=0|3|7, 0 = the bins as they were)
	bool gbins_valid = false; // the sort workspace still holds the bin sizes of the last global launch (bmh_last_global_bin_counts)
	DevBuf d_gband;     // ... those bands: n bytes by input position, then kSortBins x n bytes parallel to the sort's lists
	int64_t gband_n = 0; // tasks of the last global launch if its band pass ran, else 0 (bmh_last_global_bands)
	int sw_wave = 1;  // batches of up to 32 k tasks: one wave per task (sw_wave.hip); env BMH_SW_WAVE=0 turns it off
	DevBuf d_bins; // per-launch bin lists of the extension dispatcher: 4 counters + 4 x n task indices
	int grid_mult = 1;    // env BMH_GRID_MULT: persistent grid = resident waves x this (tuning knob)
	int ext_sched = -1;   // env BMH_EXT_SCHED: launch order / streams of the extension bins, -1 = by query length (see launch_extend)
	bool ext_mode_forced = false; // BMH_EXT_MODE was given
	int small_batch = 49152;      // batches of at most this many extension tasks go to the one-task-per-wave kernels (env BMH_EXT_SMALL, 0 = never)
	int force_kernel = 0; // kernels for qlen<=128: 0 lane-per-task, 1 LDS kernel, 2 one task/wave, 3 four tasks/wave (env BMH_EXT_MODE=lds|reg|grp)
	bool pool_resident = false; // d_pool holds a pool uploaded by bmh_upload_pool()
	size_t pool_bytes = 0;
	// pinned staging of the entry points that move bulk data per call from many host threads at once (the runtime's own
	// path for pageable memory was the slowest part of a seeding batch: 5-36 ms for 11 MB with eight threads in flight)
	DevBuf h_up, h_down;
	int *d_err = nullptr; // device error flag (BMH_E_* or 0) in [0]; [2..3]: bin 4's running task count (global_kernel.hip)
	int *h_err = nullptr; // pinned mirror
	// kernel timing
	bool timing = false;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	bool ev_valid = false;
	hipEvent_t ev_bin[kExtBinsMax + 1] = {};     // start of each extension bin's kernels
	hipEvent_t ev_bin_end[kExtBinsMax + 1] = {}; // ... and their end (bins run on two streams, see launch_extend)
	hipStream_t aux_stream = nullptr;            // the few long flanks (bins 3-5) run beside the lane kernels
	hipEvent_t ev_fork = nullptr, ev_join = nullptr;
	hipStream_t aux2_stream = nullptr; // ... and the two short-query bins beside the 128-column one
	hipEvent_t ev_join2 = nullptr;
	hipEvent_t ev_wait = nullptr; // hipEventBlockingSync: what stream_wait() sleeps on in blocking mode
	bool ev_bin_valid = false;
	int ext_split96 = 1; // the 65-128 column bin sends its tasks of up to 96 columns to extend_lane_kernel<96> (3 waves/SIMD); BMH_EXT_SPLIT96=0:
	                     // one kernel for the bin.  Measured: a 1 M-read batch 3.55 against 3.83 ms; the 20 M-read step's extension stage level at
	                     // 4 M-read chunks (83.4 ms: the bin's 4-8 k waves per launch lose to wave quantisation what the third resident wave wins),
	                     // 76.1 against 80.3 ms at 10 M-read chunks
	double ext_bin_ms_sum[kExtBinsMax + 1] = {}; // timing mode: per-bin kernel time summed over dispatcher launches (bmh_extend_bin_ms_sum)
	long long ext_bin_launches = 0;
	hipEvent_t ev_gbin[4] = {}; // boundaries of the three kernels of a global-alignment launch (64-slot, 128-slot, wave)
	bool ev_gbin_valid = false;
	hipEvent_t ev_sround[5] = {}; // boundaries of the four rounds of a fused per-seed launch
	bool ev_sround_valid = false;
	std::string last_error;
	bmh_driver_stats_t dstats{};
	int ncu = 256; // compute units of the device (persistent grids are sized from it)
	bool ext_persist = false; // extension lane kernels as one strided launch with a capped grid (env BMH_EXT_PERSIST=1)
	int ext_grid_mult = 2; // extension lane kernels: grid cap = resident waves x this (env BMH_EXT_GRID_MULT)
	int ext_stop = 1;      // extension lane kernels end a flank once no later row can change its result (host/extstop_core.h; env BMH_EXT_STOP=0 turns it off)
	int64_t ext_rows_cap = 0; // diagnostic (bmh_ctx_set_extend_rows): plain extension launches record the rows each lane-kernel task ran, for task indices below this
	DevBuf d_ext_rows;        // ... uint16 by task index, 0xffff where no lane kernel took the task
	int64_t ext_rows_n = 0;   // entries the last extension launch recorded into (its ext_rows_cap), 0 if it recorded none (bmh_last_extend_rows)
	int ext_narrow = 1;    // extension lane kernels run each flank on the band its result needs (host/extband_core.h; env BMH_EXT_NARROW=0 turns it
	                       // off, and so does an armed rows diagnostic: ext_rows_cap > 0).  Off, the band pass still runs and lists every task's own w
	int ext_bandkey = 1;   // the sort key's 3-bit middle field: 1 the band's class, 0 the h0 bucket (env BMH_EXT_BANDKEY, A/B knob)
	DevBuf d_eband;        // the bands of a dispatcher launch with a band pass: n bytes by input position, then kSortBins x n bytes parallel to the sort's lists
	int64_t eband_n = 0;   // entries of the last such launch, else 0 (bmh_last_extend_bands)
	// Bin sizes of the extension dispatcher are only known on the device.  After every launch they are copied to pinned
	// memory WITHOUT waiting; the next launch of the same kind (plain API call, or stage k of the fused per-seed
	// pipeline) reads whatever has arrived and sizes its grids / picks the kernel of bin 3 from it.  A stale or missing
	// hint costs speed, never correctness: every kernel strides over its bin whatever the grid.
	static constexpr int kHintKinds = 6;
	struct BinHint {
		uint32_t *h = nullptr;   // pinned, 16 words: the bins' counts of the launch that wrote it
		hipEvent_t ev = nullptr; // recorded behind the copy
		bool pending = false, valid = false;
		uint32_t cnt[8] = {};
	} hint[kHintKinds];
	DevBuf d_seedws; // workspace of the fused per-seed extension (seedext.hip)
	DevBuf d_region; // region records, their results, CIGAR and MD slots (bmh_region_cigar_batch)
	// the long round of bmh_region_cigar_batch_long (region_long.hip)
	DevBuf d_rlong;                           // block sums, entries, the rerun's tasks and results
	DevBuf d_lcig, d_lmd;                     // the dense CIGAR and MD pools, 16 guard bytes behind each
	hipEvent_t ev_rlong[4] = {};              // around the round's two halves (timing mode)
	long long rlong_regions = -1, rlong_words = -1, rlong_md = -1; // of the last bmh_region_cigar_batch_long (bmh_last_region_long_stats), -1 = none yet
	float rlong_ms = -1.f;                    // ... and its kernels' duration with kernel timing on, else -1
	bool region_long = false;                 // bmh_ctx_set_region_long: bmh_reg2cigar_batch finishes flagged regions through that call
	long long r2c_regions = -1, r2c_long_device = -1, r2c_redone_host = -1; // of the last bmh_reg2cigar_batch (bmh_last_reg2cigar_stats)
	bmh_seedext_stats_t sstats{};
	int64_t seed_pending_n = -1; // tasks of the bmh_seedext_submit() in flight, -1 = none
	DevBuf d_chain;                // device chainer (chain.hip): per-read bounds, arena, compact output
	hipEvent_t ev_chain[2] = {};   // around its chain kernel (timing mode)
	bmh_chain_stats_t cstats{-1, -1, -1, -1, -1, -1.f};
	DevBuf d_c2r; // chains to regions on the device (chain2reg.hip): status words, chain records, keys, tasks, results, regions
	// int32 extension kernel (extend_wide.hip), opt-in: bmh_ctx_set_wide_extension
	bool wide_ext = false;
	bool wide_last = false;           // the last extension launch (a flat batch, or the four rounds of a fused call) ran with it on
	unsigned long long *d_wide_stat = nullptr; // device: tasks the wide bin received since the launch began
	double wide_ms_sum = 0.0;         // timing mode: the wide kernels' time over the same span
	long long wide_total = 0;         // tasks the wide bin received over the host-buffer extension calls so far (preload shim log)
	DevBuf d_wide_slab;               // per-block state slices of its HBM variant
	// bin 4 of the global path (the band ring, global_kernel.hip): its tasks are counted on the device in d_err[2..3]
	hipEvent_t ev_glong[2] = {};      // around its kernel (timing mode)
	double glong_ms_sum = 0.0;        // timing mode: its time over the context's life (bmh_global_long_stats)
	// word-mode Smith-Waterman on one wave per task for long queries and saturating scores (sw_long.hip), opt-in: bmh_ctx_set_wide_sw
	bool wide_sw = false;
	unsigned long long *d_swl_stat = nullptr; // device: tasks its kernels took over the context's life
	DevBuf d_swl;                             // its row-maximum slab, then the state slices of its HBM variant
	hipEvent_t ev_swl[2] = {};                // around its kernels (timing mode)
	double swl_ms_sum = 0.0;                  // timing mode: their time over the context's life (bmh_sw_wide_stats)
	// mem_sort_and_dedup on the device (region_dedup_kernel, chain2reg.hip): bmh_sort_dedup_batch, and with the switch on
	// (bmh_ctx_set_regs_dedup) the chains-to-regions calls before their gather
	bool regs_dedup = false;
	float regs_dedup_mask = 0.95f;            // mask_level_redun the switch was set with
	DevBuf d_dedup;                           // bmh_sort_dedup_batch: removed-regions counter, offsets, counts, regions
	hipEvent_t ev_dedup[2] = {};              // around the kernel (timing mode)
	long long dedup_in = -1, dedup_out = -1;  // regions in / kept of the last call that ran it (bmh_last_dedup_stats), -1 = none yet
	float dedup_ms = -1.f;                    // ... and the kernel's duration with kernel timing on, else -1
	// mem_pestat's pair walk on the device (pestat_collect_kernel, pestat.hip): bmh_pestat_device, and with a switch on
	// (bmh_ctx_set_pestat_collect, bmh_ctx_set_regs_drop_exact) the chains-to-regions calls behind their de-duplication
	bool pestat_collect = false, regs_drop_exact = false;
	bmh_sam_opt_t pestat_opt{};               // the options the collect switch was set with
	DevBuf d_pestat;                          // bmh_pestat_device: offsets, counts, words, regions
	hipEvent_t ev_pestat[2] = {};             // around the kernel (timing mode)
	std::vector<uint32_t> pestat_cand;        // the words of the last successful collecting call (bmh_last_pestat_candidates)
	long long pestat_pairs = -1;              // ... and its pair count, -1 = none yet
	float pestat_ms = -1.f;                   // ... and the kernel's duration with kernel timing on, else -1
	long long drop_exact_removed = -1;        // regions drop-exact removed in the last successful call that ran it (bmh_last_drop_exact_stats)
	// pass A of phase 2 on the device (decide_kernel, decide.hip): bmh_decide_device, and bmh_sam_batch with the switch on
	bool decide_device = false;               // bmh_ctx_set_decide_device
	DevBuf d_decide;                          // a call's block: offsets, parameters, pair table, regions, outputs, scratch
	DevBuf d_logk;                            // log(k), k = 0..logk_n-1, resident; grown when a call needs more
	long long logk_n = 0;
	double *h_logk = nullptr;                 // the host's copy (malloc), logk_host_n entries
	long long logk_host_n = 0;
	hipEvent_t ev_decide[2] = {};             // around the kernel (timing mode)
	long long decide_units = -1, decide_fallbacks = 0; // of the last bmh_decide_device call (bmh_last_decide_stats)
	float decide_ms = -1.f;
	// pass B's planning on the device (wanted.hip): bmh_wanted_cigar_device, and bmh_sam_batch with the switch on
	bool wanted_device = false;               // bmh_ctx_set_wanted_device
	DevBuf d_refidx;                          // (offset, len) of every reference sequence, resident (bmh_ctx_set_refidx)
	int refidx_n = 0;                         // its records, 0 = none
	std::vector<bmh_refspan_t> h_refidx;      // the host's copy of it: a table with the same records is not uploaded again
	long long refidx_l_pac = 0;               // bns->l_pac it was set with
	DevBuf d_wanted;                          // a call's block: offsets, parameters, want list, regions, records, keys, sums, status, results
	void *h_wstat = nullptr;                  // pinned: the two status records as the host reads them between launches
	hipEvent_t ev_wanted[4] = {};             // around the two groups of planning kernels (timing mode)
	long long wanted_n = -1, wanted_fixed = -1, wanted_redone = -1; // of the last bmh_wanted_cigar_device call (bmh_last_wanted_stats)
	float wanted_ms = -1.f;
	// pass A and pass B as one device session (api.hip): bmh_phase2_device, and bmh_sam_batch with the switch on
	bool phase2_device = false;               // bmh_ctx_set_phase2_device
	bmh_phase2_stats_t p2 = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1.f, -1.f}; // of the last fused call (bmh_last_phase2_stats)
	// pass C of phase 2 on the device (samtext.hip): bmh_sam_text_device, and bmh_sam_batch with the switch on
	bool samtext_device = false;              // bmh_ctx_set_samtext_device
	DevBuf d_refnames;                        // n + 1 offsets, then the names' bytes, resident (bmh_ctx_set_refnames)
	int refnames_n = 0;                       // its names, 0 = none
	std::vector<char> h_refnames;             // the host's copy of it (offsets and bytes): the same names are not uploaded again
	DevBuf d_samtext;                         // a call's block: the upload, then records, plans, sizes, offsets, status
	DevBuf d_sam_out;                         // the text
	void *h_ststat = nullptr;                 // pinned: the status as the host reads it between scan and emit
	hipEvent_t ev_samtext[4] = {};            // around the size kernel and the emit kernel (timing mode)
	bmh_samtext_stats_t stx = {-1, -1, -1, -1, -1, -1, 0, -1.f, -1.f}; // of the last bmh_sam_text_device call (bmh_last_samtext_stats)
	// passes A, B and C as one device session (api.hip): bmh_phase2_text_device, and bmh_sam_batch with the switch on.  Its blocks are
	// d_decide (pass A's), d_wanted (pass B's, the overflow area behind it) and d_samtext (pass C's inputs and work arrays)
	bool phase2_text_device = false;          // bmh_ctx_set_phase2_text_device
	void *h_ptstat = nullptr;                 // pinned: SamtextStatus and SamtextFused as the host reads them behind the scan
	hipEvent_t ev_gather[2] = {};             // around reads_gather_kernel (timing mode)
	bmh_phase2_text_stats_t pt = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1.f, -1.f, -1.f, -1.f, -1.f, -1}; // of the last such call (bmh_last_phase2_text_stats)
	// reads to SAM text with the regions resident between the phases (bmh_reads_sam_device: chain2reg.hip's hand-off, api.hip's session)
	hipEvent_t ev_plan[2] = {};               // around table_plan_kernel (timing mode)
	bmh_reads_sam_stats_t rs = {-1, -1, -1, -1, -1, -1, -1, -1.f, -1, -1}; // of the last such call (bmh_last_reads_sam_stats)
	DevBuf d_msw; // mate rescue on the device (matesw.hip): status words, counts, region arena, pair records, hits, reads, machines, tasks, results
	// ... over a region table (matesw_resident): behind those the output table, offsets first, and n_sw per pair
	DevBuf d_mswt;                            // its filter stage: plan record, per-wave parts, per-pair records, block sums
	DevBuf d_mswin;                           // bmh_matesw_table_device's upload: read offsets, region offsets, regions, reads
	hipEvent_t ev_mswt[6] = {};               // around the filter, pack and merge kernels (timing mode)
	bmh_matesw_table_stats_t mt = {-1, -1, -1, -1, -1, -1, -1, -1, -1.f, -1.f, -1.f}; // of the last such call (bmh_last_matesw_table_stats)
	// paired-end reads to SAM text with the region table resident from phase 1 through mate rescue to phase 2 (bmh_pairs_sam_device)
	DevBuf d_pbase;                           // the bases for the rescue: 64-bit offsets, the reads, 16 zero bytes (copied from seeding's pool)
	bmh_pairs_sam_stats_t ps = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1.f, -1, {0, 0, 0, 0, 0, 0}}; // of the last such call (bmh_last_pairs_sam_stats)
	bool park_consumed = false;               // the last bmh_pairs_sam_finish on this context consumed its handle (bmh_pairs_finish_consumed)
};

namespace bmh {

// the caller's gate around a device section (bmh_set_device_gate), held for the lifetime of the guard
extern bmh_gate_fn g_gate_enter, g_gate_leave;
struct GateGuard {
	bmh_gate_fn leave;
	GateGuard() : leave(g_gate_leave)
	{
		if (g_gate_enter) g_gate_enter();
	}
	~GateGuard()
	{
		if (leave) leave();
	}
	GateGuard(const GateGuard &) = delete;
	GateGuard &operator=(const GateGuard &) = delete;
};

int set_hip_error(bmh_ctx *ctx, hipError_t e, const char *what);

// bmh_seed_batch's per-read tables where they lie on the device after its kernels (fmindex.hip), for a consumer that stays there
struct DevSeedTables {
	int n_reads;
	const int *len;               // read lengths
	const uint32_t *coff;         // n_reads + 1 call offsets
	const bmh_smem_call_t *calls; // in per-read call order, .first relative to the read's intervals
	const uint64_t *ioff;         // n_reads + 1 interval offsets
	const bmh_smem_intv_t *intv;
	const uint64_t *sa_off, *sa_pos; // per interval: where its positions start (UINT64_MAX: none); the positions
	uint64_t n_calls, n_intv, n_pos;
	const uint8_t *pool;      // the reads as the seeding stage uploaded them, base codes, ...
	const uint64_t *read_off; // ... read r at pool + read_off[r]; at least 16 bytes of padding behind the last one
	// Everything here points into ctx->d_scratch (the chainer's output into ctx->d_chain): a consumer must neither grow nor write
	// d_scratch while it reads them.  The chains-to-regions driver relies on that: it gives launch_sw explicit caps, so that its
	// cap reduction in d_scratch is not taken, and calls nothing else that uses d_scratch (today: launch_global's slab only).
};
// the device chainer's compact output where chain_place_kernel leaves it (in ctx->d_chain): per read the exclusive sums of its chains
// and kept seeds, per chain its seed count, the seeds; n_keys: per read its chains before the filter
struct DevChains {
	int n_reads;
	const unsigned long long *coff, *soff; // n_reads + 1 each
	const uint32_t *cn;
	const bmh_seed_t *seeds;
	const uint32_t *n_keys;
	unsigned long long tc, ts; // chains and seeds of the batch
	unsigned long long n_equal; // look-ups that met an equal key
	float kernel_ms;            // the chain kernel's duration with kernel timing on, else -1
};
int chain_compact_device(bmh_ctx *ctx, const bmh_chain_opt_t *o, int64_t l_pac, const DevSeedTables &t, DevChains *out);
typedef int (*SeedTablesFn)(bmh_ctx *ctx, const DevSeedTables &t, void *user);
// bmh_seed_batch up to its device tables, then fn on them (on the context's stream, inside the same gate); returns fn's result.
// Capacities grow inside; env BMH_CHAIN_INIT_CAP (test knob) starts them at that many entries.
int seed_tables_device(bmh_ctx *ctx, const bmh_smem_opt_t *o, int max_occ, int n_reads, const bmh_read_t *reads, SeedTablesFn fn, void *user);
// A batch's regions where c2r_place_kernel left them, in ctx->d_c2r: read r's at reg[roff[r] .. roff[r + 1]), and what table_plan_kernel
// found in them (host/handoff_core.h's bmh_ho_plan_t fields).  Valid until the next call that uses d_c2r; nothing phase 2 allocates does.
// A table mate rescue left in ctx->d_msw has the same form; pair_kmax: what its mates add (bmh_ho_pairs), 0 for single-end reads.
struct ResidentRegs {
	const unsigned long long *roff = nullptr; // n_reads + 1
	const bmh_alnreg_t *reg = nullptr;
	long long total = 0, kmax = 1, opool_cap = 0;
	bool neg = false;
	long long pair_kmax = 0;
};
// bmh_seed_chain_regs_batch's checks and its run for bmh_reads_sam_device (chain2reg.hip): the context's three switches are neither read
// nor written, the de-duplication runs at o->mask_level_redun, drop-exact with MEM_F_NO_EXACT in o->flag, and the driver ends behind
// c2r_place_kernel and table_plan_kernel: *out, and ctx->rs up to the hand-off.  reads_regs_check refuses before anything is uploaded.
int reads_regs_check(bmh_ctx *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                     int min_seed_len, const char *who);
int reads_regs_resident(bmh_ctx *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                        int min_seed_len, const bmh_sam_opt_t *o, ResidentRegs *out);
// The same run for bmh_pairs_sam_device: no plan over the table (mate rescue changes it first; out->kmax, opool_cap and neg stay as
// they start), the bases kept for the rescue, and with `collect` mem_pestat's word per pair under *o, brought down in the wait that
// brings the status words.  ctx->rs and what bmh_last_pestat_candidates answers are not touched.
struct PairsPhase1 {
	ResidentRegs regs;                        // in ctx->d_c2r
	const uint8_t *pool = nullptr;            // in ctx->d_pbase: matesw_resident's form, nothing else writes that buffer
	const unsigned long long *soff = nullptr; // n_reads + 1
	std::vector<uint32_t> cand;               // n_reads / 2 words, with collect
	long long regions_in = 0;                 // before the de-duplication
	long long d2h_bytes = 0;                  // what the hand-off's one wait brought down
};
int pairs_regs_resident(bmh_ctx *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                        int min_seed_len, const bmh_sam_opt_t *o, bool collect, PairsPhase1 *out);
// table_plan_kernel (chain2reg.hip) over any table of that form: host/handoff_core.h's fold per read with the paired-end clause and,
// n_sw not NULL, the sum of n_sw[0 .. n_reads / 2).  rec: kTablePlanRecBytes, which the caller has zeroed on the stream (the ticket
// starts at 0), part: table_plan_part_bytes(n_reads), both device memory the caller owns; cap: the table's room in records; err: set to
// BMH_E_ARG where the offsets leave it.  Timed by ctx->ev_plan.
constexpr size_t kTablePlanRecBytes = 64;
size_t table_plan_part_bytes(int n_reads);
int launch_table_plan(bmh_ctx *ctx, const bmh_sam_opt_t &o, int n_reads, const unsigned long long *d_roff, const bmh_alnreg_t *d_reg, unsigned long long cap,
                      const int *d_n_sw, void *d_part, void *d_rec, int *d_err);
// ... its record as it came down into *out (roff and reg are left alone) and *n_sw_sum; false: not every wave has reported, or a sum is negative
bool table_plan_read(const void *h_rec, int n_reads, ResidentRegs *out, long long *n_sw_sum);
// Mate rescue over a resident table (matesw.hip): reads 2p and 2p + 1 are mates, read k's bases d_pool[d_soff[k] .. d_soff[k + 1]) with 16
// bytes of padding behind the last, its regions in.reg[in.roff[k] .. in.roff[k + 1]) (in.total of them; the other fields are not read).
// Fills out->roff, out->reg and out->total, and *d_n_sw (n_pairs entries): all in ctx->d_msw, valid until the next call that uses that
// buffer, so `in` must not lie there.  Between its first launch and its return the host reads the 64-byte plan record, 16 bytes per
// round and the 16-byte total.  ctx->dstats and ctx->mt are the call's.  The caller holds the gate and has checked l_pac against the
// resident reference.  plan_opt not NULL (bmh_pairs_sam_device): table_plan_kernel runs over the output table under *plan_opt and its
// record comes down in the copy that brings the total: out's other fields and *n_sw_sum are filled from it, no wait is added, and
// ctx->mt.mid_bytes counts its 64 bytes.
int matesw_resident(bmh_ctx *ctx, int64_t l_pac, int n_pairs, const uint8_t *d_pool, const unsigned long long *d_soff, const ResidentRegs &in,
                    const bmh_pestat_t pes[4], const bmh_matesw_opt_t *o, float mask_level_redun, ResidentRegs *out, int **d_n_sw,
                    const bmh_sam_opt_t *plan_opt = nullptr, long long *n_sw_sum = nullptr);
// After an error inside a driver's enqueued section (chain2reg.hip, matesw.hip): nothing of the call is left running, and the
// extension and Smith-Waterman kernels' error flag is clean for the next call; rc and the context's error text stay the answer.
int abandon_call(bmh_ctx *ctx, int rc);
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; } // the drivers' buffers are laid out in 256-byte steps
// every host wait for a stream goes through here (bmh_set_wait_mode)
extern int g_wait_blocking;
inline hipError_t stream_wait(bmh_ctx *ctx, hipStream_t s)
{
	if (!g_wait_blocking || !ctx->ev_wait) return hipStreamSynchronize(s);
	const hipError_t e = hipEventRecord(ctx->ev_wait, s);
	return e != hipSuccess ? e : hipEventSynchronize(ctx->ev_wait);
}
int ensure(bmh_ctx *ctx, DevBuf &b, size_t bytes);
int ensure_host(bmh_ctx *ctx, DevBuf &b, size_t bytes); // same, pinned host memory

#define BMH_HIP(ctx, call)                                                   \
	do {                                                                     \
		hipError_t e_ = (call);                                              \
		if (e_ != hipSuccess) return bmh::set_hip_error((ctx), e_, #call);   \
	} while (0)

// kernel launchers (defined next to the kernels)
// grid cap of the extension kernels: enough blocks to keep every wave slot refilled (256 CUs x 32 waves x 4),
// each block walks its bin with a grid stride
constexpr long long kPersistentGrid = 256LL * 32 * 4;

// gap costs the extension kernels are exact for: o+e within 16 bits and e below 2^14.  The bound is empirical:
// e = 25535 and 65535, and o_ins+e_ins = 70000, gave other extensions than the reference in every family, and
// tests/test_score_domain_gpu.py pins e = 16383 as exact; the cause is not established
inline bool ext_gaps_too_large(const bmh_params_t &p)
{
	return (long long)p.o_del + p.e_del > 65535 || (long long)p.o_ins + p.e_ins > 65535 || p.e_del > 16383 || p.e_ins > 16383;
}
// dispatcher: classifies the tasks by query length on the device and runs each bin on its kernel
// d_n (nullable): device-side count <= n of the entries of d_order (or of d_tasks) that are tasks; kind: which
// BinHint slot the launch reads and refreshes
int launch_extend(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n,
                  bmh_ext_result_t *d_res, const uint32_t *d_order, int qmax, const uint32_t *d_n = nullptr, int kind = 0);
int launch_seedext(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_seed_task_t *d_tasks, int64_t n,
                   bmh_seed_result_t *d_res, int qmax);
const uint32_t *seedext_counters(const bmh_ctx *ctx); // the four list lengths of the last launch_seedext, on the device
inline long long ext_resident_waves(const bmh_ctx *ctx, int waves_per_simd) { return (long long)ctx->ncu * 4 * waves_per_simd; }
// the LDS kernel holds 12 bytes per query column in 160 KiB: queries up to this many columns (launch_extend_lds)
constexpr int kLdsQcap = 13632;
// the wide kernel's LDS variant holds 13 bytes per column: up to this many; longer queries use its HBM slab (extend_wide.hip)
constexpr int kWideLdsQcap = 12544;
int launch_extend_wide(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n, bmh_ext_result_t *d_res,
                       const uint32_t *d_order, const uint32_t *d_count, int qmax, long long grid_cap = 0);
// starts the span bmh_extend_wide_stats reports on: one flat extension batch, or the four rounds of a fused per-seed call
int wide_stats_begin(bmh_ctx *ctx);
int launch_extend_lds(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n,
                      bmh_ext_result_t *d_res, const uint32_t *d_order, const uint32_t *d_count, int qmax, long long grid_cap = 0);
constexpr int kSortKeysHost = 2048; // == kSortKeys in extend_dispatch.hip
int sort_tasks_begin(bmh_ctx *ctx, int64_t n, uint32_t **counts, uint32_t **lists);
// d_total (nullable): receives the sum of the bin sizes
// d_payload (nullable): one byte per input position, placed in d_plists (kSortBins x n bytes) exactly as the index is in lists
int sort_tasks_finish(bmh_ctx *ctx, int64_t n, const uint32_t *d_order, unsigned blocks, const uint32_t *d_n = nullptr,
                      uint32_t *d_total = nullptr, const uint8_t *d_payload = nullptr, uint8_t *d_plists = nullptr);
int launch_global_lane(bmh_ctx *ctx, int c, const uint8_t *d_pool, const bmh_glb_task_t *d_tasks, int64_t n,
                       bmh_glb_result_t *d_res, uint32_t *d_cigar, const uint32_t *d_order, const uint32_t *d_count,
                       int rows_cap, const uint8_t *d_band = nullptr);
int launch_global_narrow(bmh_ctx *ctx, int wlo, const uint8_t *d_pool, const bmh_glb_task_t *d_tasks, int64_t n, bmh_glb_result_t *d_res,
                         uint32_t *d_cigar, const uint32_t *d_order, const uint32_t *d_count, int rows_cap, const uint8_t *d_band = nullptr);
constexpr int kExtBins = 6;        // length bins of the extension dispatcher (the 16-bit kernels)
constexpr int kWideBin = 6;        // ... and the int32 kernel's bin, used only with bmh_ctx_set_wide_extension on
constexpr int kSortBins = 8;       // bins the shared counting sort can tell apart (extension 6, global 8, Smith-Waterman 8)
constexpr int kGrpTcapHost = 1024; // == kGrpTcap in extend_grp.hip

// ---- the extension dispatcher's binning rule, for every kernel that fills binkey[] and the histogram: sort_hist_kernel over
// tasks that exist (extend_dispatch.hip), and the fused per-seed record's kernels that bin a task while they make it (seedext.hip)
constexpr int kCapBin = 7;          // tasks past the launch's qmax: listed, never launched
constexpr int kSortBlocks = 512;    // most blocks a pass of the sort uses
constexpr uint16_t kNoTask = 0xffff; // binkey of an entry that holds no task (a seed without the flank): counted and placed nowhere
static_assert(kSortBins * kSortKeysHost <= kNoTask, "binkey is 16 bits wide and keeps one value for entries without a task");

__device__ __forceinline__ int ext_bin_of(int qlen, int tlen, int mode)
{
	// mode 0: lane-per-task kernels (qlen <= 256); 1: LDS kernel only; 2: one task per wave; 3: four tasks per wave;
	// 4: like 0 plus the four-lanes-per-task kernel for qlen <= 512
	if (mode == 1 || qlen < 1) return 5;
	if (mode == 3 && qlen <= 256 && tlen > kGrpTcapHost) return 3; // the group kernels stage the target in LDS
	return qlen <= 32 ? 0 : qlen <= 64 ? 1 : qlen <= 128 ? 2 : qlen <= 256 ? 3 : (qlen <= 512 && mode == 4) ? 4 : 5;
}

// bin 6: the task leaves the 16-bit kernels' domain (with the switch on; the gap costs are checked per batch on the host)
__device__ __forceinline__ bool ext_goes_wide(int qlen, int h0, int max_mat)
{
	return (long long)max(h0, 0) + (long long)qlen * max_mat > kScoreLimit || qlen > kLdsQcap;
}

// sort key inside a bin: query-length bucket (major; lanes of a wave then share the unused leading columns,
// which the lane kernels skip), h0 bucket, and expected row count (minor; lanes of a wave then finish together).
// rows run at most to tlen, and the band leaves the query after ~qlen+w <= 2*qlen rows (ksw.c:418).
// (With the lane kernels' early stop, DESIGN.md 4.3, a good flank ends near row qlen instead.  Two minor keys that follow that -- h0 to
// the base, and tlen - qlen -- were measured level or slower than this one, profiles/ext_stop.md, so it stays.)
// cls >= 0: the class of the band the lane kernel will run the task on (bmh_extband_class) stands in the h0 bucket's
// place -- with a band pass the band decides the interval's width, and narrowed and un-narrowed tasks must not share waves.
__device__ __forceinline__ int ext_sort_key(int bin, int qlen, int tlen, int h0, int cls = -1)
{
	if (bin > 4) return 0;
	const int qlo = bin == 0 ? 1 : (16 << bin) + 1, qsh = bin < 2 ? 1 : bin; // 16 query-length buckets per bin
	const int rows = min(tlen, 2 * qlen + 8) >> (bin > 2 ? bin - 2 : 0);
	// h0 decides how wide the live interval is (cells stay non-zero within ~h0-o-e of the diagonal), so lanes
	// with a similar h0 need the same 8-column blocks
	return ((max(qlen - qlo, 0) >> qsh) * 8 + (cls >= 0 ? cls : min(max(h0, 0) >> 4, 7))) * 16 + min(rows >> 4, 15);
}

struct ExtBinRule { // what a launch fixes for all of its tasks
	int mode;       // see ext_bin_of
	int wide;       // 0 switch off, 1 per task, 2 every task
	int max_mat, qmax;
	bmh_ext_result_t *out; // results, for the failure record of a task past qmax
	int *err_flag;
};

// bin and sort key of ONE task as binkey holds them (bin * kSortKeys + key).  Past qmax: the failure record of the kernels, here,
// since the bins that qmax calls empty are not launched
__device__ __forceinline__ int ext_task_bin(const ExtBinRule &r, int qlen, int tlen, int h0)
{
	return qlen > r.qmax ? kCapBin : r.wide && (r.wide == 2 || ext_goes_wide(qlen, h0, r.max_mat)) ? kWideBin : ext_bin_of(qlen, tlen, r.mode);
}

__device__ __forceinline__ int ext_binkey_of(const ExtBinRule &r, int qlen, int tlen, int h0, size_t idx, int cls = -1)
{
	const int bin = ext_task_bin(r, qlen, tlen, h0);
	if (bin == kCapBin) {
		int *p = (int *)(r.out + idx);
		p[0] = INT32_MIN, p[1] = p[2] = p[3] = p[4] = p[5] = 0;
		atomicExch(r.err_flag, BMH_E_RANGE);
	}
	return bin * kSortKeysHost + ext_sort_key(bin, qlen, tlen, h0, cls);
}

// The dispatcher in two halves, for a caller whose own kernel makes the tasks and bins them in the same pass (the fused
// per-seed record).  Between the two calls the caller enqueues that kernel on ctx->stream with at most p.blocks blocks: for
// entry i of 0..n-1 it writes p.binkey[i] = ext_binkey_of(p.rule, ...) and counts it in p.hist -- or kNoTask and nothing.
struct ExtBinned {
	ExtBinRule rule;
	uint32_t *hist;   // kSortBins * kSortKeys counters, zeroed
	uint16_t *binkey; // n entries
	unsigned blocks;
	uint8_t *band; // non-null: the launch has a band pass (extend_dispatch.hip), which bins the tasks itself.  The caller's kernel then
	               // only marks: binkey[i] = 0 for an entry with a task, kNoTask without, and it leaves hist alone
	bool tiny; // the bin-size hint calls the batch (almost) empty: rule.mode sends every task to bin 5, and one launch of the
	           // any-length kernel walks that list (as launch_extend does for a device-counted list)
};
int extend_binned_begin(bmh_ctx *ctx, int64_t n, bmh_ext_result_t *d_res, int qmax, int kind, ExtBinned *p);
// d_total (nullable): receives the number of tasks, i.e. the sum of the bin sizes
int extend_binned_finish(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n, bmh_ext_result_t *d_res,
                         int qmax, int kind, const ExtBinned &p, uint32_t *d_total);

int launch_extend_grp(bmh_ctx *ctx, int nv, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n,
                      bmh_ext_result_t *d_res, const uint32_t *d_order, const uint32_t *d_count);
int launch_extend_lanex(bmh_ctx *ctx, int lpt, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n,
                        bmh_ext_result_t *d_res, const uint32_t *d_order, const uint32_t *d_count, int min_count);
int launch_sw(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_sw_task_t *d_tasks, int64_t n, bmh_sw_result_t *d_res,
              int qcap, int tcap, int qmin);
// ksw_u8 holds o+e in 8-bit lanes (reference ksw.c:125-128), where 256 and more wrap; the kernels do not restate that,
// so byte-mode tasks under such penalties are refused (BMH_E_RANGE)
inline bool sw_byte_gaps_wrap(const bmh_params_t &p) { return p.o_del + p.e_del > 255 || p.o_ins + p.e_ins > 255; }
int launch_sw_lane(bmh_ctx *ctx, int b, bool corr, bool word, const uint8_t *d_pool, const bmh_sw_task_t *d_tasks, int64_t n,
                   bmh_sw_result_t *d_res, const uint32_t *d_order, const uint32_t *d_count, uint16_t *d_rm, int rows_cap,
                   int grid, int pass2, uint32_t *d_next);
bool sw_wave_fits(int64_t n, int qcap, int tcap);
int launch_sw_wave(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_sw_task_t *d_tasks, int64_t n, bmh_sw_result_t *d_res, int max_cols,
                   int tcap, const uint32_t *d_order = nullptr, const uint32_t *d_count = nullptr);
// skip_long: sw_long_kernel has taken what sw_long_takes (bmh_ctx_set_wide_sw on)
int launch_sw_generic(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_sw_task_t *d_tasks, int64_t n,
                      bmh_sw_result_t *d_res, const uint32_t *d_order, const uint32_t *d_count, int qcap, int tcap, int wave_cols = 0,
                      bool skip_long = false);
// the long-query Smith-Waterman kernel (sw_long.hip): 5 bytes of state per padded query column; padded queries up to kSwLongLdsCols
// columns keep it in LDS (20 KiB: seven waves per CU at the cutoff, more for shorter batches), longer ones in an HBM slab
constexpr int kSwLongLdsCols = 4096;
constexpr long long sw_long_state_bytes(int cols) { return 5LL * cols; }
int launch_sw_long(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_sw_task_t *d_tasks, int64_t n, bmh_sw_result_t *d_res,
                   const uint32_t *d_order, const uint32_t *d_count, int qmax, int qmin, int tcap, int wave_cols);
int launch_extend_lane(bmh_ctx *ctx, int c, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n,
                       bmh_ext_result_t *d_res, const uint32_t *d_order, const uint32_t *d_count, bool exact, const uint32_t *d_skip = nullptr,
                       const uint8_t *d_bands = nullptr); // d_bands (nullable): one byte beside every entry of d_order, see the kernel
int launch_extend_reg(bmh_ctx *ctx, int ns, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n,
                      bmh_ext_result_t *d_res, const uint32_t *d_order, const uint32_t *d_count, int max_count = 0, long long grid_cap = 0);
// The global wave kernel (global_kernel.hip) in LDS: H and E int32 [qcap+2] each, the profile 8 bytes [qcap], smat; up to
// 160 KiB.  Queries up to kGlbLdsQcap columns; bin 4's ring variant holds 10 bytes per slot (H, E, two query bytes) in
// power-of-two rings of up to kGlbRingMax slots, so bands with 2*min(w,qlen)+2 <= kGlbRingMax.
constexpr size_t kGlbLdsBytes = 160 * 1024;
constexpr size_t glb_state_bytes(int qcap) { return (size_t)8 * (qcap + 2) + (size_t)8 * qcap + 32; }
constexpr size_t glb_ring_bytes(int ring) { return (size_t)10 * ring + 32; }
constexpr int glb_lds_qcap()
{
	int q = 65536;
	while (glb_state_bytes(q) > kGlbLdsBytes) q -= 64; // (the launch rounds qmax up to a multiple of 64)
	return q;
}
constexpr int glb_ring_max()
{
	int r = 65536;
	while (glb_ring_bytes(r) > kGlbLdsBytes) r >>= 1;
	return r;
}
constexpr int kGlbLdsQcap = glb_lds_qcap();
constexpr int kGlbRingMax = glb_ring_max();
static_assert(kGlbLdsQcap == 10176 && kGlbRingMax == 8192, "the header states these bounds");
// bin 4's tasks (qlen > kGlbLdsQcap): maxima of qlen, tlen and min(w, qlen), and how many; qmax = 0: no bin 4 in this launch
struct GlbLongShape {
	int qmax = 0, tmax = 0, wmax = 0;
	int64_t n = 0;
};
// qmax, tmax, wmax: the bin-2 tasks' (qlen <= kGlbLdsQcap) maxima; wmax: the widest band in stored columns (min(w, qlen)),
// sizes the wave kernel's direction matrix; wgate: the largest w as the tasks carry it -- the device bins by that, so it
// decides which lane kernels are launched; lg: bin 4's shape, or null
int launch_global(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_glb_task_t *d_tasks, int64_t n,
                  bmh_glb_result_t *d_res, uint32_t *d_cigar, const uint32_t *d_order, int qmax, int tmax,
                  int wmax, int wgate, const GlbLongShape *lg);

// mem_sort_and_dedup, one lane per read, in place on read r's slice [off[r], off[r] + cnt[r]) of reg (total records in all); rewrites
// cnt[r] and adds the regions it removed to *removed.  A slice outside the array: BMH_E_ARG into *err (atomicCAS from 0), nothing touched.
// In timing mode ctx->ev_dedup are recorded around the kernel.
int launch_region_dedup(bmh_ctx *ctx, bmh_alnreg_t *d_reg, const unsigned long long *d_off, unsigned long long *d_cnt, int n_reads,
                        unsigned long long total, float mask_level_redun, unsigned long long *d_removed, int *d_err);

// mem_pestat's pair walk (host/pestat_core.h), one lane per pair p over the slices of reads 2p and 2p + 1 of reg (slices as above: the
// counts decide, not the slice lengths); d_cand[p], n_reads / 2 words, receives the word (null: none wanted).  With drop_exact the lane
// first applies mem_test_and_remove_exact (d_len[r] * match) to its slices -- the lone last read of an odd batch included --, rewrites
// cnt[r] and adds what it removed to *removed; d_len and d_removed may be null without it.  A slice outside the array: BMH_E_ARG into
// *err, nothing written.  In timing mode ctx->ev_pestat are recorded around the kernel.
int launch_pestat_collect(bmh_ctx *ctx, bmh_alnreg_t *d_reg, const unsigned long long *d_off, unsigned long long *d_cnt, const int *d_len,
                          int n_reads, unsigned long long total, const bmh_sam_opt_t &o, int64_t l_pac, int match, bool drop_exact, uint32_t *d_cand,
                          unsigned long long *d_removed, int *d_err);

int launch_region_orient(bmh_ctx *ctx, uint8_t *d_pool, size_t rpool_off, const bmh_region_req_t *d_reqs, int64_t n);
int launch_region_finish(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_region_req_t *d_reqs, int64_t n, const bmh_glb_task_t *d_tasks,
                         const bmh_glb_result_t *d_gres, const uint32_t *d_tcig, bmh_region_res_t *d_out, uint32_t *d_cig_out, int cig_cap,
                         char *d_md_out, int md_cap);

// ---- the long round behind launch_region_finish (region_long.hip, bmh_region_cigar_batch_long).  One entry per flagged region, in
// region order; the scans run over pairs of 64-bit sums, one per block of 256 positions and one more for the total
struct RegionLongSum {
	unsigned long long a, b;
};
struct RegionLongEnt { // 64 bytes
	int64_t region;
	uint64_t cigar_off, md_off; // first word / byte in the two dense pools
	int32_t fin, tix;           // final task of round 1 (-1: the no-gap case); its rerun among the long tasks (-1: none, the CIGAR fitted its slot)
	int32_t n_cigar, score, NM, md_len;
	uint32_t flags; // BMH_REGION_*_CUT as round 1 set them
	int32_t bad;    // left out of the round, BMH_E_ARG is in the error word
	int64_t rsv_;
};
// the flagged records of d_res, compacted into d_ent (n_ent of them, as the host counted); d_gres: round 1's task results
int launch_region_long_list(bmh_ctx *ctx, const bmh_region_req_t *d_reqs, const bmh_region_res_t *d_res, int64_t n,
                            const bmh_glb_result_t *d_gres, RegionLongSum *d_bsum, RegionLongEnt *d_ent, int64_t n_ent);
// cigar_off of every entry in a pool of `words` words, and the n_cut tasks of the CIGAR-cut ones (their final try, n_cigar slots)
int launch_region_long_tasks(bmh_ctx *ctx, RegionLongEnt *d_ent, int64_t n_ent, RegionLongSum *d_bsum, const bmh_glb_task_t *d_tasks,
                             bmh_glb_task_t *d_ltasks, int64_t n_cut, uint64_t words);
// behind the rerun: its results against round 1's, the slot CIGARs of the other entries into the pool, NM and md_len of every entry,
// and the scan of md_len: d_bsum[blocks of n_ent].a is the MD pool's size
int launch_region_long_sizes(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_region_req_t *d_reqs, RegionLongEnt *d_ent, int64_t n_ent,
                             const bmh_glb_result_t *d_lres, const uint32_t *d_cig_out, int cig_cap, uint32_t *d_lcig, RegionLongSum *d_bsum);
int launch_region_long_md(bmh_ctx *ctx, const uint8_t *d_pool, const bmh_region_req_t *d_reqs, RegionLongEnt *d_ent, int64_t n_ent,
                          const uint32_t *d_lcig, const RegionLongSum *d_bsum, char *d_lmd, uint64_t md_bytes);

} // namespace bmh
