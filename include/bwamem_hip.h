/*
 * bwamem_hip.h -- C-ABI of libbwamem_hip.so: BWA-MEM's seed-extension hot
 * path (banded affine-gap DP) on AMD Instinct MI355X (gfx950).
 *
 * This is the drop-in boundary for the path named in BASELINE.json
 * (SURVEY.md §8b).  Plain C: pointers, sizes, fixed-width integers; no C++,
 * HIP or torch types appear in any signature.  Citations are relative to the
 * reference tree (peterpengwei/bwa-mem-quickassist, bwa-0.7.8/).
 *
 * Three levels, lowest first:
 *
 *   L2  batch DP         bmh_extend_batch*   replaces N calls of ksw_extend2 (ksw.h:108, ksw.c:379-476)
 *                        bmh_global_batch*   replaces N calls of ksw_global2 (ksw.h:84,  ksw.c:501-584)
 *   L2' per-call drop-in ksw_extend2 / ksw_global2 with the exact ksw.h signatures
 *                        (libbwamem_hip_dropin.so; each call is a batch of one)
 *   L3  extension driver bmh_chain2aln_batch and the fork's own seam
 *                        mem_chain2aln_batched(...) (bwamem.c:580, call site bwamem.c:1110),
 *                        which replace the per-read loop over mem_chain2aln (bwamem.c:730-878)
 *                        inside mem_align1_core_batched (bwamem.c:1086-1120).
 *
 * Error convention: every function returns BMH_OK (0) or a negative
 * BMH_E_* code; nothing is ever silently dropped.  The reference has no error
 * returns on this path (assert/exit: bwamem.c:758,845,1184; malloc_wrap.c:14-19),
 * so the integration stub in INTEGRATION.md aborts on a negative code.
 * There is NO CPU fallback inside this library: without a usable GPU every
 * compute entry point fails with BMH_E_NODEVICE.
 */
#ifndef BWAMEM_HIP_H
#define BWAMEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMH_VERSION 310 /* 0.3.1: bmh_region_cigar_batch (0.3.0: bmh_smem_opt_t grew min_emit_len (20 bytes), mem_align1_core, *_batch_sharded) */

enum {
	BMH_OK = 0,
	BMH_E_NODEVICE = -1, /* no HIP device / HIP runtime error at init        */
	BMH_E_HIP = -2,      /* a HIP call failed; see bmh_last_error()           */
	BMH_E_ARG = -3,      /* invalid argument (NULL, negative size, ...)       */
	BMH_E_RANGE = -4,    /* a task is outside the supported range (see below) */
	BMH_E_NOMEM = -5,    /* host or device allocation failed                  */
	BMH_E_CIGAR_CAP = -6 /* a global task produced more CIGAR ops than its cap */
};

/* ---- scoring / band parameters: the hot-path fields of mem_opt_t
 * (bwamem.h:21-48; defaults bwamem.c:45-75; matrix bwa.c:77-86). Constant for a run. */
typedef struct bmh_params {
	int32_t o_del, e_del, o_ins, e_ins; /* bwamem.h:23-24                             */
	int32_t zdrop;                      /* bwamem.h:28 ; <=0 disables (ksw.c:455)      */
	int32_t a;                          /* match score; only the L3 driver reads it    */
	int32_t w;                          /* opt->w;       only the L3 driver reads it    */
	int32_t pen_clip5, pen_clip3;       /* bwamem.h:26;  only the L3 driver reads it    */
	int8_t mat[25];                     /* bwamem.h:47 ; m = 5                           */
	int8_t pad_[3];
} bmh_params_t;

/* ---- one ksw_extend2 call (ksw.c:379).  32 bytes.
 * Sequences are base codes 0..4, one byte per base, living in a byte pool.
 * With BMH_F_QREV / BMH_F_TREV the sequence is read backwards from the offset:
 * base k = pool[off - k].  That is how the left extension's reversed copies
 * (bwamem.c:813-817) are expressed without materialising them. */
#define BMH_F_QREV 1u
#define BMH_F_TREV 2u
/* target taken from the 2-bit reference resident on the device (bmh_ctx_set_pac): t_off is then a position on
 * bwa's doubled coordinate [0, 2*l_pac) (reference bntseq.c:355-376), walked forwards or, with BMH_F_TREV,
 * backwards; no target bytes are needed in the pool */
#define BMH_F_TPAC 4u
typedef struct bmh_ext_task {
	uint64_t q_off;    /* pool offset of query base 0                     */
	uint64_t t_off;    /* pool offset of target base 0                    */
	uint16_t qlen;     /* ksw_extend2 arg 1                               */
	uint16_t tlen;     /* arg 3                                           */
	int32_t h0;        /* arg 14                                          */
	int16_t w;         /* arg 11 (before the clamp of ksw.c:398-406)      */
	int16_t end_bonus; /* arg 12                                          */
	uint16_t flags;    /* BMH_F_*                                         */
	uint16_t rsv_;
} bmh_ext_task_t;

/* ---- what ksw_extend2 returns (ksw.c:470-475).  24 bytes. */
typedef struct bmh_ext_result {
	int32_t score, qle, tle, gtle, gscore, max_off;
} bmh_ext_result_t;

/* ---- one ksw_global2 call (ksw.c:501).  32 bytes. */
typedef struct bmh_glb_task {
	uint64_t q_off, t_off;
	uint16_t qlen, tlen;
	int32_t w;          /* arg 11                                                   */
	uint32_t cigar_off; /* first uint32 slot of this task in the CIGAR output pool   */
	uint32_t cigar_cap; /* slots reserved; 0 = score only (cigar_==NULL, ksw.c:566)  */
} bmh_glb_task_t;

typedef struct bmh_glb_result {
	int32_t score;   /* return value, ksw.c:565                                  */
	int32_t n_cigar; /* *n_cigar_; if > cigar_cap the CIGAR was NOT fully written */
} bmh_glb_result_t;

/* Supported range (checked on the host, BMH_E_RANGE otherwise):
 *   extend: 0 <= qlen,tlen <= 65535; scores must fit int16 lanes:
 *           h0 + qlen*max(mat) <= 32000; o_ins >= 0 (SURVEY.md §7 hard part 1);
 *           o_del+e_del, o_ins+e_ins <= 65535, e_del, e_ins <= 16383 (also for bmh_seedext_batch);
 *           queries up to 13 632 columns (the LDS kernel's 160 KiB).
 *   extend with bmh_ctx_set_wide_extension(ctx, 1): what the range above refuses goes to an int32 kernel instead:
 *           h0 + qlen*max(mat) <= 2^24 (bmh_seedext_batch: l_query*max(max(mat), a) <= 2^24), any query up to 65535
 *           (with *_device calls: up to bmh_ctx_set_qcap), any gap costs >= the minimums of bmh_ctx_set_params.  The
 *           fused record keeps its flank bound of 65535 and 2*w <= 32767.  Tasks inside the range above keep their kernels.
 *           Mate rescue (bmh_sw_batch / bmh_matesw_batch) has a switch of its own, bmh_ctx_set_wide_sw below; not covered
 *           by either: the 65535 limits of bmh_global_batch and bmh_reg2cigar_batch below.
 *   Smith-Waterman with bmh_ctx_set_wide_sw(ctx, 1): word-mode tasks (no BMH_SW_XBYTE) accept any qlen up to 65535 whatever
 *           qlen*max(mat); scores saturate at 32 767 exactly as ksw_i16's 16-bit lanes do.  Byte mode keeps its limits.
 *   global: qlen,tlen <= 65535 (the uint16 fields of bmh_glb_task_t).  Tasks with up to 10 176 query columns keep H, E and the
 *           profile of the whole row in LDS (16 bytes per column).  Longer ones that no lane kernel takes go to a band-ring
 *           kernel, whose LDS holds 2*min(w,qlen)+2 columns or more, rounded up to a power of two, at 10 bytes each: bands
 *           with min(w,qlen) <= 4 095 (bmh_global_long_stats counts its tasks).  The direction bytes of every wave-kernel task,
 *           min(qlen,2w+1)*tlen, must fit an 8 GiB slab.  Past these, BMH_E_RANGE: for host-buffer calls the batch when a
 *           direction slab does not fit, the task (the rest are delivered) when its band does not fit the ring; *_device calls
 *           size both kernels from bmh_ctx_set_qcap and a band of max(4w,100) and flag the tasks beyond them.
 *           A CIGAR task must let its band reach the end cell (tlen <= qlen + w, qlen <= tlen + w); score-only tasks may not. */

typedef struct bmh_ctx bmh_ctx_t;

int bmh_version(void);
const char *bmh_strerror(int code);
const char *bmh_last_error(const bmh_ctx_t *ctx); /* text of the last failing HIP call */

int bmh_device_count(int *n);
/* One context = one GPU + one HIP stream + grow-only device/pinned workspaces.
 * A context is used by one host thread at a time. */
int bmh_ctx_create(bmh_ctx_t **ctx, int device);
int bmh_ctx_destroy(bmh_ctx_t *ctx);
/* Gap costs must not be negative (BMH_E_RANGE).  With e_del = 0 or e_ins = 0 the parameters serve bmh_global_batch and
 * bmh_global_batch_device alone (ksw_global2 never divides by a gap extension; the reference's extension does, ksw.c:401,404):
 * every other call then answers BMH_E_ARG, as on a context whose parameters were never set. */
int bmh_ctx_set_params(bmh_ctx_t *ctx, const bmh_params_t *p);
/* Run on a caller-owned hipStream_t (passed as void*); NULL restores the context's own. */
int bmh_ctx_set_stream(bmh_ctx_t *ctx, void *hip_stream);
/* Make the 2-bit packed reference (bwaidx_t.pac, reference bwa.h:16; l_pac/4+1 bytes) resident in HBM: enables
 * BMH_F_TPAC tasks and lets the L3 drivers skip the host-side bns_get_seq.  hg38: 0.78 GB, uploaded once. */
int bmh_ctx_set_pac(bmh_ctx_t *ctx, const uint8_t *pac, int64_t l_pac);
int bmh_ctx_sync(bmh_ctx_t *ctx); /* waits for the stream; returns a pending BMH_E_RANGE/CIGAR_CAP of a *_device call */
/* Opt-in int32 extension kernel (see "Supported range"): with enable != 0, extension and fused per-seed batches accept scores up
 * to 2^24, queries up to 65535 and gap costs past 16 bits.  Off by default; the default context refuses them as before. */
int bmh_ctx_set_wide_extension(bmh_ctx_t *ctx, int enable);
/* Opt-in long-query Smith-Waterman kernel: with enable != 0, bmh_sw_batch / _device / _sharded and bmh_matesw_batch accept
 * word-mode tasks with qlen*max(mat) >= 32000 (up to qlen 65535) and run every word-mode task that would otherwise go to the
 * one-lane-per-task slab kernel -- queries past the register kernels, scores of 512 and more -- on one wave per task
 * (bmh_sw_wide_stats counts them).  Results are those of the reference, saturation included: in-range tasks change kernel but
 * not result.  Off by default; the default context refuses such tasks and routes every task as before. */
int bmh_ctx_set_wide_sw(bmh_ctx_t *ctx, int enable);
/* Capacity hint for the *_device entry points, which cannot look at the tasks on the host:
 * the longest query the launch must handle (default 512).  bmh_extend_batch_device and bmh_seedext_batch_device fail longer
 * queries with BMH_E_RANGE (bmh_ctx_sync returns it) and deliver the other tasks of the call: an extension task longer than
 * qcap gets the failure record score = INT32_MIN, the other fields 0; a seed with a left or right flank longer than qcap gets
 * the record of a seed outside the supported range, score = truesc = INT32_MIN, the other fields 0.  For
 * bmh_global_batch_device see "Supported range" above.  The host-buffer entry points ignore qcap. */
int bmh_ctx_set_qcap(bmh_ctx_t *ctx, int max_qlen);

/* A process-wide gate around the DEVICE SECTIONS of the host-buffer entry points below (upload, kernels, download):
 * enter() is called before the first device operation of a call and leave() after its last.  A program that drives the
 * library from many host threads -- the reference runs phase 1 and 2 on n_threads pthreads -- can bound how many of
 * them are inside device sections at once (more only queue up behind one another on the GPU), while the host work of
 * the L3 drivers around those sections (state machines, band logic, text) runs on all threads.  NULL, NULL removes it. */
typedef void (*bmh_gate_fn)(void);
int bmh_set_device_gate(bmh_gate_fn enter, bmh_gate_fn leave);
/* How the host-buffer entry points wait for the GPU, process-wide.  0 (default): spinning on the completion signal --
 * the shortest latency, one core per waiting thread.  1: sleeping until the GPU's interrupt (an event created with
 * hipEventBlockingSync, and hipDeviceScheduleBlockingSync on the devices of contexts created afterwards) -- for programs
 * with as many or more runnable host threads than cores: measured on the preload shim at 16 threads on 16 cores, a third
 * of all CPU time was spent spinning inside these waits. */
void bmh_set_wait_mode(int blocking);

/* ---- L2, host buffers: H2D copy, launch, D2H copy, synchronous on return. */
int bmh_extend_batch(bmh_ctx_t *ctx, const uint8_t *seqpool, size_t pool_bytes,
                     const bmh_ext_task_t *tasks, int64_t n, bmh_ext_result_t *results);
int bmh_global_batch(bmh_ctx_t *ctx, const uint8_t *seqpool, size_t pool_bytes,
                     const bmh_glb_task_t *tasks, int64_t n, bmh_glb_result_t *results,
                     uint32_t *cigar_pool, size_t cigar_pool_words);

/* Leave a sequence pool resident on the device; afterwards bmh_extend_batch(ctx, NULL, 0, ...) and
 * bmh_global_batch(ctx, NULL, 0, ...) run tasks against it without re-uploading (the L3 drivers
 * upload once per batch and then only move task and result records per round). */
int bmh_upload_pool(bmh_ctx_t *ctx, const uint8_t *seqpool, size_t pool_bytes);

/* ---- L2, device-resident buffers: asynchronous on the context's stream.
 * `d_order` (nullable) is a device array of n task indices giving the launch
 * order (e.g. sorted by length for tail balance); results stay at task index. */
int bmh_extend_batch_device(bmh_ctx_t *ctx, const uint8_t *d_seqpool,
                            const bmh_ext_task_t *d_tasks, int64_t n,
                            bmh_ext_result_t *d_results, const uint32_t *d_order);
int bmh_global_batch_device(bmh_ctx_t *ctx, const uint8_t *d_seqpool,
                            const bmh_glb_task_t *d_tasks, int64_t n,
                            bmh_glb_result_t *d_results, uint32_t *d_cigar_pool,
                            const uint32_t *d_order);

/* ---- static shard of one host batch over several contexts (one per GPU,
 * SURVEY.md §8e): contiguous split, one stream per device, no collective. */
int bmh_extend_batch_sharded(bmh_ctx_t *const *ctxs, int n_ctx, const uint8_t *seqpool,
                             size_t pool_bytes, const bmh_ext_task_t *tasks, int64_t n,
                             bmh_ext_result_t *results);
/* The same static split for the other three batches of the DP path (declared here, records defined below): the fused per-seed
 * records, ksw_global2 + traceback, ksw_align2.  Contiguous task ranges like kt_for_batch's (reference kthread_batch.c:44-56,
 * bwamem.c:1313), every device gets the whole pool, results land at their task index; a shard's CIGAR words are copied into the
 * caller's pool task by task.  All four validate every shard before anything is enqueued on any device, so a refused call has
 * no effect (nothing run, nothing written to the caller's arrays); then, inside the device gate, everything is enqueued on every
 * device before any is waited for, and every device is waited for before the call returns, on an error too. */
struct bmh_seed_task; struct bmh_seed_result; struct bmh_sw_task; struct bmh_sw_result;
int bmh_seedext_batch_sharded(bmh_ctx_t *const *ctxs, int n_ctx, const uint8_t *seqpool, size_t pool_bytes,
                              const struct bmh_seed_task *tasks, int64_t n, struct bmh_seed_result *results);
int bmh_global_batch_sharded(bmh_ctx_t *const *ctxs, int n_ctx, const uint8_t *seqpool, size_t pool_bytes,
                             const bmh_glb_task_t *tasks, int64_t n, bmh_glb_result_t *results,
                             uint32_t *cigar_pool, size_t cigar_pool_words);
int bmh_sw_batch_sharded(bmh_ctx_t *const *ctxs, int n_ctx, const uint8_t *seqpool, size_t pool_bytes,
                         const struct bmh_sw_task *tasks, int64_t n, struct bmh_sw_result *results);

/* ---- L2.5: one record per SEED -- the accelerator record the fork sketched and never used
 * (ext_param_t / ext_res_t, reference bwamem.c:553-577).  The device runs, for every seed, what
 * mem_chain2aln does between bwamem.c:810 and :866: the left extension on the reversed flanks (up to MAX_BAND_TRY = 2
 * band widths, retry rule :828), the clip-or-reach-the-end decision (:831-837), the right extension started from the
 * LEFT SCORE (:842,854; retry rule :856), its decision (:859-865) -- and returns the finished region fields.  Inside
 * the library that is four dependent rounds of ksw_extend2 batches (left, left at 2w, right, right at 2w), the
 * retry lists and the right tasks built ON THE DEVICE from the previous round's results; nothing returns to the host
 * in between, the whole call is asynchronous on the context's stream.
 * ext_param_t gave the flanks as four pointers + lengths; here they are expressed by the seed's position inside the
 * read and inside the chain's reference window [rmax0,rmax1) (bwamem.c:740-757), which is what the driver has. */
typedef struct bmh_seed_task { /* 40 bytes */
	uint64_t q_off;   /* pool offset of query base 0 (the whole read, base codes)                                  */
	uint64_t t_off;   /* pool offset of rseq[0], i.e. of window base rmax0; with BMH_F_TPAC the doubled-coordinate
	                     position rmax0 itself (the window is then read from the resident 2-bit reference)          */
	int32_t l_query;  /* read length                                                                                */
	int32_t qbeg, len;/* the seed on the query: mem_seed_t.qbeg / .len (bwamem.c:168-171); h0 = len * a            */
	int32_t rbeg;     /* the seed inside the window: mem_seed_t.rbeg - rmax0  (left target length, bwamem.c:815)    */
	int32_t wlen;     /* rmax1 - rmax0                                                                              */
	uint16_t flags;   /* BMH_F_TPAC or 0                                                                            */
	uint16_t rsv_;
} bmh_seed_task_t;

typedef struct bmh_seed_result { /* 32 bytes; ext_res_t (bwamem.c:568-577) in 32-bit fields */
	int32_t qb, qe;        /* mem_alnreg_t.qb / .qe                                    (bwamem.c:832,835,860,863,866) */
	int32_t rb, re;        /* mem_alnreg_t.rb / .re MINUS rmax0 (window-relative)                                     */
	int32_t score, truesc; /* mem_alnreg_t.score / .truesc                                                            */
	int32_t w;             /* max(aw[0], aw[1]), bwamem.c:875                                                         */
	int32_t n_ext;         /* ksw_extend2 calls the reference would have made for this seed (0..4)                    */
} bmh_seed_result_t;

/* Range: qbeg, l_query-qbeg-len, rbeg, wlen-rbeg-len <= 65535, 2*w <= 32767, and the extension limits above. */
int bmh_seedext_batch(bmh_ctx_t *ctx, const uint8_t *seqpool, size_t pool_bytes, const bmh_seed_task_t *tasks, int64_t n,
                      bmh_seed_result_t *results); /* pool == NULL: the pool left by bmh_upload_pool() */
int bmh_seedext_batch_device(bmh_ctx_t *ctx, const uint8_t *d_seqpool, const bmh_seed_task_t *d_tasks, int64_t n,
                             bmh_seed_result_t *d_results);
/* Two-step form of bmh_seedext_batch for callers that overlap host work with the device: _submit stages the tasks and
 * enqueues everything (uploads, the four rounds, the download into the context's pinned buffer) and returns at once;
 * _wait blocks until the results are there and copies them out.  One submission may be in flight per context. */
int bmh_seedext_submit(bmh_ctx_t *ctx, const bmh_seed_task_t *tasks, int64_t n);
int bmh_seedext_wait(bmh_ctx_t *ctx, bmh_seed_result_t *results);
typedef struct bmh_seedext_stats { /* of the last completed bmh_seedext_batch / _wait (host-buffer forms only) */
	int64_t seeds, left_tasks, left_retries, right_tasks, right_retries;
} bmh_seedext_stats_t;
int bmh_seedext_stats(const bmh_ctx_t *ctx, bmh_seedext_stats_t *st);

/* ---- kernel timing: HIP events recorded on the context's stream around the
 * dominant kernel of the last *_device call.  ms < 0 if none. */
int bmh_last_kernel_ms(bmh_ctx_t *ctx, float *ms);
int bmh_set_kernel_timing(bmh_ctx_t *ctx, int enable);
/* Per-kernel duration of the last extension launch, one entry per query-length bin of the dispatcher:
 * qlen <= 32, <= 64, <= 128, <= 256, <= 512, longer (LDS kernel).  -1 when timing was off. */
int bmh_last_extend_bin_ms(bmh_ctx_t *ctx, float ms[6]);
/* With timing on, every dispatcher launch (a fused per-seed call makes four) waits for its kernels and adds their per-bin durations
 * to running sums: ms[b] = the sum for bin b, *launches (nullable) = dispatcher launches counted; reset != 0 clears the sums. */
int bmh_extend_bin_ms_sum(bmh_ctx_t *ctx, double ms[6], long long *launches, int reset);
/* What the last extension launch (a flat batch, or the four rounds of a fused per-seed call) sent to the int32 kernel:
 * *tasks = its tasks (0 with the wide extension off), *ms = its kernel time (-1 when timing is off).  Waits for the stream. */
int bmh_extend_wide_stats(const bmh_ctx_t *ctx, int64_t *tasks, float *ms);
/* Per-kernel duration of the last global-alignment launch: the 64-slot lane kernel (w <= 31), the 128-slot one (w <= 63),
 * the one-wave-per-task kernel (everything else).  -1 when timing was off. */
int bmh_last_global_bin_ms(bmh_ctx_t *ctx, float ms[3]);
/* Diagnostic: the band the device computed for every task of the context's most recent global-alignment launch, in front of
 * its sort (the lane kernels run each task on the band its result needs).  bands[k] belongs to the task at input position k --
 * entry k of d_order where the launch had one, else task k; 255 stands for every band of 255 and more.  n must be that launch's task
 * count.  BMH_E_ARG when it is not, or when the launch ran no band pass (BMH_GLB_NARROW=0, BMH_GLB_MODE=wave, nothing
 * launched yet, or the workspace was grown since by bmh_ctx_reserve_device).  A call that makes several global launches leaves
 * the last one's bands.  Waits for the stream and copies n bytes; the launches themselves do nothing for it. */
int bmh_last_global_bands(bmh_ctx_t *ctx, uint8_t *bands, int64_t n);
/* Diagnostic: how many tasks of the context's most recent global-alignment launch its sort put into each of the dispatcher's eight
 * bins -- 0, 3, 1, 5: the lane kernels of 64, 96, 128 and 32 slots; 2 and 4: one wave per task; 6 and 7: the exact-band kernel for
 * bands of 0..3 and 4..7 (BMH_GLB_EXACT).  Read from the sort's workspace where the launch left them: the launch does nothing for
 * it, the call waits for the stream and copies 32 bytes.  BMH_E_ARG when no global launch has run, or when any later call has used
 * or grown the sort's workspace (every batch call of the extension, global and Smith-Waterman paths sorts its tasks there). */
int bmh_last_global_bin_counts(bmh_ctx_t *ctx, uint32_t counts[8]);
/* Diagnostic: the DP rows each task of a plain extension launch ran.  The lane-per-task kernels end a flank once no later row can
 * change any of its six results (BMH_EXT_STOP=0 in the environment of bmh_ctx_create turns that off), so this is at
 * most what ksw_extend2 runs.  With cap > 0, bmh_extend_batch and bmh_extend_batch_device keep cap x uint16 on the device, indexed as
 * the result array is -- by task index -- which the lane kernels fill, for indices below cap, where they write a result.  cap = 0
 * (the default): they get a null pointer and do nothing for it. */
int bmh_ctx_set_extend_rows(bmh_ctx_t *ctx, int64_t cap);
/* rows[k] belongs to task k of the most recent plain extension launch: the rows it ran, 0 for a task that ran none or was refused,
 * 0xffff where no lane kernel took it (queries past 128 columns, small batches, the other BMH_EXT_MODEs, an index d_order does not
 * list).  n <= the cap that launch ran with; BMH_E_ARG when it is not or when nothing was recorded.  Waits for the stream and copies
 * 2 n bytes. */
int bmh_last_extend_rows(bmh_ctx_t *ctx, uint16_t *rows, int64_t n);
/* Diagnostic: the band each task of the most recent extension launch with a band pass was run on.  Where the lane-per-task kernels
 * take queries of up to 128 columns -- a flat batch above the small-batch threshold, the two big rounds of the fused per-seed call --
 * a pass in front of the sort computes per task the band its six results need (host/extband_core.h) and those kernels
 * run min(w, that band); the task record keeps its w, and every other kernel family, the retry rounds and tiny lists run the task's
 * own band.  bands[k] belongs to input position k (entry k of d_order, or task k): the band, 255 for "255 or wider" (the task's own
 * is kept), the task's own w for a task the rule leaves alone or no lane kernel takes, 255 for an entry of a fused round that holds
 * no task.  BMH_EXT_NARROW=0 in the environment of bmh_ctx_create turns the narrowing off, and so does an armed rows diagnostic
 * (bmh_ctx_set_extend_rows with cap > 0 -- it reports the rows of the reference's band): the pass then lists every task's own w.
 * n must be that launch's entry count; BMH_E_ARG when it is not or when the launch had no band pass.  Waits for the stream and
 * copies n bytes; the launches themselves do nothing for it. */
int bmh_last_extend_bands(bmh_ctx_t *ctx, uint8_t *bands, int64_t n);
/* What the global-alignment launches of this context so far sent to bin 4, the band-ring kernel (tasks with more than 10 176
 * query columns that no lane kernel takes): *tasks = their number, *ms = the ring kernel's time summed over the launches made
 * with timing on (-1 when timing is off).  The counterpart of bmh_extend_wide_stats.  Waits for the stream. */
int bmh_global_long_stats(const bmh_ctx_t *ctx, int64_t *tasks, float *ms);
/* What the Smith-Waterman launches of this context so far sent to the long-query kernel (bmh_ctx_set_wide_sw): *tasks = their
 * number, *ms = its time summed over the launches made with timing on (-1 when timing is off).  The counterpart of
 * bmh_global_long_stats.  Waits for the stream. */
int bmh_sw_wide_stats(const bmh_ctx_t *ctx, int64_t *tasks, float *ms);
/* Duration of the four rounds of the last fused per-seed launch (left, left at 2w, right, right at 2w), each with the
 * small list-building kernel in front of it.  -1 when timing was off. */
int bmh_last_seedext_round_ms(bmh_ctx_t *ctx, float ms[4]);

/* ---- L3: data carriers of the extension driver, layout-compatible with the
 * reference so that its structs can be passed straight through. */
typedef struct bmh_seed {  /* == mem_seed_t, bwamem.c:168-171 */
	int64_t rbeg;
	int32_t qbeg, len;
} bmh_seed_t;

typedef struct bmh_chain { /* == mem_chain_t, bwamem.c:173-177 */
	int32_t n, m;
	int64_t pos;
	bmh_seed_t *seeds;
} bmh_chain_t;

typedef struct bmh_chain_v { /* == mem_chain_v, bwamem.c:179 */
	size_t n, m;
	bmh_chain_t *a;
} bmh_chain_v;

typedef struct bmh_alnreg { /* == mem_alnreg_t, bwamem.h:50-62 (64 bytes) */
	int64_t rb, re;
	int32_t qb, qe;
	int32_t score, truesc, sub, csub, sub_n, w, seedcov, secondary;
	uint64_t hash;
} bmh_alnreg_t;

typedef struct bmh_alnreg_v { /* == mem_alnreg_v, bwamem.h:64; a is malloc/realloc'd */
	size_t n, m;
	bmh_alnreg_t *a;
} bmh_alnreg_v;

typedef struct bmh_read { /* the two bseq1_t fields the driver reads (bwa.h:18-22) */
	int32_t l_seq;
	const uint8_t *seq; /* base codes 0..4 (after bwamem.c:1093-1094) */
} bmh_read_t;

/* Optional per-chain pre-step, called right before chain `chain` of read `read` would be
 * extended, in the reference's order.  It mirrors `ret = mem_chain2aln_short(...)`
 * (bwamem.c:1104 / :1140): it may append to *av; a return value <= 0 means the chain is
 * done and must not be extended, > 0 means "run mem_chain2aln on it" (bwamem.c:1105). */
typedef int (*bmh_chain_pre_fn)(void *user, int read, int chain, bmh_alnreg_v *av);

/* Replaces, for `n_reads` reads at once, the loop
 *     for each chain c of read r: [pre-step;] mem_chain2aln(opt,l_pac,pac,l_seq,seq,c,&regs[r])
 * (bwamem.c:1101-1107 / :1136-1143).  Regions are APPENDED to regs[r] (kv_pushp semantics,
 * bwamem.c:804; regs[r].a must be NULL or malloc'd), so entries already there take part in
 * the containment test of bwamem.c:769-802.  `pre` may be NULL (every chain is extended). */
int bmh_chain2aln_batch(bmh_ctx_t *ctx, int64_t l_pac, const uint8_t *pac, int n_reads,
                        const bmh_read_t *reads, const bmh_chain_v *chains, bmh_chain_pre_fn pre,
                        void *pre_user, bmh_alnreg_v *regs);

/* The whole loop body of mem_align1_core (bwamem.c:1101-1107 / :1136-1143) for n_reads reads: per chain first
 * mem_chain2aln_short (bwamem.c:495-542) -- its qualifying tests on the host, the ksw_align2 calls of all chains of the
 * batch as ONE bmh_sw_batch, its verdict folded in where the reference calls it -- then, unless that settled the chain,
 * mem_chain2aln as in bmh_chain2aln_batch.  min_seed_len = opt->min_seed_len (the XSUBO threshold, bwamem.c:529). */
int bmh_chains2regs_batch(bmh_ctx_t *ctx, int64_t l_pac, const uint8_t *pac, int n_reads, const bmh_read_t *reads,
                          const bmh_chain_v *chains, int min_seed_len, bmh_alnreg_v *regs);

/* ---- L3, phase 2: the caller of ksw_global2.
 * One request = one alignment region after bwa_fix_xref2, as mem_reg2aln sees it at bwamem.c:1187. */
typedef struct bmh_cigar_req {
	int32_t read;    /* index into reads[]                                              */
	int32_t qb, qe;  /* query interval [qb,qe)                    (mem_alnreg_t.qb/qe)   */
	int64_t rb, re;  /* reference interval, doubled coordinate    (mem_alnreg_t.rb/re)   */
	int32_t truesc;  /* mem_alnreg_t.truesc: band inference + retry test, bwamem.c:1187,1201;
	                    INT32_MIN = ONE bwa_gen_cigar2 call with w_ = reg_w instead of that loop (bwa_fix_xref2, bwa.c:198) */
	int32_t reg_w;   /* mem_alnreg_t.w:      cap of the inferred band, bwamem.c:1191     */
} bmh_cigar_req_t;

typedef struct bmh_cigar_res {
	int32_t score;      /* global alignment score of the last try (bwa_gen_cigar2 *score)   */
	int32_t n_cigar;    /* number of CIGAR words                                             */
	int32_t NM;         /* edit distance, bwa.c:162; -1 if the request was rejected (bwa.c:99) */
	int32_t tries;      /* bwa_gen_cigar2 calls the reference would have made (1..3)          */
	uint32_t cigar_off; /* first word in cigar_pool                                           */
	uint32_t md_off;    /* first byte of the NUL-terminated MD string in md_pool              */
	uint32_t md_len;    /* strlen(MD)                                                         */
	uint32_t rsv_;
} bmh_cigar_res_t;

/* Replaces, for n_req regions at once, the loop of mem_reg2aln (bwamem.c:1187-1201) over
 * bwa_gen_cigar2 (bwa.c:89-172): band inference, up to three banded global alignments per region
 * (one GPU batch per try), NM and MD.  The reference appends the MD string to the CIGAR buffer
 * (bwa.c:136,161-163); here both are returned separately -- INTEGRATION.md shows the two-line glue.
 * Pools: cigar_words >= sum(qlen+tlen+2), md_bytes >= sum(3*(qlen+tlen)+16) always suffice. */
int bmh_reg2cigar_batch(bmh_ctx_t *ctx, int64_t l_pac, const uint8_t *pac, const bmh_read_t *reads, int64_t n_req,
                        const bmh_cigar_req_t *reqs, bmh_cigar_res_t *results, uint32_t *cigar_pool,
                        size_t cigar_words, char *md_pool, size_t md_bytes);

/* ---- L2.6: one record per REGION -- everything bwa_gen_cigar2 (bwa.c:89-172) does with sequence bytes, and the replay of mem_reg2aln's
 * band loop (bwamem.c:1193-1201), on the device, against the 2-bit reference made resident by bmh_ctx_set_pac():
 *   - bns_get_seq of [rb, rb+tl) on the doubled coordinate and the reversal of query and window for reverse-strand hits (bwa.c:100-107):
 *     the oriented copies are written into a device pool, query k at o_off, its window right behind it at o_off + ql;
 *   - the no-gap shortcut's score, sum of mat[t*5+q] (bwa.c:108-114), for a region whose task[0] is -1;
 *   - ksw_global2 + traceback of `tasks` (their q_off / t_off address that oriented pool; cigar_off / cigar_cap a device-side scratch
 *     of `task_cigar_words` words);
 *   - per region the loop over its tries task[0..2]: stop when the score repeats or reaches truesc - a, or after one try when
 *     truesc == INT32_MIN (bwamem.c:1194-1201; equal bands share a task index);
 *   - NM and MD of the final try (bwa.c:134-164), MD with "ACGTN" or, on the reverse strand, "TGCAN".
 * The host keeps what needs no sequence: band inference and the band of each try (bwamem.c:884-891,1187-1191, bwa.c:116-125).
 * Returned per region: the record below, its CIGAR words at cigar_out[k*cig_cap ..] and its MD bytes (no NUL) at md_out[k*md_cap ..].
 * A CIGAR longer than the final task's cigar_cap or cig_cap, or an MD longer than md_cap, is flagged and not returned (the caller
 * redoes those few regions with full capacities, e.g. through bmh_global_batch); score, n_cigar and tries are exact either way. */
#define BMH_REGION_CIGAR_CUT 1u /* n_cigar exceeds the capacity: CIGAR, NM and MD not returned */
#define BMH_REGION_MD_CUT 2u    /* MD longer than md_cap: NM is exact, the MD bytes are not returned */
typedef struct bmh_region_req { /* 48 bytes */
	uint64_t q_src;  /* offset in readpool of query base qb, read orientation, one base code per byte */
	int64_t rb;      /* doubled coordinate of the window's first base; [rb, rb+tl) must not bridge l_pac (bwa.c:99) */
	uint64_t o_off;  /* where the oriented query goes in the device pool (the window follows at o_off + ql) */
	int32_t ql, tl;
	int32_t truesc;  /* INT32_MIN: one try */
	int32_t task[3]; /* index into tasks[] of try 0..2; -1 = no such try; task[0] == -1: the no-gap case */
} bmh_region_req_t;
typedef struct bmh_region_res { /* 24 bytes */
	int32_t score, n_cigar, tries, NM;
	int32_t md_len;
	uint32_t flags; /* BMH_REGION_* */
} bmh_region_res_t;
/* Bytes of a region's MD slot past md_len are unspecified.  readpool: the query windows; opool_bytes: size of the oriented pool the o_off / q_off / t_off fields address.  BMH_E_ARG without a
 * resident reference or with offsets outside the pools. */
int bmh_region_cigar_batch(bmh_ctx_t *ctx, const uint8_t *readpool, size_t readpool_bytes, size_t opool_bytes,
                           const bmh_region_req_t *reqs, int64_t n_req, const bmh_glb_task_t *tasks, int64_t n_tasks,
                           size_t task_cigar_words, int cig_cap, int md_cap, bmh_region_res_t *results, uint32_t *cigar_out,
                           char *md_out);

/* ---- the same call with no region left to the caller: a region record of any CIGAR and MD length.  The regions bmh_region_cigar_batch
 * would flag are finished on the device behind it, where the oriented copies already lie: their final try runs once more with exactly
 * n_cigar slots in one dense CIGAR pool (through the same dispatcher: lane, wave or ring kernel by shape), NM and MD are walked there
 * (host/regfinish_core.h), and the MD bytes go into one dense MD pool, without NUL, as in the slots.
 *   - A region that call would not flag comes back exactly as from it, bytes of the three arrays included.
 *   - A region it would flag: results[k] holds the exact score, n_cigar, tries, NM and md_len; flags has BMH_REGION_LONG beside the cut
 *     bit or bits; its slots in cigar_out / md_out are unspecified; longs[] -- ascending by region -- names its n_cigar words in
 *     long_cigar and its md_len bytes in long_md.  A region whose MD alone was cut has its CIGAR in the pool all the same.
 *   - *longs, *long_cigar and *long_md are malloc'd and the caller's to free(); all three are NULL and *n_long is 0 when nothing was
 *     flagged, and such a call enqueues and waits exactly as bmh_region_cigar_batch does.  Otherwise the long round adds two waits
 *     (the MD pool's size, the download).
 *   - Both pools are dense: the last entry's data ends them.  Behind each the call leaves BMH_REGION_LONG_GUARD bytes of 0xA5 that
 *     were set on the device before the long round's kernels ran and came back with the pool; the call checks them (BMH_E_HIP).
 *   - On any error nothing stays allocated and no output is written.  BMH_E_RANGE when the flagged regions' n_cigar sum to more than
 *     2^32 - 1 words (the tasks' cigar_off is 32 bits wide), before the long round is enqueued, and -- as from the old call -- for a
 *     task no kernel takes; BMH_E_ARG without a resident reference, and if the rerun of a try disagrees with its first run. */
#define BMH_REGION_LONG_GUARD 16
#define BMH_REGION_LONG 4u /* finished by the long round: CIGAR and MD are in the pools bmh_region_cigar_batch_long returned */
typedef struct bmh_region_long { /* 24 bytes */
	int64_t region;     /* index into reqs / results */
	uint64_t cigar_off; /* first word in long_cigar */
	uint64_t md_off;    /* first byte in long_md    */
} bmh_region_long_t;
int bmh_region_cigar_batch_long(bmh_ctx_t *ctx, const uint8_t *readpool, size_t readpool_bytes, size_t opool_bytes,
                                const bmh_region_req_t *reqs, int64_t n_req, const bmh_glb_task_t *tasks, int64_t n_tasks,
                                size_t task_cigar_words, int cig_cap, int md_cap, bmh_region_res_t *results, uint32_t *cigar_out,
                                char *md_out, bmh_region_long_t **longs, int64_t *n_long, uint32_t **long_cigar, char **long_md);
/* Of the context's last successful bmh_region_cigar_batch_long: regions the long round finished, the words and bytes of its two pools,
 * and with bmh_set_kernel_timing on the duration of its kernels (0 when nothing was flagged), else -1.  All -1 before the first call. */
int bmh_last_region_long_stats(const bmh_ctx_t *ctx, int64_t *regions, int64_t *cigar_words, int64_t *md_bytes, float *kernel_ms);

/* Per context, off by default: bmh_reg2cigar_batch -- and through it pass B of phase 2 in all its forms, which redo the regions
 * past their slots with it -- finishes the regions whose CIGAR or MD outgrow the region record's slots through
 * bmh_region_cigar_batch_long, instead of redoing them with oriented copies made on the host.  The records and bytes it returns
 * are the same; where they lie in the two pools may differ.  Without a resident reference, or under BMH_REG2CIGAR_HOST=1, the call
 * takes the path with host copies as before. */
int bmh_ctx_set_region_long(bmh_ctx_t *ctx, int on);
/* Of the context's last bmh_reg2cigar_batch that reached the device: the regions it was given, those the long round finished and
 * those redone with host copies (every region, on the path without the region record).  All -1 before the first call. */
int bmh_last_reg2cigar_stats(const bmh_ctx_t *ctx, int64_t *regions, int64_t *long_device, int64_t *redone_host);

/* Counters of the last bmh_chain2aln_batch call (for the bench / logs). */
typedef struct bmh_driver_stats {
	int64_t rounds, ext_tasks, seeds_extended, seeds_skipped;
	int64_t pool_bytes; /* bytes of sequence shipped to the device for the call */
	int64_t seeds_speculated; /* seeds the device extended ahead of the replay whose result was not needed */
	int64_t short_sw;         /* ksw_align2 calls of mem_chain2aln_short run as one batch (bmh_chains2regs_batch) */
} bmh_driver_stats_t;
int bmh_driver_stats(const bmh_ctx_t *ctx, bmh_driver_stats_t *st);

/* The host-buffer entry points stage transfers of up to 64 MB per direction through pinned buffers owned by the context
 * (they grow on demand).  A caller that creates its contexts ahead of time -- the preload shim does, while the host
 * program is still loading its index -- can reserve them here, so that the first batch does not pay for the
 * allocation.  No counterpart in the reference (it has no device). */
int bmh_ctx_reserve_staging(bmh_ctx_t *ctx, size_t upload_bytes, size_t download_bytes);
/* The same for the device-side workspaces of the host-buffer entry points (sequence pool, task / result records, CIGAR
 * words, the dispatcher's sort lists): growing one of them in the middle of a run frees and re-allocates device memory,
 * which synchronises the device under every other host thread's batch. */
int bmh_ctx_reserve_device(bmh_ctx_t *ctx, size_t pool_bytes, int64_t max_tasks, size_t cigar_words);
/* ... and the two large kernel workspaces, which otherwise grow inside a context's first batches (a hipMalloc of hundreds
 * of megabytes under every other thread's work): the SMEM kernels' interval stacks for batches of up to seed_reads reads of
 * up to seed_read_len bases, and the ksw_global2 lane kernels' direction slab for batches of up to global_tasks tasks with
 * targets of up to global_rows rows.  0 skips either. */
int bmh_ctx_reserve_kernels(bmh_ctx_t *ctx, int seed_reads, int seed_read_len, int64_t global_tasks, int global_rows);

/* ------------------------------------------------------------------------------------------------------------
 * Local Smith-Waterman for mate rescue and short chains.
 * Replaces: kswr_t ksw_align2(qlen, query, tlen, target, m, mat, o_del, e_del, o_ins, e_ins, xtra, qry)
 *           reference bwa-0.7.8/ksw.h:62, ksw.c:341-364 (over ksw_qinit / ksw_u8 / ksw_i16, ksw.c:62-331);
 *           callers mem_matesw (bwamem_pair.c:109-175) and mem_chain2aln_short (bwamem.c:495-542).
 * One record per call; `xtra` is passed through unchanged (KSW_XBYTE/XSTOP/XSUBO/XSTART | threshold, ksw.h:6-9)
 * and the result is field for field kswr_t (ksw.h:14-19), including the byte-mode (16 columns per vector) versus
 * word-mode (8) differences of the striped reference, which are visible in score2/te2 and, rarely, the scores.
 * m = 5 and the matrix / gap penalties come from bmh_params_t.  Inputs outside the exact domain are refused with
 * BMH_E_RANGE: qlen*max(mat) >= 32000, gap penalties above 255, byte-mode tasks that can overflow (qlen*max(mat) + shift
 * >= 255) combined with KSW_XSTART, for which the reference reads uninitialised memory (ksw.c:355-357), and byte-mode
 * tasks when o_del+e_del or o_ins+e_ins reaches 256, which ksw_u8 wraps in its 8-bit lanes (ksw.c:125-128).
 * With bmh_ctx_set_wide_sw on, word-mode tasks are accepted past qlen*max(mat) >= 32000 (qlen up to 65535) with ksw_i16's
 * saturation at 32 767, and run on one wave per task; *_device calls flag a task that kernel cannot hold (BMH_E_RANGE,
 * the others are delivered). */
#define BMH_SW_XBYTE 0x10000u
#define BMH_SW_XSTOP 0x20000u
#define BMH_SW_XSUBO 0x40000u
#define BMH_SW_XSTART 0x80000u
/* query base = complement of the pool byte (3-b; N stays N).  With BMH_F_QREV the query is the reverse complement
 * of the stored mate, so the host needs no second copy of it (reference bwamem_pair.c:130-133). */
#define BMH_F_QCOMP 8u

typedef struct bmh_sw_task {
	uint64_t q_off;  /* query base k = pool[q_off + k], or pool[q_off - k] with BMH_F_QREV */
	uint64_t t_off;  /* target likewise (BMH_F_TREV); with BMH_F_TPAC a doubled-coordinate position */
	uint32_t tlen;
	uint16_t qlen;
	uint16_t flags;  /* BMH_F_QREV | BMH_F_TREV | BMH_F_TPAC | BMH_F_QCOMP */
	uint32_t xtra;   /* ksw_align2's xtra */
	uint32_t rsv;
} bmh_sw_task_t; /* 32 bytes */

typedef struct bmh_sw_result {
	int32_t score, te, qe, score2, te2, tb, qb; /* kswr_t, ksw.h:14-19; unset values are -1 */
	int32_t rsv;
} bmh_sw_result_t; /* 32 bytes */

int bmh_sw_batch(bmh_ctx_t *ctx, const uint8_t *pool, size_t pool_bytes, const bmh_sw_task_t *tasks, int64_t n,
                 bmh_sw_result_t *results);
/* device-resident variant: nothing crosses PCIe; completion is ordered on the context's stream */
int bmh_sw_batch_device(bmh_ctx_t *ctx, const uint8_t *d_pool, const bmh_sw_task_t *d_tasks, int64_t n,
                        bmh_sw_result_t *d_results);

/* ------------------------------------------------------------------------------------------------------------
 * Batched mate rescue: the loop mem_sam_pe runs per pair (reference bwamem_pair.c:251-263) over mem_matesw
 * (bwamem_pair.c:109-175), for a whole chunk of pairs.
 *   reads[2p], reads[2p+1]   the two mates of pair p (base codes), regs[2p], regs[2p+1] their region vectors as
 *                            phase 1 left them (mem_alnreg_v, layout-compatible); rescued regions are inserted into
 *                            the MATE's vector exactly as the reference does (kv_push growth, score-sorted insert,
 *                            then mem_sort_and_dedup)
 *   pes[4]                   mem_pestat_t per orientation (bwamem.h:66-70), opt fields of mem_opt_t in `o`
 *   dedup                    the caller's mem_sort_and_dedup(n, a, opt->mask_level_redun) (bwamem.c:395); it is host
 *                            post-processing outside this path, so the reference's own function is passed in
 *   n_sw[p] (nullable)       the sum of mem_matesw's return values for pair p
 * Each mem_matesw invocation tests its four orientations against the current state of the mate's vector, so the
 * invocations of one pair are sequential; the driver runs them as rounds -- per unfinished pair its next few
 * invocations (planned ahead against the current state, re-checked when folded), their ksw_align2 calls as one GPU
 * batch over all pairs.  The outcome is exactly the reference's; a call planned ahead may go unused.
 * With the reference resident (bmh_ctx_set_pac, same pac pointer) the windows are BMH_F_TPAC tasks and the
 * reverse-complemented mate is BMH_F_QREV|BMH_F_QCOMP: the pool holds every read once and nothing else.
 * Its ksw_align2 calls obey bmh_sw_batch's range: a mate with l_seq*max(mat) >= 32000 needs bmh_ctx_set_wide_sw on the context
 * (word mode, the long-query kernel), and the call fails with BMH_E_RANGE otherwise. */
typedef struct bmh_pestat { /* mem_pestat_t, bwamem.h:66-70 */
	int32_t low, high;
	int32_t failed;
	double avg, std;
} bmh_pestat_t;
typedef struct bmh_matesw_opt { /* the mem_opt_t fields mem_sam_pe / mem_matesw read beside the scoring (bwamem.h:21-48) */
	int32_t pen_unpaired, max_matesw, min_seed_len, rsv;
} bmh_matesw_opt_t;
typedef int (*bmh_dedup_fn)(void *user, int n, bmh_alnreg_t *a);
int bmh_matesw_batch(bmh_ctx_t *ctx, int64_t l_pac, const uint8_t *pac, int n_pairs, const bmh_read_t *reads,
                     bmh_alnreg_v *regs, const bmh_pestat_t pes[4], const bmh_matesw_opt_t *o, bmh_dedup_fn dedup,
                     void *dedup_user, int *n_sw);
/* The same driver as kernels (csrc/matesw.hip): the planning, the folding and mem_sort_and_dedup run on the device, one lane per
 * pair that needs rescue, over the rules the host driver uses (one text, host/matesw_core.h) -- so both make the same ksw_align2
 * calls in the same number of rounds.  Inside a call only 16-byte status words cross PCIe between the launches, and no host
 * callback remains: mem_sort_and_dedup is bmh_sort_and_dedup's text at mask_level_redun.
 *   result       regs and n_sw exactly as bmh_matesw_batch leaves them when its dedup is bmh_sort_and_dedup(n, a, mask_level_redun).
 *                Only the vectors of pairs that need rescue are written: regs[k].a is realloc'd where m is too small, n is updated;
 *                every other vector is not touched.  n_sw (nullable) is 0 for the other pairs.
 *   BMH_E_ARG    a NULL ctx, reads, regs, pes or o; n_pairs < 0; l_pac <= 0; no parameters set; no 2-bit reference of this l_pac
 *                resident on the device (bmh_ctx_set_pac); a vector with n > 0 and a == NULL
 *   BMH_E_RANGE  a pair that needs rescue with a read outside 1..65535 bases, or whose ksw_align2 calls bmh_sw_batch would refuse
 *                (they depend on the read's length and the parameters only): byte mode under gap penalties that wrap, and
 *                l_seq*max(mat) >= 32000 without bmh_ctx_set_wide_sw.  Checked on the host before anything is uploaded.
 *   BMH_OK       without a launch for n_pairs == 0 and for a batch in which no pair needs rescue
 * On any error the caller's vectors are as they were: they are written after the last kernel has finished, all or none.
 * bmh_driver_stats reports the host driver's numbers with the host driver's meanings: rounds that launched Smith-Waterman,
 * ksw_align2 tasks, and as pool_bytes the reads of the pairs that need rescue plus 16 bytes of padding (0 if no round launched). */
int bmh_matesw_device(bmh_ctx_t *ctx, int64_t l_pac, int n_pairs, const bmh_read_t *reads, bmh_alnreg_v *regs,
                      const bmh_pestat_t pes[4], const bmh_matesw_opt_t *o, float mask_level_redun, int *n_sw);
/* The same rescue over a flat region table that stays on the device (csrc/matesw.hip): read k's regions are reg[roff[k] .. roff[k+1]),
 * reads 2p and 2p+1 are mates.  What bmh_matesw_device does on the host around its rounds runs as kernels here: the pre-filter and the
 * refusals (mt_filter_kernel, one lane per pair, over host/matesw_table_core.h), the sizing (scans), the packing of the arena slices,
 * the candidate hits and the pair records (mt_pack_kernel, mt_slices_kernel; the reads are one pool on the device and are not copied),
 * and the merge of the rescued vectors with the untouched ones into a second table (mt_count_kernel, mt_place_kernel, mt_copy_kernel).
 * The rounds between are bmh_matesw_device's own.  The call uploads every read as one pool and the table, runs that, and downloads
 * the result; between the upload and the download the host reads one 64-byte plan record, 16 status bytes per round as
 * bmh_matesw_device does, and one 16-byte total.
 *   result       roff_out[0 .. 2*n_pairs], *reg_out (malloc'd, the caller frees it; one record at least) and n_sw (nullable) are the
 *                flattening of what bmh_matesw_device leaves in the vectors and in n_sw for the same reads, regions, pes, o and
 *                mask_level_redun, byte for byte
 *   BMH_E_ARG    before anything is uploaded: a NULL ctx, roff, pes, o, roff_out or reg_out; NULL reads with n_pairs > 0; n_pairs < 0;
 *                l_pac <= 0; no parameters set; no 2-bit reference of this l_pac resident on the device (bmh_ctx_set_pac); roff[0] != 0
 *                or roff not non-decreasing; a vector of more than 2^31 - 1 regions; a NULL reg with roff[2*n_pairs] > 0; a read with
 *                l_seq < 0, or with l_seq > 0 and a NULL seq (every read goes up, also those of pairs that need no rescue)
 *   BMH_E_RANGE  from the plan record, before any round runs: bmh_matesw_device's conditions with its texts and the read's index -- a
 *                pair that needs rescue with a read outside 1..65535 bases, byte mode under gap penalties that wrap, l_seq*max(mat) >=
 *                32000 without bmh_ctx_set_wide_sw.  The reads of pairs that need no rescue do not count.
 *   BMH_OK       without a round for n_pairs == 0 and for a batch in which no pair needs rescue: the output is a copy of the input,
 *                made on the device
 * All or nothing: on any error roff_out, *reg_out and n_sw are untouched, the Smith-Waterman kernels' error flag is clean and the
 * context stays usable.  bmh_driver_stats reports bmh_matesw_device's rounds and ext_tasks; pool_bytes is the uploaded pool -- every
 * read plus 16 bytes of padding -- when a round launched Smith-Waterman, else 0.  Nothing routes to this call by default. */
int bmh_matesw_table_device(bmh_ctx_t *ctx, int64_t l_pac, int n_pairs, const bmh_read_t *reads,
                            const uint64_t *roff, const bmh_alnreg_t *reg,
                            const bmh_pestat_t pes[4], const bmh_matesw_opt_t *o, float mask_level_redun,
                            uint64_t *roff_out, bmh_alnreg_t **reg_out, int *n_sw);
/* Of the last bmh_matesw_table_device call on this context that got past its argument checks; all -1 before the first.
 *   regions_in, regions_out  of the two tables
 *   arena_records, hits      what the filter sized for the pairs that need rescue: the slices' records, the candidate hits
 *   mid_bytes                bytes that crossed PCIe between the upload and the final download: 64 + 16 per status read-back + 16
 *   pairs, active            of the batch; that need rescue
 *   waits                    host waits between the upload and the final download: 2 + the status read-backs
 *   filter_ms, pack_ms, merge_ms   the three kernel groups' milliseconds with bmh_set_kernel_timing on, else -1 */
typedef struct bmh_matesw_table_stats {
	int64_t regions_in, regions_out, arena_records, hits, mid_bytes;
	int32_t pairs, active, waits;
	float filter_ms, pack_ms, merge_ms;
} bmh_matesw_table_stats_t; /* 64 bytes */
int bmh_last_matesw_table_stats(const bmh_ctx_t *ctx, bmh_matesw_table_stats_t *st);

/* ------------------------------------------------------------------------------------------------------------
 * Region post-processing and SAM text: everything mem_process_seqs does with a read's region
 * vector after the extensions -- host code (plain C, batched per chunk slice), with the one DP it contains
 * (ksw_global2 under mem_reg2aln / bwa_fix_xref2) run as GPU batches.
 * Replaces: mem_sort_and_dedup (reference bwamem.c:395-436), mem_mark_primary_se (:445-475), mem_approx_mapq_se
 *           (:1023-1047), mem_reg2aln (:1164-1236) over bwa_fix_xref2 (bwa.c:179-222), mem_aln2sam (:904-1017),
 *           mem_reg2sam_se (:1049-1083); mem_pestat (bwamem_pair.c:46-107), mem_pair (:177-238), mem_sam_pe (:240-332)
 *           -- i.e. worker2 of mem_process_seqs (bwamem.c:1281-1295).
 * Ties in the reference's unstable sorts decide which duplicate survives and which hit is primary; the library sorts
 * with the same comparison/exchange sequence (host/sort_exact.h), so the output order is the reference's. */
typedef struct bmh_sam_opt { /* the mem_opt_t fields phase 2 reads (bwamem.h:21-48); scoring as in bmh_params_t */
	int32_t a, b, o_del, e_del, o_ins, e_ins, pen_unpaired, w;
	int32_t T, flag, min_seed_len, max_ins, mapQ_coef_fac, max_matesw;
	float mask_level, mask_level_redun, mapQ_coef_len;
	int8_t mat[25];
	int8_t pad_[3];
} bmh_sam_opt_t;
#define BMH_MEM_F_PE 0x2        /* bwamem.h:14-20 */
#define BMH_MEM_F_NOPAIRING 0x4
#define BMH_MEM_F_ALL 0x8
#define BMH_MEM_F_NO_MULTI 0x10
#define BMH_MEM_F_NO_RESCUE 0x20
#define BMH_MEM_F_NO_EXACT 0x40

typedef struct bmh_refann { /* == bntann1_t, bntseq.h:39-45: one reference sequence */
	int64_t offset;
	int32_t len, n_ambs;
	uint32_t gi;
	char *name, *anno;
} bmh_refann_t;
typedef struct bmh_refidx { /* == the head of bntseq_t, bntseq.h:53-61 (a bntseq_t* may be passed) */
	int64_t l_pac;
	int32_t n_seqs;
	uint32_t seed;
	bmh_refann_t *anns;
} bmh_refidx_t;
typedef struct bmh_seq { /* == bseq1_t, bwa.h:19-22; seq holds base codes (after bwamem.c:1093-1094); sam is malloc'd */
	int32_t l_seq;
	char *name, *comment, *seq, *qual, *sam;
} bmh_seq_t;

int bmh_sort_and_dedup(int n, bmh_alnreg_t *a, float mask_level_redun);                       /* mem_sort_and_dedup; on the device: bmh_sort_dedup_batch */
void bmh_mark_primary_se(const bmh_sam_opt_t *o, int n, bmh_alnreg_t *a, int64_t id);         /* mem_mark_primary_se */
int bmh_approx_mapq_se(const bmh_sam_opt_t *o, const bmh_alnreg_t *a);                         /* mem_approx_mapq_se  */
/* (the three above and bmh_pair below as one batch call, on the host or the device: bmh_decide_batch / bmh_decide_device) */
/* mem_pestat; with verbose >= 3 it prints the reference's "[M::mem_pestat] ..." lines to stderr.  Out of host memory (where the
 * reference aborts) it prints a "[bwamem_hip]" message and marks all four orientations as failed. */
void bmh_pestat(const bmh_sam_opt_t *o, int64_t l_pac, int n, const bmh_alnreg_v *regs, bmh_pestat_t pes[4], int verbose);
/* mem_pestat in its two halves; bmh_pestat equals the first followed by the second, field for field and in its stderr text.
 * bmh_pestat_candidates: the pair walk (bwamem_pair.c:56-72, the text of host/pestat_core.h) over n reads, reads 2p and 2p+1 being
 * mates (an odd n ignores the last read); cand[p], n/2 words, is 0 where pair p is no candidate and orientation << 30 | insert size
 * where it is (1 <= insert size <= o->max_ins, so a candidate's word is never 0).  On the device: bmh_pestat_device, and
 * bmh_ctx_set_pestat_collect behind the chains-to-regions calls.
 * bmh_pestat_from_candidates: the statistics (:73-106) from such words.  A word whose insert size is 0 or above o->max_ins is
 * refused with BMH_E_ARG and pes is left untouched.
 * Both: BMH_E_ARG for a NULL argument or a negative size, BMH_E_RANGE for o->max_ins >= 2^30 (the word cannot hold it; bmh_pestat
 * serves such a value). */
int bmh_pestat_candidates(const bmh_sam_opt_t *o, int64_t l_pac, int n, const bmh_alnreg_v *regs, uint32_t *cand);
int bmh_pestat_from_candidates(const bmh_sam_opt_t *o, int64_t n_pairs, const uint32_t *cand, bmh_pestat_t pes[4], int verbose);
/* mem_pair (bwamem_pair.c:177-238): the best-scoring properly oriented pair of hits of the two ends; returns its score
 * (0 = none), *sub / *n_sub the runner-up and how many lie within one event of it, z[] the chosen hit of each end */
int bmh_pair(const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t pes[4], const bmh_alnreg_v a[2], uint64_t id, int *sub,
             int *n_sub, int z[2]);
/* Phase 2 for reads [0,n) of a chunk slice: marks primaries, pairs (when o->flag has BMH_MEM_F_PE: n is even, reads 2p
 * and 2p+1 are mates, pes = the four insert-size models, mate rescue already done or off), runs the global alignments
 * of exactly the regions that get printed as GPU batches, and writes seqs[i].sam (malloc'd, the caller frees it as
 * fastmap.c:201 does).  id0 = n_processed + index of read 0 (the reference's per-read id, bwamem.c:1287,1291).
 * rg_id: the reference's bwa_rg_id ("" = none).  regs[i].a is left sorted/marked as the reference leaves it -- except with
 * bmh_ctx_set_phase2_text_device on (below), where all three passes are one device session and the vectors stay exactly as they came.
 * The decisions (everything before the global alignments) are bmh_decide_batch's, or with bmh_ctx_set_decide_device on
 * bmh_decide_device's: the same text either way (below).  With bmh_ctx_set_phase2_device on, decisions and alignments are one device
 * session, bmh_phase2_device's: the same text again.  The text itself (pass C) is bmh_sam_text_batch's, or with
 * bmh_ctx_set_samtext_device on bmh_sam_text_device's: the same bytes (below).  All or nothing: on an error no seqs[i].sam is set. */
int bmh_sam_batch(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes,
                  int64_t id0, int n, bmh_seq_t *seqs, bmh_alnreg_v *regs, const char *rg_id);

/* ---- Pass A of bmh_sam_batch on its own: what gets printed, and with which mapQ (mem_mark_primary_se, mem_pair, the tail of
 * mem_sam_pe, the selection of mem_reg2sam_se, mem_approx_mapq_se of every region), for reads [0,n) of a chunk slice.  One text,
 * host/postproc_core.h, compiled by gcc for the host call and by hipcc for the device call: both give the same bytes.
 *   regs      regs[i] is read i's vector as phase 1 or mate rescue left it; on return sorted and marked as the reference leaves
 *             it, with sub / secondary = -2 of a winning pair's hits
 *   roff      n + 1 entries: roff[i] = regions before read i
 *   pd        with BMH_MEM_F_PE in o->flag (n even, pes the four insert-size models): pd[p] is the verdict on reads 2p, 2p+1, whose
 *             pair id is (id0>>1)+p and read ids id<<1|r.  score, sub, n_sub are mem_pair's (0 where it was not asked); q_pe is 0
 *             where it is not computed; z[] and q_se[] mean something for paired != 0.  NULL (like pes) for single-end reads.
 *   reg_mapq  reg_mapq[roff[i]+j] = mem_approx_mapq_se of region j of read i in its final state, for every region
 *   n_want, want_k   want_k[roff[i] .. roff[i]+n_want[i]) are the indices of read i's regions that get printed, in the order
 *             mem_reg2sam_se visits them; for a paired decision that is z[r] alone (or nothing, for a region off the reference)
 * BMH_E_ARG: a NULL argument with n > 0, n < 0, odd n or no pes with PE, a vector with n > 0 and no array, roff that does not
 * match the vectors.  n == 0: BMH_OK. */
typedef struct bmh_pairdec { int32_t paired, z[2], q_se[2], extra_flag, score, sub, n_sub, q_pe, rsv[2]; } bmh_pairdec_t; /* 48 B */
int bmh_decide_batch(const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t *pes, int64_t id0, int n,
                     bmh_alnreg_v *regs, const int64_t *roff, bmh_pairdec_t *pd, int32_t *reg_mapq,
                     int32_t *n_want, int32_t *want_k);
/* The same as a kernel (csrc/decide.hip), one lane per read or pair: one upload, decide_kernel, one download.  log and erfc do
 * not run on the device: the host tabulates log(k) for k = 0..K (resident per context, grown on demand) and, per call, mem_pair's
 * insert-size term for every distance of every orientation that has not failed.  Needs neither parameters nor a resident
 * reference.  Refused on the host before anything is uploaded:
 *   BMH_E_ARG    a NULL ctx, and what bmh_decide_batch refuses
 *   BMH_E_RANGE  a table would pass 1 << 20 entries: the log table must reach max(qe-qb, re-rb) (mapQ_coef_len > 0) or seedcov
 *                (otherwise) of every region, a vector's n + 1 (plus the sub_n it came with), a pair's (n0 + n1)^2 + 1; a negative
 *                index is refused too; the pair table needs the sum of high - low + 1 over the orientations that have not failed
 *                (not with BMH_MEM_F_NOPAIRING, which never pairs)
 *   BMH_OK       without a launch for n == 0
 * The caller's vectors and outputs are written only after the kernel has finished: all or nothing. */
int bmh_decide_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t *pes, int64_t id0, int n,
                      bmh_alnreg_v *regs, const int64_t *roff, bmh_pairdec_t *pd, int32_t *reg_mapq,
                      int32_t *n_want, int32_t *want_k);
/* Per context, off by default.  While on, bmh_sam_batch takes its pass A from bmh_decide_device; a slice that call answers
 * BMH_E_RANGE for goes through bmh_decide_batch instead.  The text is the same either way. */
int bmh_ctx_set_decide_device(bmh_ctx_t *ctx, int on);
/* Of the last bmh_decide_device call on this context, direct or from bmh_sam_batch with the switch on: the reads (single-end) or
 * pairs the kernel decided, 1 if the call answered BMH_E_RANGE (bmh_sam_batch then fell back to the host) else 0, and the kernel's
 * milliseconds with bmh_set_kernel_timing on (else -1).  -1, 0, -1 before the first such call.  With the switch on bmh_sam_batch
 * sets them to 0, 0, -1 at its entry, so that after it they are that call's even where it returned before its decisions (n == 0, a
 * refused argument).  Any pointer may be NULL. */
int bmh_last_decide_stats(const bmh_ctx_t *ctx, int64_t *units, int64_t *fallbacks, float *kernel_ms);

/* ---- Pass B of bmh_sam_batch on its own: the global alignments of exactly the regions pass A listed (mem_reg2aln's first half,
 * bwamem.c:1164-1201, over bwa_fix_xref2, bwa.c:179-222), for reads [0,n) of a chunk slice.  regs, roff, n_want, want_k as
 * bmh_decide_batch leaves them; w = opt->w (the band of bwa_fix_xref2's single alignment); the context's parameters give the scoring.
 * Wanted region number j = (wanted regions of the reads before read i) + q stands for want_k[roff[i] + q]; results[j] is:
 *   qb, qe, rb, re   the region's ends after bwa_fix_xref2
 *   score, n_cigar, NM, tries, md_len   as bmh_cigar_res_t
 *   cigar_off, md_off   into cigar_pool / md_pool, packed in want order (the MD strings NUL-terminated); BMH_E_CIGAR_CAP when a
 *                    pool is too small -- the sums of qe-qb + re-rb + 2 words and of 3*(qe-qb + re-rb) + 16 bytes always suffice
 *   band[3]          the band of each try as planned: -1 where there is no try, band[0] == -1 for the no-gap case (bwa.c:108-114)
 *   flags            BMH_WANTED_MOVED: the region hung over an end of its reference sequence and bwa_fix_xref2 moved an end;
 *                    BMH_WANTED_HOST: an alignment of the region outgrows the device's slots (a CIGAR of more than 24 operations,
 *                    its own or that of bwa_fix_xref2's alignment, or an MD string of more than 128 bytes), so wherever the
 *                    region records run it is redone with host copies; the BMH_REGION_* bits are cleared by then and never set here
 * What the planning sees is checked per wanted region: 0 <= want_k < regs[i].n, 0 <= qb < qe <= l_seq, 0 <= rb < re <= 2*l_pac and no
 * strand bridge (BMH_E_ARG, as for a region of which bwa_fix_xref2 leaves nothing), qe-qb and re-rb at most 65535 (BMH_E_RANGE).
 * The caller's memory is written only after everything has succeeded.  n == 0 or no wanted region: BMH_OK, nothing runs. */
#define BMH_WANTED_MOVED 4u
#define BMH_WANTED_HOST 8u
typedef struct bmh_wanted_res { /* 72 bytes */
	int64_t rb, re;
	int32_t qb, qe;
	int32_t score, n_cigar, NM, tries;
	uint32_t cigar_off, md_off, md_len, flags;
	int32_t band[3];
	int32_t rsv_;
} bmh_wanted_res_t;
int bmh_wanted_cigar_batch(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads,
                           const bmh_alnreg_v *regs, const int64_t *roff, const int32_t *n_want, const int32_t *want_k,
                           bmh_wanted_res_t *results, uint32_t *cigar_pool, size_t cigar_words, char *md_pool, size_t md_bytes);
/* The same with the planning as kernels (csrc/wanted.hip over host/regplan_core.h, the text the host form uses): one upload of
 * offsets, regions, the want list and the reads, the planning kernels and the region kernels of bmh_region_cigar_batch behind it,
 * one download.  The host reads one status record between launches, at most twice.  The same bytes out as the host form.  Needs the
 * 2-bit reference (bmh_ctx_set_pac with bns->l_pac) and the sequence table (bmh_ctx_set_refidx) resident: BMH_E_ARG otherwise.  The few
 * regions flagged BMH_WANTED_HOST are redone on the host; the rest of the call is unaffected. */
int bmh_wanted_cigar_device(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads,
                            const bmh_alnreg_v *regs, const int64_t *roff, const int32_t *n_want, const int32_t *want_k,
                            bmh_wanted_res_t *results, uint32_t *cigar_pool, size_t cigar_words, char *md_pool, size_t md_bytes);
/* Copies (offset, len) of every reference sequence of bns to the device, where it stays like the 2-bit reference; NULL drops it. */
int bmh_ctx_set_refidx(bmh_ctx_t *ctx, const bmh_refidx_t *bns);
/* Per context, off by default.  While on, bmh_sam_batch takes its pass B from the device form (BMH_E_ARG without the two resident
 * tables).  The text is the same either way. */
int bmh_ctx_set_wanted_device(bmh_ctx_t *ctx, int on);
/* Of the last bmh_wanted_cigar_device call on this context, direct or from bmh_sam_batch with the switch on: wanted regions, regions
 * bwa_fix_xref2 moved, regions redone on the host, and the planning kernels' milliseconds with bmh_set_kernel_timing on (else -1).
 * -1, -1, -1, -1 before the first such call.  Any pointer may be NULL.  (With bmh_ctx_set_decide_device also on, pass A and pass B
 * are still two device sessions: the want list is downloaded and uploaded again between them.  The one session without that hop is
 * bmh_phase2_device below, behind a switch of its own.) */
int bmh_last_wanted_stats(const bmh_ctx_t *ctx, int64_t *wanted, int64_t *fixed, int64_t *redone, float *kernel_ms);

/* ---- Pass A and pass B as one device session: bmh_decide_device's kernel and bmh_wanted_cigar_device's kernels on one upload, the
 * want list and the sorted regions read where decide_kernel left them.  The regions go up once, the want list never goes up, and the
 * host waits at most three times (two status records, the end).  Arguments as in the two calls, w = o->w.  Every output is byte for
 * byte what bmh_decide_batch followed by bmh_wanted_cigar_batch(..., w = o->w, ...) leaves in the same arguments; entries of want_k
 * past a read's n_want stay the caller's.  *n_wanted = the wanted regions, the records written.
 *   capacities   the caller does not know the want list: results_cap = roff[n] always suffices, and for the pools the sums of
 *                qe-qb + re-rb + 2 words and of 3*(qe-qb + re-rb) + 16 bytes over ALL regions of the slice; BMH_E_CIGAR_CAP when
 *                one of the three is too small
 *   BMH_E_ARG    before any upload: what bmh_decide_batch refuses, what bmh_wanted_cigar_batch refuses of reads, vectors and
 *                offsets, a NULL n_wanted, no parameters, no resident 2-bit reference or sequence table; from the kernels: a wanted
 *                region as bmh_wanted_cigar_device refuses it
 *   BMH_E_RANGE  before any upload: exactly what bmh_decide_device refuses (a table past 1 << 20 entries); from the kernels: a wanted
 *                window past 65535
 *   BMH_OK       for n == 0 with *n_wanted = 0, nothing runs
 * All or nothing: the caller's vectors and every output are written only after everything has succeeded, the host's redo of the
 * BMH_WANTED_HOST regions included; on any error they are untouched (the vectors not even sorted). */
int bmh_phase2_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes,
                      int64_t id0, int n, const bmh_read_t *reads, bmh_alnreg_v *regs, const int64_t *roff, bmh_pairdec_t *pd,
                      int32_t *reg_mapq, int32_t *n_want, int32_t *want_k, bmh_wanted_res_t *results, int64_t results_cap,
                      int64_t *n_wanted, uint32_t *cigar_pool, size_t cigar_words, char *md_pool, size_t md_bytes);
/* Per context, off by default.  While on, bmh_sam_batch takes pass A and pass B from bmh_phase2_device (BMH_E_ARG without the two
 * resident tables); a slice that call refuses with BMH_E_RANGE before its upload goes the way the other two switches say.  The text
 * is the same either way. */
int bmh_ctx_set_phase2_device(bmh_ctx_t *ctx, int on);
/* Of the last bmh_phase2_device call on this context, direct or from bmh_sam_batch with the switch on; all -1 before the first.
 *   units, wanted, fixed, redone   reads or pairs decided, wanted regions, regions bwa_fix_xref2 moved, regions redone on the host
 *   fallbacks, sessions            0 and 1 for a fused run; 1 and 2 where bmh_sam_batch fell back after BMH_E_RANGE; 0 and 0 where
 *                                  nothing ran (n == 0)
 *   h2d_bytes, d2h_bytes, waits    of the fused session itself (the host's redo of a few regions is not counted)
 *   decide_ms, wanted_ms           the kernels' milliseconds with bmh_set_kernel_timing on, else -1 */
typedef struct bmh_phase2_stats {
	int64_t units, wanted, fixed, redone, fallbacks;
	int64_t h2d_bytes, d2h_bytes;
	int32_t waits, sessions;
	float decide_ms, wanted_ms;
} bmh_phase2_stats_t;
int bmh_last_phase2_stats(const bmh_ctx_t *ctx, bmh_phase2_stats_t *st);

/* ---- Pass C of bmh_sam_batch on its own: coordinates, clipping, flags and SAM text (mem_reg2aln's second half, bwamem.c:1203-1235;
 * mem_reg2sam_se and mem_aln2sam, bwamem.c:904-1083; the mate records of mem_sam_pe, bwamem_pair.c:311-324) of exactly the regions pass
 * A listed, from the alignments pass B made, for reads [0,n) of a chunk slice.  One text, host/samtext_core.h, compiled by gcc for the
 * host call and by hipcc for the device call: both give the same bytes.  Needs no context.
 *   o, bns, pes, n, seqs, regs, roff   as bmh_sam_batch and bmh_decide_batch have them, the vectors as pass A left them; of seqs the
 *             name, comment, seq (base codes), qual and l_seq are read, sam is not touched
 *   pd, reg_mapq, n_want, want_k       pass A's outputs (pd NULL for single-end reads)
 *   results, cigar_pool, md_pool       pass B's outputs: the records in want order and the pools their cigar_off / md_off address
 *   rg_id     the reference's bwa_rg_id ("" or NULL = none)
 *   text      *text = one malloc'd pool, which the caller frees
 *   text_off  n + 1 entries: read i's SAM lines are (*text)[text_off[i] .. text_off[i+1]), each line ending in '\n'; no NUL in the pool
 * BMH_E_ARG: what bmh_sam_batch refuses of these (a NULL o, bns, or with n > 0 seqs or regs; n < 0; odd n or no pes with PE; a vector with
 * n > 0 and no array), a NULL text, text_off or with n > 0 pass A output, roff that does not match the vectors, n_want or want_k
 * outside a vector, a read without a name or with l_seq > 0 and no seq, records or pools missing where a region is wanted, a record
 * outside its read or the reference, mates whose names differ (with bmh_sam_batch's message).  n == 0: BMH_OK, an empty pool,
 * text_off[0] = 0.  All or nothing: on any error *text and text_off are untouched. */
int bmh_sam_text_batch(const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs,
                       const bmh_alnreg_v *regs, const int64_t *roff, const bmh_pairdec_t *pd, const int32_t *reg_mapq,
                       const int32_t *n_want, const int32_t *want_k, const bmh_wanted_res_t *results, const uint32_t *cigar_pool,
                       const char *md_pool, const char *rg_id, char **text, int64_t *text_off);
/* The same as kernels (csrc/samtext.hip), the same bytes out.  One upload: offsets (roff, the want list's first[], the read pool's
 * offsets: 3 x 8 (n + 1) bytes), a 128-byte header, rg_id, n_want, want_k and reg_mapq (4 bytes per read / region), pd, the regions, the
 * records, the CIGAR words and MD bytes the records reach, and a per-read byte pool packed by the host: per read 16 bytes of lengths,
 * then name, base codes, qualities and comment, rounded up to 8 bytes.  samtext_size_kernel (one lane per read or pair: the records,
 * the per-unit rule, the composer counting), an exclusive 64-bit scan, samtext_emit_kernel (one lane per read: the composer writing into
 * the read's slice).  The host reads one 16-byte status between scan and emit (total and error flag) and sizes the text buffer from
 * it: two waits per call.  One download: text_off and the text.
 * Needs the sequence table (bmh_ctx_set_refidx) and the sequence names (bmh_ctx_set_refnames) resident, neither parameters nor the
 * 2-bit reference.  BMH_E_ARG: a NULL ctx, a missing table or one of another reference, and what bmh_sam_text_batch refuses.  A write
 * past a read's slice or a slice outside the buffer is not made: it raises the context's error flag and the call fails, nothing
 * written. */
int bmh_sam_text_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs,
                        const bmh_alnreg_v *regs, const int64_t *roff, const bmh_pairdec_t *pd, const int32_t *reg_mapq,
                        const int32_t *n_want, const int32_t *want_k, const bmh_wanted_res_t *results, const uint32_t *cigar_pool,
                        const char *md_pool, const char *rg_id, char **text, int64_t *text_off);
/* Copies the name of every reference sequence of bns to the device (one byte pool plus offsets), where it stays like the sequence
 * table; NULL drops it. */
int bmh_ctx_set_refnames(bmh_ctx_t *ctx, const bmh_refidx_t *bns);
/* Per context, off by default, independent of every other switch.  While on, bmh_sam_batch takes its pass C from bmh_sam_text_device
 * (BMH_E_ARG without the two resident tables).  The text is the same either way. */
int bmh_ctx_set_samtext_device(bmh_ctx_t *ctx, int on);
/* Of the last bmh_sam_text_device call on this context, direct or from bmh_sam_batch with the switch on; all -1 before the first.  With
 * the switch on bmh_sam_batch sets them to 0 (the milliseconds to -1) at its entry.
 *   reads, lines, text_bytes       of the slice
 *   h2d_bytes, d2h_bytes, waits    of the session: the upload above; the status, text_off and the text; 2
 *   size_ms, emit_ms               the two kernels' milliseconds with bmh_set_kernel_timing on, else -1 */
typedef struct bmh_samtext_stats {
	int64_t reads, lines, text_bytes;
	int64_t h2d_bytes, d2h_bytes;
	int32_t waits, rsv_;
	float size_ms, emit_ms;
} bmh_samtext_stats_t; /* 56 bytes */
int bmh_last_samtext_stats(const bmh_ctx_t *ctx, bmh_samtext_stats_t *st);

/* ---- Passes A, B and C as one device session: the slice's regions and reads go up once, and only SAM text comes down.
 * *text / text_off[0..n] are byte for byte what bmh_decide_batch, then bmh_wanted_cigar_batch(..., w = o->w, ...), then
 * bmh_sam_text_batch give for the same arguments: the concatenation of the seqs[i].sam strings bmh_sam_batch writes.  regs is read
 * only: the caller's vectors are left exactly as they came, not sorted and not marked, because nothing of pass A comes down.
 *   one upload   bmh_phase2_device's block as it is (offsets, opt + pes, read offsets, parameters, pair table, regions), and pass C's
 *                inputs the device does not yet have: the 144-byte header, rg_id, the per-read pool's offsets and the per-read pool of
 *                bmh_sam_text_device (name, base codes, qualities, comment).  The bases go up once, inside that pool;
 *                reads_gather_kernel builds pass B's contiguous reads pool from it on the device.
 *   the passes   A and B exactly as in bmh_phase2_device, through wanted_result_kernel (the host reads one 64-byte status record
 *                twice).  phase2_text_bind_kernel then turns every record's slot number into the slot's address in the main round's
 *                CIGAR and MD slots, where pass C reads them -- nothing is packed -- and lists the regions flagged BMH_WANTED_HOST.
 *                samtext_size_kernel and the scan follow with no wait between; the host reads one 32-byte status (text total, error
 *                word, host-region count, lines), launches samtext_emit_kernel and downloads text_off and the text: four waits.
 *   the redo     where the host-region count is not zero only the list comes down (112 bytes per region); the host redoes those
 *                regions as bmh_wanted_cigar_device does, uploads their records, CIGAR words and MD bytes into an overflow area behind
 *                the slots, patches the records on the device and runs size and scan again: six waits, the rest of the slice unaffected
 *                (seven where the overflow area outgrew the block, which then moves with its contents kept).
 * Needs the context's parameters, the resident 2-bit reference, the sequence table (bmh_ctx_set_refidx) and the sequence names
 * (bmh_ctx_set_refnames): BMH_E_ARG without any of them.
 *   BMH_E_ARG    before any upload: a NULL ctx, text or text_off, and what bmh_phase2_device and bmh_sam_text_batch refuse of o, bns,
 *                pac, pes, n, seqs and regs (a read without a name, mates whose names differ, ...); from the kernels: what
 *                bmh_phase2_device's and bmh_sam_text_device's raise
 *   BMH_E_RANGE  before any upload: what bmh_decide_device refuses (a table past 1 << 20 entries), and a slice whose slot addresses
 *                (regions x 24 words, regions x 128 bytes) do not fit in 32 bits; from the kernels: a wanted window past 65535;
 *                behind the redo: an overflow area whose addresses do not fit in 32 bits
 *   BMH_OK       for n == 0 with an empty pool and text_off[0] = 0, nothing runs
 * All or nothing: on any error *text and text_off are untouched. */
int bmh_phase2_text_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes,
                           int64_t id0, int n, const bmh_seq_t *seqs, const bmh_alnreg_v *regs, const char *rg_id, char **text,
                           int64_t *text_off);
/* Per context, off by default.  While on, bmh_sam_batch takes all three passes from bmh_phase2_text_device (BMH_E_ARG without the
 * resident tables) and leaves regs[i].a exactly as it came.  A slice that call refuses with BMH_E_RANGE before its upload goes the way
 * the other switches say, and is counted as a fall-back.  The text is the same either way. */
int bmh_ctx_set_phase2_text_device(bmh_ctx_t *ctx, int on);
/* Of the last bmh_phase2_text_device call on this context, direct or from bmh_sam_batch with the switch on; all -1 before the first.
 * With the switch on bmh_sam_batch sets the counts to 0 (the milliseconds to -1) at its entry.
 *   units, wanted, fixed, redone   reads or pairs decided, wanted regions, regions bwa_fix_xref2 moved, regions redone on the host
 *   reads, lines, text_bytes       of the slice
 *   h2d_bytes, d2h_bytes, waits    of the fused session only (not of the host's redo): waits is 4, or 6 with redone regions, 7 where
 *                                  the overflow area outgrew the block (2 for a slice without a single region, where pass B has
 *                                  nothing to run)
 *   fallbacks, sessions            0 and 1 for a fused run; 1 and 0 where the call refused the slice before its upload (BMH_E_RANGE)
 *   decide_ms, wanted_ms, gather_ms, size_ms, emit_ms   the kernels' milliseconds with bmh_set_kernel_timing on, else -1 */
typedef struct bmh_phase2_text_stats {
	int64_t units, wanted, fixed, redone;
	int64_t reads, lines, text_bytes;
	int64_t h2d_bytes, d2h_bytes, fallbacks;
	int32_t waits, sessions;
	float decide_ms, wanted_ms, gather_ms, size_ms, emit_ms;
	int32_t rsv_;
} bmh_phase2_text_stats_t; /* 112 bytes */
int bmh_last_phase2_text_stats(const bmh_ctx_t *ctx, bmh_phase2_text_stats_t *st);

/* ------------------------------------------------------------------------------------------------------------
 * FM-index queries of the seeding stage (first slice): super-maximal exact matches and suffix-
 * array look-ups on the device, over the reference's own index arrays made resident in HBM.
 * Replaces: bwt_smem1 (reference bwa-0.7.8/bwt.c:288-347; over bwt_extend :261-274 and bwt_2occ4 :191-219), called in the
 *           order smem_next2 calls it for one read (bwamem.c:118-162 as driven by mem_insert_seed, bwamem.c:208-214), and
 *           bwt_sa (bwt.c:85-95; over bwt_invPsi :52-58 and bwt_occ :107-129).
 * Chaining (mem_insert_seed's B-tree, mem_chain_flt) is bmh_chain_reads on the host or bmh_chain_batch /
 * bmh_seed_chain_batch on the device (below); INTEGRATION.md shows how the reference's mem_chain consumes these results
 * unchanged. */
typedef struct bmh_bwt { /* the fields of bwt_t the queries read (bwt.h:45-57); arrays are borrowed, never modified */
	uint64_t primary, L2[5], seq_len, bwt_size; /* bwt_size in 32-bit words */
	const uint32_t *bwt;                        /* BWT with the interleaved occurrence counts (bwt.h:63-64 layout) */
	int32_t sa_intv;
	uint64_t n_sa;
	const uint64_t *sa;
} bmh_bwt_t;
typedef struct bmh_smem_intv { uint64_t x[3], info; } bmh_smem_intv_t; /* == bwtintv_t, bwt.h:59-61 */
typedef struct bmh_smem_opt {
	int32_t min_seed_len; /* mem_opt_t.min_seed_len (only used to bound the look-ups, not the calls)            */
	int32_t split_len;    /* (int)(min_seed_len*split_factor + .499), bwamem.c:211 (clamped to the read length there) */
	int32_t split_width;  /* mem_opt_t.split_width                                                              */
	int32_t start_width;  /* 2 with MEM_F_NO_EXACT, else 1, bwamem.c:212                                        */
	int32_t min_emit_len; /* 0: every interval of every call comes back, like bwt_smem1.  > 0: only intervals at least this
	                       * long do (call.n counts those) -- all that mem_insert_seed looks at with min_emit_len <=
	                       * min_seed_len (bwamem.c:219), about one interval in twenty on 150 bp reads; the calls made, their
	                       * arguments and return values are the same either way.  Must be >= 0; bmh_seed_batch and
	                       * bmh_chain_reads additionally need min_emit_len <= min_seed_len (chaining recomputes the longest
	                       * match and the re-seeding decision from the intervals it is given): BMH_E_ARG otherwise.
	                       * The struct is 20 bytes since BMH_VERSION 300 (16 before: rebuild callers)               */
} bmh_smem_opt_t;
typedef struct bmh_smem_call { /* one bwt_smem1 call and where its result intervals lie */
	int32_t x, min_intv; /* arguments (bwt.c:288)                         */
	int32_t ret, n;      /* return value and mem->n                       */
	uint32_t first;      /* first interval in the read's slice of the pool */
	uint32_t rsv;
} bmh_smem_call_t;

/* The index files of `bwa index` (<prefix>.bwt/.sa/.ann/.amb/.pac; reference bwt.c:380-421, bntseq.c:94-150, bwa.c:291)
 * read into plain arrays: what bmh_ctx_set_bwt / bmh_ctx_set_pac take.  Host I/O only, no GPU involved. */
typedef struct bmh_index {
	bmh_bwt_t bwt;    /* arrays owned by the index */
	int64_t l_pac;
	uint8_t *pac;     /* l_pac/4+1 bytes */
	int32_t n_seqs;   /* reference sequences (.ann): name, offset in the concatenation, length */
	char **names;
	int64_t *offsets;
	int32_t *lens;
	int32_t n_holes;  /* runs of ambiguous bases (.amb; bntamb1_t, bntseq.h:47-51): start, length, the letter */
	int64_t *hole_offsets;
	int32_t *hole_lens;
	char *hole_chars;
} bmh_index_t;
int bmh_index_load(const char *prefix, bmh_index_t **out); /* BMH_E_ARG if a file is missing or inconsistent */
void bmh_index_free(bmh_index_t *ix);

/* Make the index resident on the context's device: one copy per device, host arrays and shape (every field of *bwt),
 * shared by all contexts and kept for the life of the process.  The host arrays must not change while an index is
 * bound: the library does not compare contents, so new contents at the same addresses and with the same shape would
 * keep the old copy.  A different shape at the same addresses (an index freed and another built in its place) gets
 * a fresh copy. */
int bmh_ctx_set_bwt(bmh_ctx_t *ctx, const bmh_bwt_t *bwt);
/* For every read: the bwt_smem1 calls of smem_next2's iteration, in order.  Read r's calls are
 * calls[call_off[r] .. call_off[r+1]) and their intervals lie in intv[intv_off[r] + call.first ...].  call_off and
 * intv_off have n_reads+1 entries.  BMH_E_CIGAR_CAP if a capacity is too small (nothing partial is returned). */
int bmh_smem_batch(bmh_ctx_t *ctx, const bmh_smem_opt_t *o, int n_reads, const bmh_read_t *reads, uint32_t *call_off,
                   bmh_smem_call_t *calls, size_t call_cap, uint64_t *intv_off, bmh_smem_intv_t *intv, size_t intv_cap);
/* bmh_smem_batch + the suffix-array look-ups chaining will make, in ONE device round trip: for every interval that comes
 * back and is long and rare enough to become seeds (length >= o->min_seed_len, x[2] <= max_occ; bwamem.c:218-225),
 * sa_off[k] = index of its first position in sa_pos (its x[2] positions follow one another: bwt_sa(x[0] + j)), for the
 * others UINT64_MAX -- what bmh_chain_sa_keys + bmh_sa_batch produce, in the form bmh_chain_reads takes (the runs lie in
 * sa_pos in no particular order).  sa_off has intv_cap entries.  *n_pos (nullable) = positions written.
 * BMH_E_CIGAR_CAP if a capacity is too small. */
int bmh_seed_batch(bmh_ctx_t *ctx, const bmh_smem_opt_t *o, int max_occ, int n_reads, const bmh_read_t *reads, uint32_t *call_off,
                   bmh_smem_call_t *calls, size_t call_cap, uint64_t *intv_off, bmh_smem_intv_t *intv, size_t intv_cap, uint64_t *sa_off,
                   uint64_t *sa_pos, size_t sa_cap, uint64_t *n_pos);
/* N x bwt_sa: pos[i] = position (doubled coordinate) of suffix-array entry k[i]. */
int bmh_sa_batch(bmh_ctx_t *ctx, const uint64_t *k, int64_t n, uint64_t *pos);

/* ------------------------------------------------------------------------------------------------------------
 * Seeds to chains (the rest of SURVEY.md §8(f) row 3): host code over the results of bmh_smem_batch / bmh_sa_batch,
 * and the same on the device (bmh_chain_batch, bmh_seed_chain_batch at the end of this section).
 * Replaces: mem_chain (reference bwamem.c:283-306) = smem_next2's rounds (:118-157) + mem_insert_seed (:208-243, over
 *           test_and_merge :186-206 and klib's B-tree of chains) + the in-order read-out, followed by mem_chain_flt
 *           (:319-380) -- lines bwamem.c:1096-1097 of mem_align1_core_batched.
 * call_off / calls / intv_off / intv are bmh_smem_batch's outputs for the same reads.  The bwt_sa results come in
 * interval order: bmh_chain_sa_keys lists, for every interval that is long and rare enough (length >= min_seed_len,
 * x[2] <= max_occ), its suffix-array indices x[0]..x[0]+x[2]-1 and records in sa_off[k] where interval k's run starts
 * (UINT64_MAX = never looked up); the caller resolves the list with ONE bmh_sa_batch and passes the positions as sa_pos
 * -- no sorting, no searching.  chains[r] is filled like mem_chain's return value: a malloc'd array of chains in the
 * reference's order, each with a malloc'd seed array; the caller frees both.  bmh_chain_reads returns BMH_E_ARG when the
 * tables are inconsistent (a re-seeding record out of smem_next2's order, a long and rare interval without positions, a
 * call or read range outside the tables) and BMH_E_NOMEM when an allocation fails; either way no read keeps chains:
 * every chains[r] is {0, 0, NULL} and nothing is left allocated.
 * Precondition: the intervals come from a bmh_smem_batch / bmh_seed_batch run with min_emit_len <= o->min_seed_len (0
 * included): with a larger filter the longest match of a call and the re-seeding decision derived from it would be
 * computed from a truncated list and chains would silently differ. */
typedef struct bmh_chain_opt { /* the mem_opt_t fields seeding + chaining read (bwamem.h:21-48) */
	int32_t w, max_chain_gap, min_seed_len, max_occ;
	int32_t split_len;   /* (int)(min_seed_len * split_factor + .499), bwamem.c:211 */
	int32_t split_width;
	float mask_level, chain_drop_ratio;
} bmh_chain_opt_t;
uint64_t bmh_chain_sa_keys(const bmh_chain_opt_t *o, uint64_t n_intv, const bmh_smem_intv_t *intv, uint64_t *sa_off /* [n_intv] */,
                           uint64_t *keys /* NULL: count only */);
int bmh_chain_reads(const bmh_chain_opt_t *o, int64_t l_pac, int n_reads, const bmh_read_t *reads, const uint32_t *call_off,
                    const bmh_smem_call_t *calls, const uint64_t *intv_off, const bmh_smem_intv_t *intv, const uint64_t *sa_off,
                    const uint64_t *sa_pos, bmh_chain_v *chains);
/* bmh_chain_reads on the GPU: same inputs, same output form (chains[r].a and every seed array malloc'd, caller frees).
 * One lane per read simulates the same B-tree node for node, so chains, seeds and their order are bmh_chain_reads'.
 * n_pos: entries of sa_pos.  BMH_E_ARG (and no chains) when the tables are inconsistent: a re-seeding call out of
 * smem_next2's order, a long and rare interval without positions, offsets outside the arrays. */
int bmh_chain_batch(bmh_ctx_t *ctx, const bmh_chain_opt_t *o, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                    const uint32_t *call_off, const bmh_smem_call_t *calls, const uint64_t *intv_off,
                    const bmh_smem_intv_t *intv, const uint64_t *sa_off, const uint64_t *sa_pos, uint64_t n_pos,
                    bmh_chain_v *chains);
/* bmh_seed_batch + chaining in ONE device round trip: reads up, chains down; nothing else crosses PCIe.
 * Needs bmh_ctx_set_bwt.  so->min_seed_len / split_len / split_width must equal co's, so->min_emit_len <= co->min_seed_len
 * (BMH_E_ARG otherwise).  Capacities grow inside the call. */
int bmh_seed_chain_batch(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac,
                         int n_reads, const bmh_read_t *reads, bmh_chain_v *chains);
typedef struct bmh_chain_stats { /* of the last successful bmh_chain_batch / bmh_seed_chain_batch / bmh_seed_chain_regs_batch (-1: none yet) */
	int64_t reads, chains_in, chains_out, seeds; /* chains before / after mem_chain_flt; seeds of the chains kept */
	int64_t equal_keys; /* look-ups of the B-tree of chains that met an equal key (their answer depends on its splits) */
	float kernel_ms;    /* the chain kernel's duration with kernel timing on, else -1 */
} bmh_chain_stats_t;
int bmh_chain_stats(bmh_ctx_t *ctx, bmh_chain_stats_t *st);

/* ---- chains to regions on the device: the per-read driver of bmh_chains2regs_batch (windows, the short-chain pre-step, the replay of
 * the reference's control flow, the tasks of every round) as kernels, one lane per read.  Inside a call only 16-byte status words
 * cross PCIe between the launches; the regions come back compacted at the end.  Both calls need the 2-bit reference resident on the
 * device (bmh_ctx_set_pac with this l_pac; BMH_E_ARG otherwise) and reads of at most 65 535 bases (a longer one: BMH_E_RANGE before
 * anything runs, where the host driver looks at the flanks only).  BMH_E_RANGE where the host driver gives it (a seed outside its
 * window, a window over 2^31, the fused per-seed record's own limits); BMH_E_ARG for a caller's seed that does not lie inside its
 * read (len < 1, qbeg < 0, qbeg + len > l_seq), found on the device.  bmh_ctx_set_wide_extension is honoured.  bmh_driver_stats reports the call as it does the host driver's; pool_bytes is the sequence this call uploaded: the reads
 * plus 16 bytes of padding for bmh_chains2regs_device, 0 for bmh_seed_chain_regs_batch (seeding's copy of the reads is used).
 *
 * mem_chain2aln [+ mem_chain2aln_short when min_seed_len > 0] for n_reads reads, the whole driver on the device.
 * chains: as bmh_chain_reads / bmh_seed_chain_batch return them; uploaded in compact form.  regs[r] must be empty.
 * min_seed_len == 0: no short-chain pre-step (bmh_chain2aln_batch with pre == NULL); < 0: BMH_E_ARG. */
int bmh_chains2regs_device(bmh_ctx_t *ctx, int64_t l_pac, int n_reads, const bmh_read_t *reads,
                           const bmh_chain_v *chains, int min_seed_len, bmh_alnreg_v *regs);
/* seeding -> chaining -> regions; nothing but regions (and the statistics) comes back.  Arguments as bmh_seed_chain_batch's;
 * bmh_chain_stats is valid afterwards. */
int bmh_seed_chain_regs_batch(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int64_t l_pac,
                              int n_reads, const bmh_read_t *reads, int min_seed_len, bmh_alnreg_v *regs);

/* ---- mem_sort_and_dedup on the device (reference bwamem.c:395-436): the text of bmh_sort_and_dedup (host/dedup_core.h) as a kernel,
 * one lane per read, in place on the read's regions.  Bit-exact with the host routine, including which of two tied records survives:
 * both sorts are the same restatement of klib's introsort, and the redundancy test is the same single-precision expression.
 *
 * mem_sort_and_dedup for every vector of a batch in one device call: regions up, kernel, survivors back into the same regs[r].a.
 * regs[r].n is updated; a and m are untouched.  Needs neither parameters nor a resident reference.  BMH_E_ARG (and the vectors as
 * they were) for a NULL context, n_reads < 0, regs == NULL with n_reads > 0, a vector with n > 0 and a == NULL, or more than
 * 2^31-1 regions in all.  n_reads == 0 and batches of empty vectors: BMH_OK without a launch. */
int bmh_sort_dedup_batch(bmh_ctx_t *ctx, int n_reads, bmh_alnreg_v *regs, float mask_level_redun);
/* Per context, off by default.  While on, bmh_chains2regs_device and bmh_seed_chain_regs_batch run the kernel on the reads' region
 * slices after the last replay and before the gather, so only the survivors are placed, downloaded and malloc'd: regs[r] is what
 * bmh_sort_and_dedup(regs[r].n, regs[r].a, mask_level_redun) leaves of the switch-off result, record for record and in order.
 * bmh_driver_stats reports the same numbers either way (they are about extensions, not survivors).  A refused call leaves the
 * switch as set. */
int bmh_ctx_set_regs_dedup(bmh_ctx_t *ctx, int on, float mask_level_redun);
/* Of the last successful call on this context that ran the kernel (bmh_sort_dedup_batch, or a chains-to-regions call with the switch
 * on): regions in, regions kept, and the kernel's milliseconds with bmh_set_kernel_timing on (else -1).  -1 each before the first such
 * call.  Any of the three pointers may be NULL. */
int bmh_last_dedup_stats(const bmh_ctx_t *ctx, int64_t *regions_in, int64_t *regions_out, float *kernel_ms);

/* ---- mem_pestat's pair walk on the device (reference bwamem_pair.c:46-72): the text of bmh_pestat_candidates (host/pestat_core.h)
 * as a kernel, one lane per pair.  The words are bmh_pestat_candidates' words, bit for bit; the statistics stay on the host
 * (bmh_pestat_from_candidates).
 *
 * For a caller's own vectors: offsets, counts and regions up in one copy, the kernel, the words down, one wait.  Needs neither
 * parameters nor a resident reference.  Arguments as bmh_pestat_candidates' (an odd n ignores the last read); BMH_E_ARG as
 * bmh_sort_dedup_batch gives it, BMH_E_RANGE for o->max_ins >= 2^30.  n == 0 and batches of empty vectors: BMH_OK with zeroed
 * words and no launch. */
int bmh_pestat_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, int64_t l_pac, int n, const bmh_alnreg_v *regs, uint32_t *cand);
/* Two switches per context, off by default, both behind bmh_ctx_set_regs_dedup (which must be on).  While either is on,
 * bmh_chains2regs_device and bmh_seed_chain_regs_batch run the kernel on the reads' region slices after the de-duplication and
 * before the gather:
 *   drop exact   mem_test_and_remove_exact (bwamem.c:438-443) with MEM_F_NO_EXACT set: a read whose head region has
 *                truesc == l_seq * params.a loses it; the gather places, downloads and mallocs what is left
 *   collect      reads 2p and 2p+1 are mates; the word of every pair (bmh_pestat_candidates' under *o, which is copied) comes down
 *                with the regions' offsets, and bmh_last_pestat_candidates hands the words out.  The call waits as often as without.
 * Refused before anything is enqueued, the switches staying as set and the context usable: either switch on while regs_dedup is
 * off (BMH_E_ARG; bmh_last_error names the switch), collect with an odd n_reads (BMH_E_ARG), collect with max_ins >= 2^30
 * (BMH_E_RANGE).  bmh_driver_stats and bmh_last_dedup_stats report what they report without the switches. */
int bmh_ctx_set_regs_drop_exact(bmh_ctx_t *ctx, int on);
int bmh_ctx_set_pestat_collect(bmh_ctx_t *ctx, int on, const bmh_sam_opt_t *o);
/* The words of the last successful collecting call on this context, copied out of host memory the context owns (no device work),
 * and the kernel's milliseconds with bmh_set_kernel_timing on (else -1; nullable).  BMH_E_ARG when n_pairs is not that call's pair
 * count, when no such call has been made, and while drop exact is on and collect is off.  A successful call with n_reads == 0 is a
 * collecting call of 0 pairs (and one that removed 0 regions): n_pairs == 0 then answers BMH_OK, cand may be NULL. */
int bmh_last_pestat_candidates(bmh_ctx_t *ctx, uint32_t *cand, int64_t n_pairs, float *kernel_ms);
/* Regions drop exact removed in the last successful chains-to-regions call that ran with it on; -1 before the first. */
int bmh_last_drop_exact_stats(const bmh_ctx_t *ctx, int64_t *removed);

/* ---- Single-end reads to SAM text as one device session: seeding, chaining, chains to regions, the de-duplication, marking, mapQ,
 * the alignments and the text, with the region vectors on the device from the kernel that makes them to the kernel that sorts them.
 * *text / text_off[0..n] are byte for byte what this composition gives on a context whose de-duplication switch is on at
 * o->mask_level_redun:
 *   bmh_seed_chain_regs_batch(so, co, bns->l_pac, n, reads, min_seed_len, regs), reads[i] = seqs[i]'s bases, with
 *       bmh_ctx_set_regs_drop_exact on exactly when o->flag has MEM_F_NO_EXACT (0x40) and bmh_ctx_set_pestat_collect off, then
 *   bmh_phase2_text_device(o, bns, pac, NULL, id0, n, seqs, regs, rg_id, text, text_off).
 *   the hand-off  the chains-to-regions driver ends behind c2r_place_kernel: the compact records and their offsets stay in its
 *                 workspace, nothing of them comes down and no vector is made.  table_plan_kernel, one lane per read, finds what phase 2
 *                 otherwise learns by walking the vectors (host/handoff_core.h): the largest index of the log table, the negative-index
 *                 flag, the capacity of the oriented pool, the region total.  They come down in one 128-byte record with the driver's
 *                 status words: one wait where bmh_seed_chain_regs_batch has two, and as many bytes for one read as for a million.
 *   phase 2       bmh_phase2_text_device's session from those numbers.  Its upload leaves out the offsets and the regions; both are copied
 *                 on the stream, device to device, into pass A's block.  From decide_kernel on it is the same code, the redo included
 *                 (the list that comes down for it carries each redone region's record).  The bases still go up a second time, inside
 *                 pass C's per-read pool.
 * The call neither reads nor changes the context's bmh_ctx_set_regs_dedup, bmh_ctx_set_regs_drop_exact and bmh_ctx_set_pestat_collect
 * switches; it honours bmh_ctx_set_wide_extension, bmh_ctx_set_wide_sw and bmh_ctx_set_region_long as the two calls do.
 * Needs what the two calls need: the parameters, the FM-index, the resident 2-bit reference with this pac, the sequence table and the
 * sequence names: BMH_E_ARG without any of them.
 *   BMH_E_ARG    before anything runs: o->flag has BMH_MEM_F_PE (mate rescue lies between the phases there); a NULL ctx, so, co, o,
 *                bns, text or text_off; what either call refuses of n, seqs, so, co or o
 *   BMH_E_RANGE  before anything runs: a read longer than 65535 bases.  After phase 1 and before phase 2's upload: what
 *                bmh_phase2_text_device refuses there (a decide table past 1 << 20 entries, a negative table index, slot addresses
 *                past 32 bits); from the kernels: as in the two calls
 *   BMH_OK       for n == 0 with a 1-byte *text and text_off[0] = 0, nothing runs
 * All or nothing: on any error *text and text_off are untouched, and the context stays usable.
 * Afterwards bmh_driver_stats, bmh_chain_stats, bmh_last_dedup_stats and bmh_last_drop_exact_stats are valid as after
 * bmh_seed_chain_regs_batch, and bmh_last_phase2_text_stats as after bmh_phase2_text_device.
 * The preload shim makes this call once per batch of a single-end chunk under BMH_READS_SAM_DEVICE=1 (host/interpose.c) and ends the run
 * on any error: it has no other route for the batch. */
int bmh_reads_sam_device(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int min_seed_len, const bmh_sam_opt_t *o,
                         const bmh_refidx_t *bns, const uint8_t *pac, int64_t id0, int n, const bmh_seq_t *seqs, const char *rg_id,
                         char **text, int64_t *text_off);
/* Of the last bmh_reads_sam_device call on this context that got as far as the hand-off; all -1 before the first.
 *   reads                 of the batch
 *   regions_in, regions   before and after the de-duplication plus drop-exact
 *   kmax, opool_cap       what table_plan_kernel found: the largest index of the log table (at least 1), the oriented pool's capacity
 *   handoff_d2h_bytes     bytes that came down between the last replay round and phase 2's upload: 128, whatever n
 *   waits_tail            host waits behind the last replay round of chains-to-regions: 1 and phase 2's (bmh_last_phase2_text_stats)
 *   plan_ms               table_plan_kernel's milliseconds with bmh_set_kernel_timing on, else -1
 *   neg_index             1 where a region asked for a negative table index (the call then returned BMH_E_RANGE), else 0 */
typedef struct bmh_reads_sam_stats {
	int64_t reads, regions_in, regions;
	int64_t kmax, opool_cap, handoff_d2h_bytes;
	int32_t waits_tail;
	float plan_ms;
	int32_t neg_index, rsv_;
} bmh_reads_sam_stats_t; /* 64 bytes */
int bmh_last_reads_sam_stats(const bmh_ctx_t *ctx, bmh_reads_sam_stats_t *st);

/* ---- Paired-end reads to SAM text as one device session: bmh_reads_sam_device's two phases with the insert-size statistics and mate
 * rescue between them, and the region table on the device from the kernel that makes it, through the rescue that grows it, to the
 * kernel that sorts it.  Reads 2p and 2p + 1 are mates.  *text / text_off[0..n] are byte for byte what this composition gives on one
 * context:
 *   bmh_seed_chain_regs_batch(so, co, bns->l_pac, n, reads, min_seed_len, regs), reads[i] = seqs[i]'s bases, with
 *       bmh_ctx_set_regs_dedup on at o->mask_level_redun, bmh_ctx_set_regs_drop_exact on exactly when o->flag has MEM_F_NO_EXACT (0x40)
 *       and bmh_ctx_set_pestat_collect on under *o exactly when pes0 is NULL, then
 *   pes = pes0 if it is given (the caller's table: -I, or the table of a chunk the caller already has), else
 *       bmh_pestat_from_candidates(o, n / 2, that call's words, pes, quiet): the table of exactly this call's reads, then
 *   bmh_matesw_device(l_pac, n / 2, reads, regs, pes, mo, o->mask_level_redun, n_sw), then
 *   bmh_phase2_text_device(o, bns, pac, pes, id0, n, seqs, regs, rg_id, text, text_off).
 * pes_out (nullable) receives the table that was used.
 *   phase 1       bmh_reads_sam_device's, without the plan over its table.  Its status words and the table's total come down in one
 *                 wait; with pes0 NULL the insert-size words, 4 bytes per pair, come down in the same wait
 *   the barrier   the host makes the table from the words (bmh_pestat_from_candidates's arithmetic): inside the call, no wait of its own
 *   the rescue    bmh_matesw_table_device's kernels over phase 1's table where it lies, against the bases kept in a buffer of their own
 *                 (copied on the stream, device to device, from the pool seeding uploaded).  The table it leaves stays on the device
 *   the plan      the same table_plan_kernel, one lane per read over the table after rescue: what it finds there, and its paired-end
 *                 clause (the square of a pair's region count).  Its 64-byte record comes down with rescue's final 16-byte record
 *   phase 2       bmh_phase2_text_device's session from those numbers, the offsets and regions copied device to device
 * Nothing of the regions crosses the bus in either direction.  The bases still go up a second time, inside pass C's per-read pool.
 * The call neither reads nor changes the context's bmh_ctx_set_regs_dedup, bmh_ctx_set_regs_drop_exact and bmh_ctx_set_pestat_collect
 * switches (nor what bmh_last_pestat_candidates answers); it honours bmh_ctx_set_wide_extension, bmh_ctx_set_wide_sw and
 * bmh_ctx_set_region_long as the composition does.  Needs what the composition needs: the parameters, the FM-index, the resident 2-bit
 * reference with this pac, the sequence table and the sequence names: BMH_E_ARG without any of them.
 *   BMH_E_ARG    before anything runs: a NULL ctx, so, co, mo, o, bns, text or text_off; o->flag without BMH_MEM_F_PE; an odd n; mates
 *                whose names differ; what either phase refuses of n, seqs, so, co or o
 *   BMH_E_RANGE  before anything runs: a read longer than 65535 bases; o->max_ins >= 2^30 with pes0 NULL (the word cannot hold it).
 *                After phase 1 and before phase 2's upload: a pair table past 1 << 20 entries (before rescue runs); rescue's per-read
 *                refusals, in bmh_matesw_device's words; what bmh_phase2_text_device refuses there (a log table past 1 << 20 entries, a
 *                negative table index, slot addresses past 32 bits); from the kernels: as in the composition
 *   BMH_OK       for n == 0 with a 1-byte *text and text_off[0] = 0, nothing runs (pes_out: pes0, or all four orientations failed)
 * A table in which all four orientations failed is no error: rescue has no active pair then and the session runs through.
 * All or nothing: on any error *text, text_off and pes_out are untouched, and the context stays usable.
 * Afterwards bmh_chain_stats, bmh_last_dedup_stats and bmh_last_drop_exact_stats are valid as after bmh_seed_chain_regs_batch,
 * bmh_last_matesw_table_stats as after bmh_matesw_table_device (its mid_bytes with the plan record's 64 bytes, which ride on its last
 * copy) and bmh_last_phase2_text_stats as after bmh_phase2_text_device.
 * bmh_driver_stats holds the rescue's numbers, as after bmh_matesw_table_device (rounds, Smith-Waterman tasks; pool_bytes stays 0: the
 * bases did not go up for it); phase 1's extension counts are not kept. */
int bmh_pairs_sam_device(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int min_seed_len, const bmh_matesw_opt_t *mo,
                         const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes0,
                         bmh_pestat_t pes_out[4] /* nullable */, int64_t id0, int n, const bmh_seq_t *seqs, const char *rg_id, char **text,
                         int64_t *text_off);
/* Of the last bmh_pairs_sam_device call on this context that got as far as the plan over rescue's table; all -1 before the first.
 *   reads, pairs          of the call
 *   regions_in, regions   before and after the de-duplication plus drop-exact
 *   regions_out           after rescue
 *   n_sw                  mem_matesw's Smith-Waterman count, summed over the pairs
 *   kmax, pair_kmax, opool_cap   what table_plan_kernel found: the largest index of the log table the regions ask for (at least 1), the
 *                         largest bmh_ho_pair_kmax of a pair, the oriented pool's capacity
 *   mid_d2h_bytes         bytes that came down between phase 1's last replay round and phase 2's upload: 72 (phase 1's status words and
 *                         total) + 64 (rescue's plan) + 16 per rescue round + 80 (rescue's total and the plan record), and 4 per pair with
 *                         pes0 NULL: nothing that grows with the regions
 *   mid_h2d_bytes         bytes that went up in the same span: 0
 *   waits_mid             host waits in the same span: 3 + rescue's rounds, that is 1 + bmh_last_matesw_table_stats' waits
 *   pes_given             1 if the caller supplied the table
 *   plan_ms               table_plan_kernel's milliseconds with bmh_set_kernel_timing on, else -1
 *   neg_index             1 where a region asked for a negative table index (the call then returned BMH_E_RANGE), else 0 */
typedef struct bmh_pairs_sam_stats {
	int64_t reads, pairs, regions_in, regions, regions_out, n_sw;
	int64_t kmax, pair_kmax, opool_cap, mid_d2h_bytes, mid_h2d_bytes;
	int32_t waits_mid, pes_given;
	float plan_ms;
	int32_t neg_index, rsv_[6];
} bmh_pairs_sam_stats_t; /* 128 bytes */
int bmh_last_pairs_sam_stats(const bmh_ctx_t *ctx, bmh_pairs_sam_stats_t *st);

/* ---- The same session in two calls, cut at the insert-size barrier: for a caller whose table is a whole chunk's and whose chunk is
 * many batches (the preload shim).  bmh_pairs_sam_begin is the session's phase 1; bmh_pairs_sam_finish is its rescue, plan and phase 2
 * under the table the caller made from every batch's words.  begin + bmh_pestat_from_candidates over the words + finish gives the
 * bytes of bmh_pairs_sam_device with that table as pes0.
 *   begin    the one-call form's checks up to phase 1 (BMH_MEM_F_PE, an even n, mates named alike, what phase 1 refuses, and with cand
 *            o->max_ins below 2^30), then its phase 1, the words collected exactly when cand is given (n / 2 words, written on success
 *            only).  What phase 1 leaves in the context's workspaces -- the table's offsets and regions, the bases' offsets, the bases
 *            and 16 zero bytes -- is then copied on the stream, device to device, into ONE block of its own, and *parked names it.
 *            The table's total is known only behind phase 1's wait, so the copy has a wait of its own, which the
 *            statistics of finish count in waits_mid.  When begin
 *            returns nothing of it is in flight, and the block stays valid whatever any context does afterwards.  n == 0 parks no
 *            block (the handle is still made).  On any error *parked is untouched.
 *   finish   on any context of the block's device (BMH_E_ARG with another device's).  Before anything runs, with the handle left
 *            valid: a NULL argument, BMH_E_ARG for an n or read lengths other than the parked ones, what bmh_phase2_text_device
 *            refuses of its arguments, and BMH_E_RANGE for a pair table past 1 << 20 entries.  Past those the handle is consumed
 *            whatever the result: the caller must not use or free it again.  Then rescue over the parked table and bases, the plan
 *            over its output, and phase 2 -- in which pass C's per-read pool goes up WITHOUT the bases: the kernels read them from
 *            the parked block (h2d_bytes is smaller by the difference of the two pools), and pass B's reads pool is gathered from
 *            there.  The host's redo of outgrown alignments reads seqs.
 * Afterwards the bmh_last_* calls answer as after bmh_pairs_sam_device; bmh_last_pairs_sam_stats has pes_given = 1,
 * waits_mid = 2 + bmh_last_matesw_table_stats' waits (one more than the one-call form: the copy's) and mid_d2h_bytes as in the one-call form (begin's share included).
 * Blocks are recycled through a process-wide, mutex-guarded free list per device that only grows: neither finish nor
 * bmh_pairs_parked_free gives memory back to the runtime (that would synchronise every stream of the device in the middle of a
 * chunk); bmh_pairs_parked_trim does, for the blocks that are idle at that moment.
 * bmh_pairs_parked_free(NULL) does nothing; freeing an unfinished handle returns its block to the list. */
typedef struct bmh_pairs_parked bmh_pairs_parked_t;
typedef struct bmh_pairs_parked_info {
	int32_t device, reads; /* the block's device; n as parked */
	int64_t regions, bytes; /* the parked table's records; the bytes of the block that are in use (0 for n == 0) */
} bmh_pairs_parked_info_t; /* 24 bytes */
int bmh_pairs_sam_begin(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int min_seed_len, const bmh_sam_opt_t *o,
                        const bmh_refidx_t *bns, int n, const bmh_seq_t *seqs, uint32_t *cand /* n / 2 words, nullable */,
                        bmh_pairs_parked_t **parked);
int bmh_pairs_sam_finish(bmh_ctx_t *ctx, bmh_pairs_parked_t *parked, const bmh_matesw_opt_t *mo, const bmh_sam_opt_t *o,
                         const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t pes[4], int64_t id0, int n, const bmh_seq_t *seqs,
                         const char *rg_id, char **text, int64_t *text_off);
/* 1 if the last bmh_pairs_sam_finish on this context consumed its handle, 0 if it left it valid (or none ran yet): for a binding that
 * cannot tell the two from the return code */
int bmh_pairs_finish_consumed(const bmh_ctx_t *ctx);
void bmh_pairs_parked_free(bmh_pairs_parked_t *parked);
int bmh_pairs_parked_info(const bmh_pairs_parked_t *parked, bmh_pairs_parked_info_t *info);
int bmh_pairs_parked_trim(int device);

#ifdef __cplusplus
}
#endif
#endif
