/*
 * interpose.c -- the reference-side binding, as an LD_PRELOAD-able object.
 *
 * It provides mem_align1_core_batched() with the fork's exact signature
 * (reference bwa-0.7.8/bwamem.c:1086) so that, preloaded in front of a build of the
 * reference (oracle/_ref/bwa + libbwa_ref.so), phase 1 of mem_process_seqs
 * (bwamem.c:1313 -> worker1_batched :1264) runs on the library, in one of three forms:
 *   default              seeding as one device batch (bmh_seed_batch), chaining on the host
 *                        (bmh_chain_reads), then the batch's chains go to bmh_chains2regs_batch()
 *                        -- the hook the fork left commented out at bwamem.c:1110: short-chain
 *                        Smith-Watermans and fused per-seed extensions on the device, the
 *                        per-read control flow replayed on the host;
 *   BMH_CHAIN_DEVICE=1   chaining fused with seeding on the device (bmh_seed_chain_batch), the
 *                        chains come back and go to bmh_chains2regs_batch() as above;
 *   BMH_REGS_DEVICE=1    ONE call, bmh_seed_chain_regs_batch(): seeding, chaining and the
 *                        chains-to-regions driver on the device, only regions come back.  Needs
 *                        the reference resident on the device (BMH_PAC_RESIDENT not 0).
 * After it the host sorts and de-duplicates each read's regions (bmh_sort_and_dedup) -- or, with
 *   BMH_DEDUP_DEVICE=1   (needs BMH_REGS_DEVICE=1) the same call does that on the device before the regions come down
 *                        (bmh_ctx_set_regs_dedup) and phase 1 makes no host bmh_sort_and_dedup call.
 *   BMH_PESTAT_DEVICE=1  (needs the two above) behind that, the same call answers mem_pestat's question per pair (bmh_ctx_set_pestat_collect)
 *                        and under -e applies mem_test_and_remove_exact (bmh_ctx_set_regs_drop_exact): a paired-end chunk's serial
 *                        section is bmh_pestat_from_candidates over four bytes per pair, not bmh_pestat over the region vectors.
 * Mate rescue (bmh_matesw_batch per slice of the chunk) has a switch of its own:
 *   BMH_MATESW_DEVICE=1  mate rescue's driver (planning, folding, mem_sort_and_dedup) as kernels, bmh_matesw_device(): no host
 *                        callback, 16 bytes per round back.  Needs BMH_PAC_RESIDENT not 0; independent of BMH_REGS_DEVICE.
 * Phase 2 (bmh_sam_batch per slice) has one too:
 *   BMH_DECIDE_DEVICE=1  its pass A -- primary marking, pairing, mapQ, the list of regions that get printed -- as a kernel
 *                        (bmh_ctx_set_decide_device); a slice the device call refuses as out of range is decided on the host.
 *                        Independent of the other switches; needs no resident reference.
 *   BMH_WANTED_DEVICE=1  its pass B's planning -- the bwa_fix_xref2 test and cut, bands, region records and tasks of the regions that
 *                        get printed -- as kernels (bmh_ctx_set_wanted_device).  Needs BMH_PAC_RESIDENT not 0; independent of the
 *                        other switches.
 *   BMH_REGION_LONG=1    the alignments of pass B whose CIGAR or MD outgrow the region record's slots -- on long reads, all of them --
 *                        are finished on the device behind the others (bmh_ctx_set_region_long) instead of being redone with oriented
 *                        copies made on the host.  Needs BMH_PAC_RESIDENT not 0; holds for every form of pass B above and below.
 *   BMH_PHASE2_DEVICE=1  pass A and pass B as ONE device session (bmh_ctx_set_phase2_device): the regions go up once and the want
 *                        list never leaves the device between the two.  Needs BMH_PAC_RESIDENT not 0.  A slice the fused call
 *                        refuses as out of range goes the way the two switches above say.
 *   BMH_SAMTEXT_DEVICE=1 its pass C -- coordinates, clipping, flags and the SAM text -- as kernels (bmh_ctx_set_samtext_device), with the
 *                        sequence table and the sequence names resident.  Needs no resident reference (BMH_PAC_RESIDENT=0 is fine);
 *                        independent of the other switches.  The text is the same bytes either way.
 *   BMH_PHASE2_TEXT_DEVICE=1  passes A, B and C as ONE device session (bmh_ctx_set_phase2_text_device): the regions and the reads go up
 *                        once and only SAM text comes down; the few alignments that outgrow the device's slots are redone on the host
 *                        and patched in.  Needs BMH_PAC_RESIDENT not 0; makes the sequence table and the names resident.  A slice the
 *                        fused call refuses as out of range goes the way the switches above say.
 * A single-end chunk has a route of its own that replaces all of the above:
 *   BMH_READS_SAM_DEVICE=1  both phases as ONE device session per batch (bmh_reads_sam_device): the reads go up, only SAM text comes
 *                        down, and the regions never exist on the host.  A chunk has no serial section without insert-size statistics,
 *                        so there is no barrier between the phases either: one job per batch of `-b` reads, from bases to strings.
 *                        Needs BMH_PAC_RESIDENT not 0; needs none of the other switches and consults none of them, BMH_REGION_LONG
 *                        excepted.  A call that refuses a batch ends the run: there is no other route for it.  Paired-end chunks go
 *                        the way they go without the switch.
 * So has a paired-end chunk:
 *   BMH_PAIRS_SAM_DEVICE=1  the same per batch of an even number of reads, cut in two at the insert-size barrier: pass 1 parks every
 *                        batch's region table and bases on the device (bmh_pairs_sam_begin) and brings its insert-size words down, the
 *                        chunk's table is made from all of them, pass 2 finishes every batch from its parked block
 *                        (bmh_pairs_sam_finish).  With -I the table is given and each batch is one bmh_pairs_sam_device.  Needs
 *                        BMH_PAC_RESIDENT not 0; consults no other switch but BMH_REGION_LONG; independent of BMH_READS_SAM_DEVICE.
 *                        Off for a chunk (which then goes the default way) with -P or -S, an odd or empty chunk, BMH_BATCH_EXACT=1 with an
 *                        odd -b, max_ins >= 2^30 without -I, and more than one device in BMH_DEVICES.  Threads: BMH_PS_THREADS.
 * Run `bwa mem -b <batch>` to choose the batch size.
 * INTEGRATION.md shows the same code as a patch to bwamem.c.
 *
 * Everything declared `extern` below is the reference's own symbol, resolved at load
 * time from libbwa_ref.so; nothing of the reference is compiled into this library.
 * The struct mirrors are layout-compatible re-declarations (file:line cited).
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <malloc.h>

#include <pthread.h>
#include <semaphore.h>

#include "../../include/bwamem_hip.h"
#include "samcut_core.h"
#include "tls_ctx.h"

/* At most this many host threads are inside a GPU batch call at a time ($BMH_GPU_CONCURRENCY, default 12): the calls of
 * more threads than that only queue up behind one another on the device, and their workspace (re)allocations, which
 * synchronise the whole device, collide.  The host work around the calls (chaining, folding) is not limited. */
static sem_t g_gpu_sem;
static pthread_once_t g_gpu_once = PTHREAD_ONCE_INIT;
static int gpu_concurrency(void)
{
	const char *e = getenv("BMH_GPU_CONCURRENCY");
	return e && atoi(e) > 0 ? atoi(e) : 12;
}
static void gpu_sem_init(void) { sem_init(&g_gpu_sem, 0, (unsigned)gpu_concurrency()); }
static void gpu_enter(void)
{
	pthread_once(&g_gpu_once, gpu_sem_init);
	while (sem_wait(&g_gpu_sem) != 0) {}
}
static void gpu_leave(void) { sem_post(&g_gpu_sem); }

/* When the shim is loaded: create the contexts the run will use in the background, while the host program parses its
 * arguments and loads its index ($BMH_PREWARM=0 turns this off, =N creates N; default: the host program's -t). */
static int g_prewarm_n = 16; /* contexts to create ahead: one per host thread of the widest phase (a thread holds one while it is inside a driver call) */
/* The first chunk's host code runs on heaps that have never been touched: every page of the drivers' work arrays is a
 * page fault (chaining 1.05 thread-seconds in the first chunk of a run against 0.11 in the next ones).  While the host
 * program still parses its input, one short-lived thread per worker touches $BMH_HEAP_WARM_MB (64) megabytes through
 * malloc and frees them again: glibc keeps a finished thread's arena, mapped and resident (M_TRIM_THRESHOLD above), and
 * hands it to the next new thread -- the workers of kt_for. */
static void *heap_warm_thread(void *arg)
{
	const int mb = (int)(intptr_t)arg;
	void **p = (void **)malloc(sizeof(void *) * (size_t)(mb > 0 ? mb : 1));
	int k;
	if (!p) return 0;
	for (k = 0; k < mb; ++k)
		if ((p[k] = malloc(1 << 20)) != 0) memset(p[k], 0, 1 << 20);
	for (k = 0; k < mb; ++k) free(p[k]);
	free(p);
	return 0;
}
static void heap_warm(int threads)
{
	const char *e = getenv("BMH_HEAP_WARM_MB");
	const int mb = e ? atoi(e) : 64;
	int k;
	for (k = 0; k < threads && mb > 0; ++k) {
		pthread_t t;
		if (pthread_create(&t, 0, heap_warm_thread, (void *)(intptr_t)mb) == 0) pthread_detach(t);
	}
}

extern double cputime(void), realtime(void); /* the host program's (utils.c) */
static double g_t_loaded; /* realtime() when the shim was loaded */
static void qa_shim_exit(void);
static void *prewarm_thread(void *arg)
{
	int ndev = 0;
	(void)arg;
	/* The HIP runtime registers its own exit handlers when it is first initialised -- here, in this thread.  Exit handlers run
	 * last-registered-first, so the stop-and-join handler is registered AFTER that first HIP call: it then runs BEFORE the
	 * runtime's teardown whatever the order of the two libraries' constructors was.  (It is idempotent; the constructor
	 * registers it too, for a run that ends before this line.) */
	bmh_device_count(&ndev);
	atexit(qa_shim_exit);
	bmh_pool_prewarm(g_prewarm_n); /* (several threads creating contexts side by side are no faster: measured) */
	if (getenv("BMH_VERBOSE")) fprintf(stderr, "[bwamem_hip] %d contexts ready %.3f s after the shim was loaded\n", g_prewarm_n, realtime() - g_t_loaded);
	return 0;
}
/* A run shorter than the pre-warming (a few hundred reads) must not reach the runtime's teardown with that thread still
 * inside a HIP call: it is told to stop and waited for. */
static pthread_t g_prewarm;
static volatile int g_prewarm_on;
static void qa_shim_exit(void)
{
	if (!__sync_bool_compare_and_swap(&g_prewarm_on, 1, 0)) return; /* once, whichever registration fires first */
	bmh_pool_stop();
	pthread_join(g_prewarm, 0);
}
__attribute__((constructor)) static void qa_shim_loaded(void)
{
	const char *e = getenv("BMH_PREWARM"), *pl = getenv("LD_PRELOAD");
	pthread_t t;
	/* The HIP runtime multiplexes all streams of a process onto 4 hardware queues by default; with many host threads inside
	 * batch calls a thread's small extension kernels then wait behind another thread's seeding or Smith-Waterman kernel
	 * of milliseconds that happens to share its queue (measured, steady-state chunk of 1.07 M reads at 16 threads: 0.48 s
	 * with 4 queues, 0.35 s with 8, 0.28 s with 16 and 12 threads admitted to the GPU at a time; 24 is slower again).
	 * Must be in the environment before the runtime initialises; a value the user has set is left alone. */
	setenv("GPU_MAX_HW_QUEUES", "16", 0);
	bmh_set_device_gate(gpu_enter, gpu_leave); /* the library holds a GPU place for its device sections only */
	/* The drivers allocate and free a few buffers of megabytes per batch on every thread: keep that memory in the heaps
	 * instead of handing it back to the kernel and faulting it in again each time (mprotect/munmap/page faults were ~8 % of
	 * the CPU time of a chunk). */
	{
		const char *m = getenv("BMH_MALLOPT");
		const int bits = m ? atoi(m) : 3; /* (a larger M_TOP_PAD, bit 4, measured much slower) */
		if (bits & 1) mallopt(M_TRIM_THRESHOLD, 1 << 30);
		if (bits & 2) mallopt(M_MMAP_THRESHOLD, 32 << 20);
		if (bits & 4) mallopt(M_TOP_PAD, 16 << 20);
	}
	{ /* as many host threads as cores drive the library here: a thread waiting for the GPU sleeps instead of spinning
	   * (BMH_WAIT=spin restores the library's default) */
		const char *w = getenv("BMH_WAIT");
		bmh_set_wait_mode(!(w && !strcmp(w, "spin")));
	}
	if (e && e[0] == '0') return;
	if (!pl || !strstr(pl, "libbwamem_hip_dropin")) return; /* only when preloaded into a host program, not when merely dlopen()ed */
	{ /* ... and only into `<prog> mem ...`: index building, usage errors etc. never touch the GPU */
		char buf[512];
		FILE *f = fopen("/proc/self/cmdline", "rb");
		size_t n = f ? fread(buf, 1, sizeof(buf) - 1, f) : 0, i, first_len;
		int is_mem = 0;
		if (f) fclose(f);
		buf[n] = 0;
		first_len = strlen(buf);
		for (i = first_len + 1; i < n; i += strlen(buf + i) + 1)
			if (!strcmp(buf + i, "mem")) { is_mem = 1; break; }
		if (!is_mem) return;
		for (; i < n; i += strlen(buf + i) + 1) /* its -t, as `-t N` or `-tN` */
			if (buf[i] == '-' && buf[i + 1] == 't') {
				const char *v = buf[i + 2] ? buf + i + 2 : (i + 3 < n ? buf + i + 3 : "");
				if (atoi(v) > 0) g_prewarm_n = atoi(v);
			}
		{ /* phase 2 runs -t * 3/2 threads; $BMH_P1_THREADS / $BMH_P2_THREADS / $BMH_RS_THREADS / $BMH_PS_THREADS override the phases' thread counts; $BMH_PREWARM=N: N */
			const char *v[5] = {getenv("BMH_P1_THREADS"), getenv("BMH_P2_THREADS"), getenv("BMH_RS_THREADS"), getenv("BMH_PS_THREADS"), e};
			int k;
			g_prewarm_n += g_prewarm_n / 2;
			for (k = 0; k < 4; ++k)
				if (v[k] && atoi(v[k]) > g_prewarm_n) g_prewarm_n = atoi(v[k]);
			if (v[4] && atoi(v[4]) > 0) g_prewarm_n = atoi(v[4]);
			if (g_prewarm_n > 128) g_prewarm_n = 128;
		}
	}
	g_t_loaded = realtime();
	heap_warm(g_prewarm_n);
	if (pthread_create(&t, 0, prewarm_thread, 0) == 0) {
		g_prewarm = t, g_prewarm_on = 1;
		atexit(qa_shim_exit); /* a run that ends before the pre-warming thread's first HIP call; see prewarm_thread for the other case */
	}
}

typedef struct { /* mem_opt_t of the fork, bwamem.h:21-48 */
	int a, b, o_del, e_del, o_ins, e_ins, pen_unpaired, pen_clip5, pen_clip3, w, zdrop;
	int T, flag, min_seed_len;
	float split_factor;
	int split_width, max_occ, max_chain_gap, n_threads, batch_size, chunk_size;
	float mask_level, chain_drop_ratio, mask_level_redun, mapQ_coef_len;
	int mapQ_coef_fac, max_ins, max_matesw;
	int8_t mat[25];
} ref_mem_opt_t;
#define REF_MEM_F_NO_EXACT 0x40 /* bwamem.h:19 */

typedef struct { int64_t l_pac; /* first field of bntseq_t, bntseq.h:53 */ } ref_bntseq_head_t;
typedef struct { int l_seq; char *name, *comment, *seq, *qual, *sam; } ref_bseq1_t; /* bwa.h:18-22 */

/* what this shim still takes from the host program: its base-code table and its clocks (bntseq.c, utils.c) */
extern unsigned char nst_nt4_table[256];
static double stage_now(void) /* the clock of the BMH_VERBOSE thread-second sums: wall time, or with BMH_TRACE_CPU the thread's CPU time */
{
	static int cpu = -1;
	struct timespec ts;
	if (cpu < 0) cpu = getenv("BMH_TRACE_CPU") != 0;
	if (!cpu) return realtime();
	clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
	return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* ---- seeding: the batch's FM-index queries on the GPU, chaining on top of them -----------------------------------------
 * mem_chain (bwamem.c:283) = SMEM search (smem_next2 -> bwt_smem1) + suffix-array look-ups (bwt_sa) + chaining in a
 * B-tree.  The first two are pure functions of (index, read): bmh_smem_batch and bmh_sa_batch compute them for the whole
 * batch; bmh_chain_reads (host/chain_batch.c) then does what mem_chain and mem_chain_flt do with them. */
typedef struct { /* bwt_t, bwt.h:45-57 */
	uint64_t primary, L2[5], seq_len, bwt_size;
	uint32_t *bwt;
	uint32_t cnt_table[256];
	int sa_intv;
	uint64_t n_sa;
	uint64_t *sa;
} ref_bwt_t;

typedef struct {
	const ref_bwt_t *bwt;
	int n_reads;
	const bmh_read_t *reads;
	uint32_t *call_off;
	bmh_smem_call_t *calls;
	uint64_t *intv_off;
	bmh_smem_intv_t *intv;
	uint64_t *sa_k, *sa_pos; /* per interval: where its run of positions starts (bmh_chain_sa_keys); the positions */
	size_t n_sa;
} qa_seed_t;
static double g_seed_density[3] = {0.06, 0.02, 0.03}; /* calls, intervals, suffix-array positions per base */
static long long g_seed_us[3]; /* thread-microseconds: bmh_smem_batch, building the look-up keys, bmh_sa_batch */
static __thread qa_seed_t *qa_seed; /* the batch this thread is chaining */

/* the index on the context's device, and the seeding options of mem_opt_t */
static void qa_seed_setup(bmh_ctx_t *ctx, const ref_mem_opt_t *opt, const ref_bwt_t *bwt, bmh_smem_opt_t *so)
{
	bmh_bwt_t ib;
	int i, rc;
	ib.primary = bwt->primary, ib.seq_len = bwt->seq_len, ib.bwt_size = bwt->bwt_size, ib.bwt = bwt->bwt;
	for (i = 0; i < 5; ++i) ib.L2[i] = bwt->L2[i];
	ib.sa_intv = bwt->sa_intv, ib.n_sa = bwt->n_sa, ib.sa = bwt->sa;
	if ((rc = bmh_ctx_set_bwt(ctx, &ib))) bmh_tls_die(bmh_last_error(ctx), rc);
	so->min_seed_len = opt->min_seed_len, so->split_len = (int)(opt->min_seed_len * opt->split_factor + .499); /* bwamem.c:211 */
	so->split_width = opt->split_width, so->start_width = (opt->flag & REF_MEM_F_NO_EXACT) ? 2 : 1;           /* bwamem.c:212 */
	so->min_emit_len = opt->min_seed_len; /* shorter intervals are never turned into seeds (bwamem.c:219): they stay on the device */
}

static void qa_chain_opt(const ref_mem_opt_t *opt, bmh_chain_opt_t *co)
{
	co->w = opt->w, co->max_chain_gap = opt->max_chain_gap, co->min_seed_len = opt->min_seed_len, co->max_occ = opt->max_occ;
	co->split_len = (int)(opt->min_seed_len * opt->split_factor + .499), co->split_width = opt->split_width;
	co->mask_level = opt->mask_level, co->chain_drop_ratio = opt->chain_drop_ratio;
}

static void qa_seed_batch_begin(bmh_ctx_t *ctx, const ref_mem_opt_t *opt, const ref_bwt_t *bwt, int n, const bmh_read_t *reads)
{
	bmh_smem_opt_t so;
	qa_seed_t *S;
	size_t tot = 0, call_cap, intv_cap, nk = 0;
	uint64_t *keys = 0;
	double ts[4];
	int r, rc;
	qa_seed = 0;
	qa_seed_setup(ctx, opt, bwt, &so);
	for (r = 0; r < n; ++r) tot += (size_t)reads[r].l_seq;
	S = (qa_seed_t *)calloc(1, sizeof(*S));
	S->bwt = bwt, S->n_reads = n, S->reads = reads;
	S->call_off = (uint32_t *)malloc(4 * ((size_t)n + 1)), S->intv_off = (uint64_t *)malloc(8 * ((size_t)n + 1));
	/* output arrays sized from the densest batch seen so far in this process (calls / intervals / positions per base) */
	ts[0] = stage_now();
	if (!(getenv("BMH_SEED_FUSED") && getenv("BMH_SEED_FUSED")[0] == '0')) {
		/* SMEMs and the suffix-array entries chaining will ask for (bwamem.c:218-225) in one device round trip */
		size_t sa_cap;
		uint64_t n_pos = 0;
		for (call_cap = (size_t)(g_seed_density[0] * 1.3 * (double)tot) + 4 * (size_t)n + 64,
		    intv_cap = (size_t)(g_seed_density[1] * 1.3 * (double)tot) + 1024, sa_cap = (size_t)(g_seed_density[2] * 1.3 * (double)tot) + 4096;;
		     call_cap *= 2, intv_cap *= 2, sa_cap *= 2) {
			S->calls = (bmh_smem_call_t *)malloc(sizeof(bmh_smem_call_t) * call_cap);
			S->intv = (bmh_smem_intv_t *)malloc(sizeof(bmh_smem_intv_t) * intv_cap);
			S->sa_k = (uint64_t *)malloc(8 * intv_cap), S->sa_pos = (uint64_t *)malloc(8 * sa_cap);
			rc = bmh_seed_batch(ctx, &so, opt->max_occ, n, reads, S->call_off, S->calls, call_cap, S->intv_off, S->intv, intv_cap, S->sa_k, S->sa_pos,
			                    sa_cap, &n_pos);
			if (rc != BMH_E_CIGAR_CAP) break;
			free(S->calls), free(S->intv), free(S->sa_k), free(S->sa_pos);
		}
		if (rc) bmh_tls_die(bmh_last_error(ctx), rc);
		S->n_sa = (size_t)n_pos;
		ts[1] = ts[2] = ts[3] = stage_now();
		if (tot) { /* (a benign race: statistics that only size buffers) */
			const double dc = (double)S->call_off[n] / (double)tot, di = (double)S->intv_off[n] / (double)tot, dp = (double)n_pos / (double)tot;
			if (dc > g_seed_density[0]) g_seed_density[0] = dc;
			if (di > g_seed_density[1]) g_seed_density[1] = di;
			if (dp > g_seed_density[2]) g_seed_density[2] = dp;
		}
	} else { /* the same in three calls (the A/B path): bmh_smem_batch, bmh_chain_sa_keys, bmh_sa_batch */
		for (call_cap = (size_t)(g_seed_density[0] * 1.3 * (double)tot) + 4 * (size_t)n + 64,
		    intv_cap = (size_t)(g_seed_density[1] * 1.3 * (double)tot) + 1024;;
		     call_cap *= 2, intv_cap *= 2) {
			S->calls = (bmh_smem_call_t *)malloc(sizeof(bmh_smem_call_t) * call_cap);
			S->intv = (bmh_smem_intv_t *)malloc(sizeof(bmh_smem_intv_t) * intv_cap);
			rc = bmh_smem_batch(ctx, &so, n, reads, S->call_off, S->calls, call_cap, S->intv_off, S->intv, intv_cap);
			if (rc != BMH_E_CIGAR_CAP) break;
			free(S->calls), free(S->intv);
		}
		if (rc) bmh_tls_die(bmh_last_error(ctx), rc);
		ts[1] = stage_now();
		if (tot) {
			const double dc = (double)S->call_off[n] / (double)tot, di = (double)S->intv_off[n] / (double)tot;
			if (dc > g_seed_density[0]) g_seed_density[0] = dc;
			if (di > g_seed_density[1]) g_seed_density[1] = di;
		}
		{
			bmh_chain_opt_t co;
			memset(&co, 0, sizeof(co));
			co.min_seed_len = opt->min_seed_len, co.max_occ = opt->max_occ;
			S->sa_k = (uint64_t *)malloc(8 * (S->intv_off[n] + 1)); /* here: sa_off, one entry per interval */
			nk = (size_t)bmh_chain_sa_keys(&co, S->intv_off[n], S->intv, S->sa_k, 0);
			keys = (uint64_t *)malloc(8 * (nk + 1)), S->sa_pos = (uint64_t *)malloc(8 * (nk + 1));
			bmh_chain_sa_keys(&co, S->intv_off[n], S->intv, S->sa_k, keys);
			S->n_sa = nk;
		}
		ts[2] = stage_now();
		if ((rc = bmh_sa_batch(ctx, keys, (int64_t)nk, S->sa_pos))) bmh_tls_die(bmh_last_error(ctx), rc);
		free(keys);
		ts[3] = stage_now();
	}
	__sync_fetch_and_add(&g_seed_us[0], (long long)((ts[1] - ts[0]) * 1e6)), __sync_fetch_and_add(&g_seed_us[1], (long long)((ts[2] - ts[1]) * 1e6));
	__sync_fetch_and_add(&g_seed_us[2], (long long)((ts[3] - ts[2]) * 1e6));
	qa_seed = S;
}

static void qa_seed_batch_end(void)
{
	qa_seed_t *S = qa_seed;
	qa_seed = 0;
	if (!S) return;
	free(S->call_off), free(S->calls), free(S->intv_off), free(S->intv), free(S->sa_k), free(S->sa_pos), free(S);
}

static long long g_p1_cnt[4]; /* chains, seeds extended, seeds speculated in vain, short-chain Smith-Watermans */
static long long g_p1_us[5]; /* phase 1, thread-microseconds: wait for a GPU slot, seeding batch (with BMH_CHAIN_DEVICE=1: seeding + chaining),
                              * chaining on the host (0 with BMH_CHAIN_DEVICE=1), wait, extension batch */
static long long g_seedchain_us; /* thread-microseconds in bmh_seed_chain_batch (BMH_CHAIN_DEVICE=1) */

/* BMH_REGS_DEVICE=1 extends from the reference resident on the device, so BMH_PAC_RESIDENT=0 contradicts it.  Checked once when the
 * library is loaded, before anything has opened the GPU, and left with a plain exit status: no context to tear down, no core. */
__attribute__((constructor)) static void qa_check_regs_device_env(void)
{
	const char *e = getenv("BMH_REGS_DEVICE"), *r = getenv("BMH_PAC_RESIDENT");
	if (e && e[0] && strcmp(e, "0") != 0 && r && r[0] == '0') {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_REGS_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n");
		exit(1);
	}
}

/* BMH_DEDUP_DEVICE=1 de-duplicates the regions where bmh_seed_chain_regs_batch leaves them, so it means nothing without
 * BMH_REGS_DEVICE=1.  Checked like the one above: once at load, before the GPU is opened. */
__attribute__((constructor)) static void qa_check_dedup_device_env(void)
{
	const char *d = getenv("BMH_DEDUP_DEVICE"), *e = getenv("BMH_REGS_DEVICE");
	if (d && d[0] && strcmp(d, "0") != 0 && !(e && e[0] && strcmp(e, "0") != 0)) {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_DEDUP_DEVICE=1 de-duplicates the regions of the device driver: it needs BMH_REGS_DEVICE=1\n");
		exit(1);
	}
}

/* BMH_PESTAT_DEVICE=1 takes mem_pestat's pair walk from the kernel behind the device's de-duplication, so it means nothing without
 * BMH_REGS_DEVICE=1 and BMH_DEDUP_DEVICE=1.  Checked like the two above. */
__attribute__((constructor)) static void qa_check_pestat_device_env(void)
{
	const char *p = getenv("BMH_PESTAT_DEVICE"), *d = getenv("BMH_DEDUP_DEVICE"), *e = getenv("BMH_REGS_DEVICE");
	if (p && p[0] && strcmp(p, "0") != 0 && !(d && d[0] && strcmp(d, "0") != 0 && e && e[0] && strcmp(e, "0") != 0)) {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_PESTAT_DEVICE=1 collects insert-size candidates behind the device's de-duplication: it needs BMH_REGS_DEVICE=1 and BMH_DEDUP_DEVICE=1\n");
		exit(1);
	}
}

/* BMH_MATESW_DEVICE=1 rescues mates against the reference resident on the device, so BMH_PAC_RESIDENT=0 contradicts it as well.
 * Checked like the two above; it does not depend on BMH_REGS_DEVICE. */
__attribute__((constructor)) static void qa_check_matesw_device_env(void)
{
	const char *e = getenv("BMH_MATESW_DEVICE"), *r = getenv("BMH_PAC_RESIDENT");
	if (e && e[0] && strcmp(e, "0") != 0 && r && r[0] == '0') {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_MATESW_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n");
		exit(1);
	}
}

/* BMH_MATESW_DEVICE=1: the mate-rescue driver as kernels (bmh_matesw_device), mem_sort_and_dedup included: no host callback */
static int qa_matesw_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_MATESW_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}

/* BMH_DECIDE_DEVICE=1: phase 2's pass A (primary marking, pairing, mapQ, the selection of what gets printed) on the device
 * (bmh_ctx_set_decide_device on every pooled context phase 2 uses).  Independent of the other device switches; needs no resident
 * reference. */
static int qa_decide_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_DECIDE_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}
static long long g_decide_cnt[2]; /* reads or pairs decided on the device, slices that fell back to the host */

/* BMH_WANTED_DEVICE=1: phase 2's pass B planned on the device (bmh_ctx_set_wanted_device on every pooled context phase 2 uses,
 * with the sequence table made resident where the reference is).  It aligns against the resident reference, so BMH_PAC_RESIDENT=0
 * contradicts it: checked when the library is loaded, like BMH_MATESW_DEVICE. */
__attribute__((constructor)) static void qa_check_wanted_device_env(void)
{
	const char *e = getenv("BMH_WANTED_DEVICE"), *r = getenv("BMH_PAC_RESIDENT");
	if (e && e[0] && strcmp(e, "0") != 0 && r && r[0] == '0') {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_WANTED_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n");
		exit(1);
	}
}
static int qa_wanted_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_WANTED_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}
static long long g_wanted_cnt[3]; /* regions planned on the device, fixed, redone on the host */

/* BMH_REGION_LONG=1: the regions whose CIGAR or MD outgrow the region record's slots are finished on the device
 * (bmh_ctx_set_region_long on every pooled context phase 2 uses) instead of being redone with host copies.  The region record
 * aligns against the resident reference, so BMH_PAC_RESIDENT=0 contradicts it: checked when the library is loaded, like its siblings. */
__attribute__((constructor)) static void qa_check_region_long_env(void)
{
	const char *e = getenv("BMH_REGION_LONG"), *r = getenv("BMH_PAC_RESIDENT");
	if (e && e[0] && strcmp(e, "0") != 0 && r && r[0] == '0') {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_REGION_LONG=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n");
		exit(1);
	}
}
static int qa_region_long(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_REGION_LONG");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}
void bmh_reg2cigar_totals_(long long *long_device, long long *redone_host); /* host/reg2cigar_batch.c */

/* BMH_PHASE2_DEVICE=1: phase 2's pass A and pass B as one device session (bmh_ctx_set_phase2_device on every pooled context phase 2
 * uses, with the sequence table made resident where the reference is).  It needs the resident reference as BMH_WANTED_DEVICE does:
 * checked when the library is loaded. */
__attribute__((constructor)) static void qa_check_phase2_device_env(void)
{
	const char *e = getenv("BMH_PHASE2_DEVICE"), *r = getenv("BMH_PAC_RESIDENT");
	if (e && e[0] && strcmp(e, "0") != 0 && r && r[0] == '0') {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_PHASE2_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n");
		exit(1);
	}
}
static int qa_phase2_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_PHASE2_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}
static long long g_phase2_cnt[5]; /* units, regions, fixed, redone on the host, slices that fell back to the two passes */

/* BMH_PHASE2_TEXT_DEVICE=1: phase 2's three passes as one device session (bmh_ctx_set_phase2_text_device on every pooled context phase 2
 * uses, with the sequence table and the names made resident where the reference is).  It needs the resident reference as
 * BMH_PHASE2_DEVICE does: checked when the library is loaded. */
__attribute__((constructor)) static void qa_check_phase2_text_device_env(void)
{
	const char *e = getenv("BMH_PHASE2_TEXT_DEVICE"), *r = getenv("BMH_PAC_RESIDENT");
	if (e && e[0] && strcmp(e, "0") != 0 && r && r[0] == '0') {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_PHASE2_TEXT_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n");
		exit(1);
	}
}
static int qa_phase2_text_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_PHASE2_TEXT_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}
static long long g_phase2_text_cnt[6]; /* units, regions, redone on the host, lines, bytes of text, slices that fell back to the other routes */

/* BMH_READS_SAM_DEVICE=1: a single-end chunk's batches go from bases to SAM text in one device session each (bmh_reads_sam_device:
 * mem_process_seqs below).  Its phase 1 extends from the resident reference and its phase 2 aligns against it, so BMH_PAC_RESIDENT=0
 * contradicts it: checked when the library is loaded, like its siblings.  It needs and consults no other switch. */
__attribute__((constructor)) static void qa_check_reads_sam_device_env(void)
{
	const char *e = getenv("BMH_READS_SAM_DEVICE"), *r = getenv("BMH_PAC_RESIDENT");
	if (e && e[0] && strcmp(e, "0") != 0 && r && r[0] == '0') {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_READS_SAM_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n");
		exit(1);
	}
}
static int qa_reads_sam_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_READS_SAM_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}
static long long g_reads_sam_cnt[6]; /* batches, reads, regions behind the de-duplication, redone on the host, lines, bytes of text */

/* BMH_PAIRS_SAM_DEVICE=1: the same for a paired-end chunk (bmh_pairs_sam_begin / bmh_pairs_sam_finish around the chunk's insert-size
 * table, or bmh_pairs_sam_device under -I: mem_process_seqs below).  Independent of BMH_READS_SAM_DEVICE; the same contradiction. */
__attribute__((constructor)) static void qa_check_pairs_sam_device_env(void)
{
	const char *e = getenv("BMH_PAIRS_SAM_DEVICE"), *r = getenv("BMH_PAC_RESIDENT");
	if (e && e[0] && strcmp(e, "0") != 0 && r && r[0] == '0') {
		fprintf(stderr, "[bwamem_hip] fatal: BMH_PAIRS_SAM_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n");
		exit(1);
	}
}
static int qa_pairs_sam_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_PAIRS_SAM_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}
static long long g_pairs_sam_cnt[8]; /* batches, pairs, regions, regions after rescue, ksw_align2 calls, redone on the host, lines, bytes of text */
static long long g_pairs_sam_parked; /* bytes parked at the last chunk's barrier */

/* BMH_SAMTEXT_DEVICE=1: phase 2's pass C on the device (bmh_ctx_set_samtext_device on every pooled context phase 2 uses, with the
 * sequence table and the names made resident).  It reads no base of the reference, so it does not need BMH_PAC_RESIDENT. */
static int qa_samtext_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_SAMTEXT_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}
static long long g_samtext_cnt[3]; /* reads, lines, bytes of text */

/* BMH_REGS_DEVICE=1: seeding, chaining and the chains-to-regions driver in one device call (bmh_seed_chain_regs_batch) */
static int qa_regs_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_REGS_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0;
	}
	return on;
}

/* BMH_DEDUP_DEVICE=1 (with BMH_REGS_DEVICE=1): mem_sort_and_dedup behind the regions on the device (bmh_ctx_set_regs_dedup);
 * phase 1 then makes no host bmh_sort_and_dedup call */
static int qa_dedup_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_DEDUP_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0 && qa_regs_device();
	}
	return on;
}
static long long g_dedup_cnt[3]; /* regions de-duplicated on the device, regions kept, host bmh_sort_and_dedup calls of phase 1 */

/* BMH_PESTAT_DEVICE=1 (with the two above): mem_pestat's pair walk as a kernel behind the de-duplication (bmh_ctx_set_pestat_collect),
 * and under -e mem_test_and_remove_exact with it (bmh_ctx_set_regs_drop_exact); the chunk's serial section is then
 * bmh_pestat_from_candidates over a flat array of words */
static int qa_pestat_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_PESTAT_DEVICE");
		on = e && e[0] && strcmp(e, "0") != 0 && qa_dedup_device();
	}
	return on;
}
static long long g_pes_removed; /* this chunk: exact matches removed on the device */

/* BMH_CHAIN_DEVICE=1 (implied by BMH_REGS_DEVICE=1): chaining on the device, fused with seeding (bmh_seed_chain_batch); unset or 0:
 * bmh_chain_reads on the host */
static int qa_chain_device(void)
{
	static int on = -1;
	if (on < 0) {
		const char *e = getenv("BMH_CHAIN_DEVICE");
		on = (e && e[0] && strcmp(e, "0") != 0) || qa_regs_device();
	}
	return on;
}

/* (a static body behind both exported names: inside a process that also holds the reference's own definitions -- the tests load
 * libbwa_ref.so next to this library -- a call through the exported name would bind to whichever was loaded first) */
/* cand (nullable, with pso): the chunk's insert-size words; the batch starts at an even read, holds an even number of reads and
 * leaves the words of its pairs at cand[start / 2 ...] (BMH_PESTAT_DEVICE=1, mem_process_seqs below) */
static bmh_alnreg_v *align_batch(const ref_mem_opt_t *opt, const void *bwt, const ref_bntseq_head_t *bns,
                                 const uint8_t *pac, ref_bseq1_t *seqs, int start, int batch_size, uint32_t *cand, const bmh_sam_opt_t *pso)
{
	bmh_chain_v *chn = (bmh_chain_v *)malloc(sizeof(bmh_chain_v) * (size_t)batch_size);
	bmh_alnreg_v *regs = (bmh_alnreg_v *)calloc((size_t)batch_size, sizeof(bmh_alnreg_v));
	bmh_read_t *reads = (bmh_read_t *)malloc(sizeof(bmh_read_t) * (size_t)batch_size);
	bmh_params_t p;
	bmh_ctx_t *ctx;
	double tq[6];
	int b, i, rc;
	const int collect = cand != 0 && qa_regs_device();
	const int drop_dev = collect && (opt->flag & REF_MEM_F_NO_EXACT) != 0; /* mem_test_and_remove_exact behind the same kernel */

	for (b = 0; b < batch_size; ++b) { /* bwamem.c:1093-1094 */
		ref_bseq1_t *s = &seqs[start + b];
		for (i = 0; i < s->l_seq; ++i) s->seq[i] = s->seq[i] < 4 ? s->seq[i] : (char)nst_nt4_table[(int)s->seq[i]];
		reads[b].l_seq = s->l_seq, reads[b].seq = (const uint8_t *)s->seq;
	}
	memset(&p, 0, sizeof(p)); /* the hot-path fields of mem_opt_t */
	p.o_del = opt->o_del, p.e_del = opt->e_del, p.o_ins = opt->o_ins, p.e_ins = opt->e_ins, p.zdrop = opt->zdrop;
	p.a = opt->a, p.w = opt->w, p.pen_clip5 = opt->pen_clip5, p.pen_clip3 = opt->pen_clip3;
	memcpy(p.mat, opt->mat, 25);
	tq[0] = tq[1] = stage_now();
	ctx = bmh_pool_get(&p);
	if (qa_regs_device()) { /* bwamem.c:1095-1110 in one call: reads up, regions down */
		bmh_smem_opt_t so;
		bmh_chain_opt_t co;
		bmh_driver_stats_t st;
		bmh_chain_stats_t cs;
		/* (BMH_PAC_RESIDENT=0 was refused when the library was loaded) */
		if ((rc = bmh_ctx_set_pac(ctx, pac, bns->l_pac))) bmh_tls_die(bmh_last_error(ctx), rc);
		qa_seed_setup(ctx, opt, (const ref_bwt_t *)bwt, &so);
		qa_chain_opt(opt, &co);
		if ((rc = bmh_ctx_set_regs_dedup(ctx, qa_dedup_device(), opt->mask_level_redun))) bmh_tls_die(bmh_last_error(ctx), rc); /* bwamem.c:1114 behind the call */
		/* (contexts are pooled: both switches are set on every call, on or off) */
		if ((rc = bmh_ctx_set_pestat_collect(ctx, collect, pso)) || (rc = bmh_ctx_set_regs_drop_exact(ctx, drop_dev))) bmh_tls_die(bmh_last_error(ctx), rc);
		if ((rc = bmh_seed_chain_regs_batch(ctx, &so, &co, bns->l_pac, batch_size, reads, opt->min_seed_len, regs))) bmh_tls_die(bmh_last_error(ctx), rc);
		if (collect && (rc = bmh_last_pestat_candidates(ctx, cand + (start >> 1), batch_size >> 1, 0))) bmh_tls_die(bmh_last_error(ctx), rc);
		if (drop_dev) {
			int64_t gone = 0;
			bmh_last_drop_exact_stats(ctx, &gone);
			__sync_fetch_and_add(&g_pes_removed, (long long)gone);
		}
		if (qa_dedup_device()) {
			int64_t din = 0, dout = 0;
			bmh_last_dedup_stats(ctx, &din, &dout, 0);
			__sync_fetch_and_add(&g_dedup_cnt[0], (long long)din), __sync_fetch_and_add(&g_dedup_cnt[1], (long long)dout);
		}
		bmh_driver_stats(ctx, &st);
		bmh_chain_stats(ctx, &cs);
		bmh_pool_put(ctx);
		__sync_fetch_and_add(&g_p1_cnt[0], (long long)cs.chains_out);
		__sync_fetch_and_add(&g_p1_cnt[1], st.seeds_extended), __sync_fetch_and_add(&g_p1_cnt[2], st.seeds_speculated);
		__sync_fetch_and_add(&g_p1_cnt[3], st.short_sw);
		tq[2] = tq[3] = tq[4] = tq[5] = stage_now();
		__sync_fetch_and_add(&g_seedchain_us, (long long)((tq[2] - tq[1]) * 1e6));
		for (b = 0; b < batch_size; ++b) chn[b].n = chn[b].m = 0, chn[b].a = 0;
		goto folded;
	}
	if (qa_chain_device()) { /* mem_chain + mem_chain_flt (bwamem.c:1095-1097) on the device behind the seeding: only chains come back */
		bmh_smem_opt_t so;
		bmh_chain_opt_t co;
		qa_seed_setup(ctx, opt, (const ref_bwt_t *)bwt, &so);
		qa_chain_opt(opt, &co);
		if ((rc = bmh_seed_chain_batch(ctx, &so, &co, bns->l_pac, batch_size, reads, chn))) bmh_tls_die(bmh_last_error(ctx), rc);
		bmh_pool_put(ctx);
		tq[2] = tq[3] = stage_now();
		__sync_fetch_and_add(&g_seedchain_us, (long long)((tq[2] - tq[1]) * 1e6));
	} else {
		qa_seed_batch_begin(ctx, opt, (const ref_bwt_t *)bwt, batch_size, reads); /* SMEMs + suffix-array look-ups of the batch on the GPU */
		bmh_pool_put(ctx);
		tq[2] = stage_now();
		{ /* chaining: mem_chain + mem_chain_flt (bwamem.c:1095-1097) over the batch's tables */
			const qa_seed_t *S = qa_seed;
			bmh_chain_opt_t co;
			qa_chain_opt(opt, &co);
			if ((rc = bmh_chain_reads(&co, bns->l_pac, batch_size, reads, S->call_off, S->calls, S->intv_off, S->intv, S->sa_k, S->sa_pos, chn)))
				bmh_tls_die("the batch's seeding tables do not cover its chaining", rc);
		}
		qa_seed_batch_end();
		tq[3] = stage_now();
	}
	{
		long long nc = 0;
		for (b = 0; b < batch_size; ++b) nc += (long long)chn[b].n;
		__sync_fetch_and_add(&g_p1_cnt[0], nc);
	}
	tq[4] = stage_now();
	ctx = bmh_pool_get(&p);
	{ /* reference resident in HBM, shared by all contexts: the kernels do bns_get_seq themselves.  BMH_PAC_RESIDENT=0
	   * falls back to host-decoded windows in the pool. */
		const char *e = getenv("BMH_PAC_RESIDENT");
		if (!(e && e[0] == '0') && (rc = bmh_ctx_set_pac(ctx, pac, bns->l_pac))) bmh_tls_die(bmh_last_error(ctx), rc);
	}
	if ((rc = bmh_chains2regs_batch(ctx, bns->l_pac, pac, batch_size, reads, chn, opt->min_seed_len, regs))) /* bwamem.c:1101-1110 */
		bmh_tls_die(bmh_last_error(ctx), rc);
	{
		bmh_driver_stats_t st;
		bmh_driver_stats(ctx, &st);
		__sync_fetch_and_add(&g_p1_cnt[1], st.seeds_extended), __sync_fetch_and_add(&g_p1_cnt[2], st.seeds_speculated);
		__sync_fetch_and_add(&g_p1_cnt[3], st.short_sw);
	}
	bmh_pool_put(ctx);
	tq[5] = stage_now();
folded:
	{ /* thread-seconds per stage, summed over the run (BMH_VERBOSE prints them per chunk) */
		static const int a_[5] = {0, 1, 2, 3, 4};
		int k;
		for (k = 0; k < 5; ++k) {
			const double d = tq[a_[k] + 1] - tq[a_[k]];
			long long us = (long long)(d * 1e6);
			__sync_fetch_and_add(&g_p1_us[k], us);
		}
	}

	for (b = 0; b < batch_size; ++b) { /* host stages after the path: bwamem.c:1106,1112-1117 */
		for (i = 0; i < (int)chn[b].n; ++i) free(chn[b].a[i].seeds);
		free(chn[b].a);
		if (!qa_dedup_device()) { /* (BMH_DEDUP_DEVICE=1: the device call returned the survivors) */
			regs[b].n = (size_t)bmh_sort_and_dedup((int)regs[b].n, regs[b].a, opt->mask_level_redun); /* bwamem.c:1114 */
			__sync_fetch_and_add(&g_dedup_cnt[2], 1);
		}
		if (!drop_dev && (opt->flag & REF_MEM_F_NO_EXACT) && regs[b].n && regs[b].a[0].truesc == seqs[start + b].l_seq * opt->a) { /* mem_test_and_remove_exact, bwamem.c:438-443 */
			memmove(regs[b].a, regs[b].a + 1, (regs[b].n - 1) * sizeof(bmh_alnreg_t));
			--regs[b].n;
		}
	}
	free(chn);
	free(reads);
	return regs; /* caller copies and frees, bwamem.c:1272-1278 */
}

bmh_alnreg_v *mem_align1_core_batched(const ref_mem_opt_t *opt, const void *bwt, const ref_bntseq_head_t *bns,
                                      const uint8_t *pac, ref_bseq1_t *seqs, int start, int batch_size)
{
	return align_batch(opt, bwt, bns, pac, seqs, start, batch_size, 0, 0);
}

/* mem_align1_core() with the reference's exact signature (bwamem.c:1122-1149; used by mem_align1 :1151 and example.c:44): one
 * read through the same drivers as a batch of one -- `seq` is converted to base codes in place as at :1128-1129, the result
 * vector is malloc'd and the caller's (as kv_push would have left it).  A batch of one cannot fill a GPU; the entry point
 * exists so that library users of the reference's API get the same regions from the same code path. */
bmh_alnreg_v mem_align1_core(const ref_mem_opt_t *opt, const void *bwt, const ref_bntseq_head_t *bns, const uint8_t *pac, int l_seq, char *seq)
{
	ref_bseq1_t one;
	bmh_alnreg_v *v, out;
	memset(&one, 0, sizeof(one));
	one.l_seq = l_seq, one.seq = seq;
	v = align_batch(opt, bwt, bns, pac, &one, 0, 1, 0, 0);
	out = v[0];
	free(v);
	return out;
}

/* =====================================================================================================================
 * mem_process_seqs() with the reference's exact signature (bwamem.h:117, bwamem.c:1297-1327): the same three steps as
 * the reference -- phase 1 through the batching seam above, insert-size statistics, phase 2 -- every data-parallel part
 * of them as GPU batches and the host code between them the library's own:
 *   phase 1   mem_align1_core_batched above (seeding batch, chaining, bmh_chain2aln_batch, bmh_sort_and_dedup)
 *   pairs     bmh_pestat, then the whole chunk's mate rescue (bmh_matesw_batch, one slice per GPU place)
 *   phase 2   bmh_sam_batch per slice of the chunk: primary marking, pairing, the global alignments of exactly the
 *             regions that get printed (bmh_reg2cigar_batch), SAM text
 * Nothing of the reference's bwamem.c / bwamem_pair.c runs after chaining.
 */

#define REF_MEM_F_PE 0x2         /* bwamem.h:14 */
#define REF_MEM_F_NO_RESCUE 0x20 /* bwamem.h:18 */
#define REF_MEM_F_NOPAIRING 0x4  /* bwamem.h:15 */

extern void kt_for(int n_threads, void (*func)(void *, int, int), void *data, int n);                       /* kthread.c */
extern void kt_for_batch(int n_threads, void (*func)(void *, int, int, int), void *data, int n, int batch);  /* kthread_batch.c:44 */
extern int bwa_verbose;
extern char bwa_rg_id[256]; /* bwa.c:16 */

typedef struct {
	const ref_mem_opt_t *opt;
	const void *bwt;
	const ref_bntseq_head_t *bns;
	const uint8_t *pac;
	ref_bseq1_t *seqs;
	bmh_alnreg_v *regs;
	uint32_t *cand; /* BMH_PESTAT_DEVICE=1 and the chunk qualifies: its insert-size words, one per pair; else null */
	const bmh_sam_opt_t *sopt;
} qa_worker_t;

static void qa_worker1_batched(void *data, int start, int batch_size, int tid) /* == worker1_batched, bwamem.c:1264-1279 */
{
	qa_worker_t *w = (qa_worker_t *)data;
	bmh_alnreg_v *ret = align_batch(w->opt, w->bwt, w->bns, w->pac, w->seqs, start, batch_size, w->cand, w->sopt);
	int i;
	(void)tid;
	for (i = start; i < start + batch_size; ++i) w->regs[i] = ret[i - start];
	free(ret);
}

static long long g_msw_dedup_calls, g_msw_active; /* host callbacks of mate rescue; with BMH_MATESW_DEVICE=1: pairs that needed rescue */
static int qa_dedup(void *user, int n, bmh_alnreg_t *a) /* bmh_dedup_fn of the mate-rescue driver */
{
	__sync_fetch_and_add(&g_msw_dedup_calls, 1);
	return bmh_sort_and_dedup(n, a, ((const ref_mem_opt_t *)user)->mask_level_redun);
}

typedef struct {
	const ref_mem_opt_t *opt;
	const ref_bntseq_head_t *bns;
	const uint8_t *pac;
	int n, n_slices;
	int64_t n_processed;
	ref_bseq1_t *seqs;
	bmh_alnreg_v *regs;
	const bmh_read_t *reads;
	const bmh_params_t *params;
	const bmh_sam_opt_t *sopt;
	const bmh_pestat_t *pes;
	int resident;
} qa_slice_job_t;

static bmh_ctx_t *qa_slice_ctx(const qa_slice_job_t *J)
{
	bmh_ctx_t *ctx = bmh_pool_get(J->params);
	int rc;
	if (J->resident && (rc = bmh_ctx_set_pac(ctx, J->pac, J->bns->l_pac))) bmh_tls_die(bmh_last_error(ctx), rc);
	if ((rc = bmh_ctx_set_decide_device(ctx, qa_decide_device()))) bmh_tls_die(bmh_last_error(ctx), rc); /* per pooled context */
	if (qa_wanted_device() || qa_phase2_device()) { /* the sequence table where the reference is made resident; both stay */
		if (!J->resident)
			bmh_tls_die(qa_wanted_device() ? "BMH_WANTED_DEVICE=1 needs the reference resident on the device"
			                               : "BMH_PHASE2_DEVICE=1 needs the reference resident on the device", BMH_E_ARG);
		if ((rc = bmh_ctx_set_refidx(ctx, (const bmh_refidx_t *)J->bns))) bmh_tls_die(bmh_last_error(ctx), rc);
	}
	if ((rc = bmh_ctx_set_wanted_device(ctx, qa_wanted_device()))) bmh_tls_die(bmh_last_error(ctx), rc);
	if ((rc = bmh_ctx_set_region_long(ctx, qa_region_long()))) bmh_tls_die(bmh_last_error(ctx), rc);
	if ((rc = bmh_ctx_set_phase2_device(ctx, qa_phase2_device()))) bmh_tls_die(bmh_last_error(ctx), rc);
	if (qa_samtext_device() && ((rc = bmh_ctx_set_refidx(ctx, (const bmh_refidx_t *)J->bns)) || (rc = bmh_ctx_set_refnames(ctx, (const bmh_refidx_t *)J->bns))))
		bmh_tls_die(bmh_last_error(ctx), rc);
	if ((rc = bmh_ctx_set_samtext_device(ctx, qa_samtext_device()))) bmh_tls_die(bmh_last_error(ctx), rc);
	if (qa_phase2_text_device()) { /* the sequence table and the names where the reference is made resident */
		if (!J->resident) bmh_tls_die("BMH_PHASE2_TEXT_DEVICE=1 needs the reference resident on the device", BMH_E_ARG);
		if ((rc = bmh_ctx_set_refidx(ctx, (const bmh_refidx_t *)J->bns)) || (rc = bmh_ctx_set_refnames(ctx, (const bmh_refidx_t *)J->bns)))
			bmh_tls_die(bmh_last_error(ctx), rc);
	}
	if ((rc = bmh_ctx_set_phase2_text_device(ctx, qa_phase2_text_device()))) bmh_tls_die(bmh_last_error(ctx), rc);
	return ctx;
}

/* mate rescue, one slice of pairs per host thread */
static long long g_msw_calls, g_msw_rounds_max, g_msw_bytes;
static long long g_msw_us; /* thread-microseconds in the driver call, over the run (stage_now's clock) */
static void qa_matesw_slice(void *data, int k, int tid)
{
	double t0;
	const qa_slice_job_t *J = (const qa_slice_job_t *)data;
	const int np = J->n >> 1, lo = (int)((int64_t)np * k / J->n_slices), hi = (int)((int64_t)np * (k + 1) / J->n_slices);
	bmh_matesw_opt_t mo;
	bmh_driver_stats_t st;
	bmh_ctx_t *ctx;
	int rc;
	(void)tid;
	if (hi <= lo) return;
	ctx = qa_slice_ctx(J);
	mo.pen_unpaired = J->opt->pen_unpaired, mo.max_matesw = J->opt->max_matesw, mo.min_seed_len = J->opt->min_seed_len, mo.rsv = 0;
	t0 = stage_now();
	if (qa_matesw_device()) { /* (the reference is resident: BMH_PAC_RESIDENT=0 was refused when the library was loaded) */
		int *n_sw = (int *)calloc((size_t)(hi - lo), sizeof(int)), p, act = 0;
		if (!n_sw) bmh_tls_die("out of memory", BMH_E_NOMEM);
		if ((rc = bmh_matesw_device(ctx, J->bns->l_pac, hi - lo, J->reads + 2 * lo, J->regs + 2 * lo, J->pes, &mo, J->opt->mask_level_redun, n_sw)))
			bmh_tls_die(bmh_last_error(ctx), rc);
		for (p = 0; p < hi - lo; ++p) act += n_sw[p] > 0; /* pairs with at least one ksw_align2 call */
		free(n_sw);
		__sync_fetch_and_add(&g_msw_active, act);
	} else if ((rc = bmh_matesw_batch(ctx, J->bns->l_pac, J->pac, hi - lo, J->reads + 2 * lo, J->regs + 2 * lo, J->pes, &mo, qa_dedup,
	                                  (void *)J->opt, 0)))
		bmh_tls_die(bmh_last_error(ctx), rc);
	__sync_fetch_and_add(&g_msw_us, (long long)((stage_now() - t0) * 1e6));
	bmh_driver_stats(ctx, &st);
	bmh_pool_put(ctx);
	__sync_fetch_and_add(&g_msw_calls, st.ext_tasks), __sync_fetch_and_add(&g_msw_bytes, st.pool_bytes);
	if (st.rounds > g_msw_rounds_max) g_msw_rounds_max = st.rounds; /* (a benign race: statistics only) */
}

/* phase 2, one slice of reads (whole pairs) per host thread: worker2 of the reference (bwamem.c:1281-1295) */
static long long g_sam_us[2]; /* thread-microseconds: waiting for a GPU place, bmh_sam_batch */
static void qa_sam_slice(void *data, int k, int tid)
{
	const qa_slice_job_t *J = (const qa_slice_job_t *)data;
	const int unit = (J->sopt->flag & BMH_MEM_F_PE) ? 2 : 1, nu = J->n / unit;
	const int lo = unit * (int)((int64_t)nu * k / J->n_slices), hi = unit * (int)((int64_t)nu * (k + 1) / J->n_slices);
	bmh_ctx_t *ctx;
	double t0, t1, t2;
	int rc, i;
	(void)tid;
	if (hi <= lo) return;
	t0 = t1 = stage_now();
	ctx = qa_slice_ctx(J);
	if ((rc = bmh_sam_batch(ctx, J->sopt, (const bmh_refidx_t *)J->bns, J->pac, J->pes, J->n_processed + lo, hi - lo, (bmh_seq_t *)(J->seqs + lo),
	                        J->regs + lo, bwa_rg_id)))
		bmh_tls_die(rc == BMH_E_ARG ? "a region could not be turned into an alignment (the reference aborts here too, bwamem.c:1183-1186)" : bmh_last_error(ctx), rc);
	if (qa_decide_device()) {
		int64_t du = 0, df = 0;
		bmh_last_decide_stats(ctx, &du, &df, 0);
		__sync_fetch_and_add(&g_decide_cnt[0], (long long)(du > 0 ? du : 0)), __sync_fetch_and_add(&g_decide_cnt[1], (long long)df);
	}
	if (qa_wanted_device()) {
		int64_t ww = 0, wf = 0, wr = 0;
		bmh_last_wanted_stats(ctx, &ww, &wf, &wr, 0);
		__sync_fetch_and_add(&g_wanted_cnt[0], (long long)(ww > 0 ? ww : 0)), __sync_fetch_and_add(&g_wanted_cnt[1], (long long)(wf > 0 ? wf : 0));
		__sync_fetch_and_add(&g_wanted_cnt[2], (long long)(wr > 0 ? wr : 0));
	}
	if (qa_phase2_device()) {
		bmh_phase2_stats_t ps;
		bmh_last_phase2_stats(ctx, &ps);
		__sync_fetch_and_add(&g_phase2_cnt[0], (long long)(ps.units > 0 ? ps.units : 0)), __sync_fetch_and_add(&g_phase2_cnt[1], (long long)(ps.wanted > 0 ? ps.wanted : 0));
		__sync_fetch_and_add(&g_phase2_cnt[2], (long long)(ps.fixed > 0 ? ps.fixed : 0)), __sync_fetch_and_add(&g_phase2_cnt[3], (long long)(ps.redone > 0 ? ps.redone : 0));
		__sync_fetch_and_add(&g_phase2_cnt[4], (long long)(ps.fallbacks > 0 ? ps.fallbacks : 0));
	}
	if (qa_samtext_device()) {
		bmh_samtext_stats_t ts;
		bmh_last_samtext_stats(ctx, &ts);
		__sync_fetch_and_add(&g_samtext_cnt[0], (long long)(ts.reads > 0 ? ts.reads : 0)), __sync_fetch_and_add(&g_samtext_cnt[1], (long long)(ts.lines > 0 ? ts.lines : 0));
		__sync_fetch_and_add(&g_samtext_cnt[2], (long long)(ts.text_bytes > 0 ? ts.text_bytes : 0));
	}
	if (qa_phase2_text_device()) {
		bmh_phase2_text_stats_t ps;
		int c;
		bmh_last_phase2_text_stats(ctx, &ps);
		{
			const int64_t got[6] = {ps.units, ps.wanted, ps.redone, ps.lines, ps.text_bytes, ps.fallbacks};
			for (c = 0; c < 6; ++c) __sync_fetch_and_add(&g_phase2_text_cnt[c], (long long)(got[c] > 0 ? got[c] : 0));
		}
	}
	bmh_pool_put(ctx);
	t2 = stage_now();
	for (i = lo; i < hi; ++i) free(J->regs[i].a);
	__sync_fetch_and_add(&g_sam_us[0], (long long)((t1 - t0) * 1e6)), __sync_fetch_and_add(&g_sam_us[1], (long long)((t2 - t1) * 1e6));
}

/* host threads of a phase: the program's -t unless the named variable says otherwise (a thread that waits for the GPU
 * sleeps, so more threads than cores can pay) */
static int qa_threads(const char *var, int dflt)
{
	const char *e = getenv(var);
	const int v = e ? atoi(e) : 0;
	return v > 0 ? v : dflt > 0 ? dflt : 1;
}

/* the fields of mem_opt_t phase 2 (and mem_pestat's pair walk in phase 1) reads */
static void qa_sam_opt(const ref_mem_opt_t *opt, bmh_sam_opt_t *so)
{
	memset(so, 0, sizeof(*so));
	so->a = opt->a, so->b = opt->b, so->o_del = opt->o_del, so->e_del = opt->e_del, so->o_ins = opt->o_ins, so->e_ins = opt->e_ins;
	so->pen_unpaired = opt->pen_unpaired, so->w = opt->w, so->T = opt->T, so->flag = opt->flag, so->min_seed_len = opt->min_seed_len;
	so->max_ins = opt->max_ins, so->mapQ_coef_fac = opt->mapQ_coef_fac, so->max_matesw = opt->max_matesw, so->mask_level = opt->mask_level;
	so->mask_level_redun = opt->mask_level_redun, so->mapQ_coef_len = opt->mapQ_coef_len;
	memcpy(so->mat, opt->mat, 25);
}

/* the hot-path fields of mem_opt_t */
static void qa_params(const ref_mem_opt_t *opt, bmh_params_t *p)
{
	memset(p, 0, sizeof(*p));
	p->o_del = opt->o_del, p->e_del = opt->e_del, p->o_ins = opt->o_ins, p->e_ins = opt->e_ins, p->zdrop = opt->zdrop;
	p->a = opt->a, p->w = opt->w, p->pen_clip5 = opt->pen_clip5, p->pen_clip3 = opt->pen_clip3;
	memcpy(p->mat, opt->mat, 25);
}

/* bwamem.c:1313's batch size, evened out over a chunk of n reads run by nt threads: -b 65536 cuts a chunk of 1 066 668 reads into 16
 * batches and a 17th of 18 092 that one thread runs alone after all others are done; the same reads in 16 batches of 66 667 are not a
 * read slower per batch.  As many batches as -b asks for, rounded to a multiple of the thread count, at least 4 096 reads each.
 * BMH_BATCH_EXACT=1 keeps -b to the read. */
static int qa_even_batch(const ref_mem_opt_t *opt, int n, int nt)
{
	int b = opt->batch_size > 0 ? opt->batch_size : 1;
	if (!getenv("BMH_BATCH_EXACT") && n > 0) {
		int64_t rounds = ((int64_t)n + (int64_t)b * nt / 2) / ((int64_t)b * nt), nb;
		if (rounds < 1) rounds = 1;
		nb = rounds * nt;
		if ((int64_t)n / nb < 4096) nb = ((int64_t)n + 4095) / 4096;
		b = (int)(((int64_t)n + nb - 1) / nb);
	}
	return b;
}

/* ---- BMH_READS_SAM_DEVICE=1, a single-end chunk: one job per batch, from the batch's bases to its reads' SAM strings.  Nothing of a
 * chunk is serial without insert-size statistics, so the jobs share nothing and wait for nothing but the device: no region vector, no
 * second upload of regions, no barrier between "all of phase 1" and "all of phase 2". */
typedef struct {
	const ref_mem_opt_t *opt;
	const void *bwt;
	const ref_bntseq_head_t *bns;
	const uint8_t *pac;
	int64_t n_processed;
	int n, batch;
	ref_bseq1_t *seqs;
	const bmh_params_t *params;
	const bmh_sam_opt_t *sopt;
} qa_reads_sam_job_t;

/* a batch's text into its reads' strings (both one-session routes); the text and its offsets are freed */
static void qa_text_to_strings(int n, ref_bseq1_t *seqs, char *text, int64_t *text_off)
{
	const int rc = bmh_sam_cut(n, (bmh_seq_t *)seqs, text, text_off);
	if (rc) bmh_tls_die("the batch's SAM text could not be cut into strings", rc);
	free(text), free(text_off);
}

static void qa_reads_sam_batch(void *data, int k, int tid)
{
	const qa_reads_sam_job_t *J = (const qa_reads_sam_job_t *)data;
	const int64_t lo64 = (int64_t)k * J->batch, hi64 = lo64 + J->batch < J->n ? lo64 + J->batch : J->n;
	const int lo = (int)lo64, hi = (int)hi64;
	bmh_smem_opt_t so;
	bmh_chain_opt_t co;
	bmh_reads_sam_stats_t rs;
	bmh_phase2_text_stats_t ps;
	bmh_ctx_t *ctx;
	int64_t *text_off;
	char *text = 0;
	int b, i, rc;
	(void)tid;
	if (hi <= lo) return;
	for (b = lo; b < hi; ++b) { /* bwamem.c:1093-1094 */
		ref_bseq1_t *s = &J->seqs[b];
		for (i = 0; i < s->l_seq; ++i) s->seq[i] = s->seq[i] < 4 ? s->seq[i] : (char)nst_nt4_table[(int)s->seq[i]];
	}
	if (!(text_off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)(hi - lo) + 1)))) bmh_tls_die("out of memory for the batch's text offsets", BMH_E_NOMEM);
	ctx = bmh_pool_get(J->params);
	/* what the call needs resident (BMH_PAC_RESIDENT=0 was refused when the library was loaded); contexts are pooled, so every job says it */
	if ((rc = bmh_ctx_set_pac(ctx, J->pac, J->bns->l_pac))) bmh_tls_die(bmh_last_error(ctx), rc);
	qa_seed_setup(ctx, J->opt, (const ref_bwt_t *)J->bwt, &so);
	qa_chain_opt(J->opt, &co);
	if ((rc = bmh_ctx_set_refidx(ctx, (const bmh_refidx_t *)J->bns)) || (rc = bmh_ctx_set_refnames(ctx, (const bmh_refidx_t *)J->bns)) ||
	    (rc = bmh_ctx_set_region_long(ctx, qa_region_long())))
		bmh_tls_die(bmh_last_error(ctx), rc);
	if ((rc = bmh_reads_sam_device(ctx, &so, &co, J->opt->min_seed_len, J->sopt, (const bmh_refidx_t *)J->bns, J->pac, J->n_processed + lo, hi - lo,
	                               (bmh_seq_t *)(J->seqs + lo), bwa_rg_id, &text, text_off)))
		bmh_tls_die(bmh_last_error(ctx), rc); /* no other route for the batch */
	bmh_last_reads_sam_stats(ctx, &rs);
	bmh_last_phase2_text_stats(ctx, &ps);
	bmh_pool_put(ctx);
	qa_text_to_strings(hi - lo, J->seqs + lo, text, text_off);
	{
		const int64_t got[6] = {1, rs.reads, rs.regions, ps.redone, ps.lines, ps.text_bytes};
		int c;
		for (c = 0; c < 6; ++c) __sync_fetch_and_add(&g_reads_sam_cnt[c], (long long)(got[c] > 0 ? got[c] : 0));
	}
}

static void qa_reads_sam_chunk(const ref_mem_opt_t *opt, const void *bwt, const ref_bntseq_head_t *bns, const uint8_t *pac, int64_t n_processed, int n,
                               ref_bseq1_t *seqs)
{
	/* A thread inside the call sleeps on several waits per batch, so half again as many threads as -t pay here as they do in phase 2
	 * (measured at -t 16 on 2.4 M reads of 150 bases, from the second chunk on: 2.39 M reads/s with 16 threads, 2.46 M with 24, 2.20 M
	 * with 32; the process 4.03, 3.28 and 3.81 s: profiles/reads_sam_shim.md).  The pre-warming makes that many contexts. */
	const int nt = qa_threads("BMH_RS_THREADS", opt->n_threads + opt->n_threads / 2);
	const double t0 = realtime();
	qa_reads_sam_job_t J;
	bmh_params_t p;
	bmh_sam_opt_t so;
	qa_sam_opt(opt, &so);
	qa_params(opt, &p);
	J.opt = opt, J.bwt = bwt, J.bns = bns, J.pac = pac, J.n_processed = n_processed, J.n = n, J.seqs = seqs, J.params = &p, J.sopt = &so;
	J.batch = qa_even_batch(opt, n, nt);
	kt_for(nt, qa_reads_sam_batch, &J, (int)(((int64_t)n + J.batch - 1) / J.batch));
	if (getenv("BMH_VERBOSE")) {
		fprintf(stderr, "[bwamem_hip] single-end reads to SAM text in one session so far: %lld batches, %lld reads, %lld regions, %lld redone on the host, %lld lines, %lld bytes\n",
		        g_reads_sam_cnt[0], g_reads_sam_cnt[1], g_reads_sam_cnt[2], g_reads_sam_cnt[3], g_reads_sam_cnt[4], g_reads_sam_cnt[5]);
		fprintf(stderr, "[bwamem_hip] chunk of %d reads: reads to SAM text in one session %.3f s\n", n, realtime() - t0);
	}
}

/* ---- BMH_PAIRS_SAM_DEVICE=1, a paired-end chunk: the same, with the insert-size barrier in the middle.  The table is the whole chunk's
 * (bwamem.c:1314-1317), so every batch's words must be down before the first batch's mate rescue: pass 1 runs bmh_pairs_sam_begin per
 * batch, which parks the batch's region table and bases in a device block of its own; one bmh_pestat_from_candidates makes the table;
 * pass 2 runs bmh_pairs_sam_finish per batch on whatever context the pool hands out.  With the table given (-I) there is no barrier:
 * one pass of bmh_pairs_sam_device per batch, nothing parked. */
typedef struct {
	const ref_mem_opt_t *opt;
	const void *bwt;
	const ref_bntseq_head_t *bns;
	const uint8_t *pac;
	int64_t n_processed;
	int n, batch; /* batch: even */
	ref_bseq1_t *seqs;
	const bmh_params_t *params;
	const bmh_sam_opt_t *sopt;
	const bmh_pestat_t *pes;      /* pass 2: the chunk's table; the one-pass form: the caller's */
	uint32_t *cand;               /* pass 1: n / 2 words */
	bmh_pairs_parked_t **parked;  /* one per batch, from pass 1 to pass 2 */
} qa_pairs_sam_job_t;

static bmh_ctx_t *qa_pairs_sam_ctx(const qa_pairs_sam_job_t *J, bmh_smem_opt_t *so, bmh_chain_opt_t *co)
{
	bmh_ctx_t *ctx = bmh_pool_get(J->params);
	int rc;
	/* what the calls need resident (BMH_PAC_RESIDENT=0 was refused when the library was loaded); contexts are pooled, so every job says it */
	if ((rc = bmh_ctx_set_pac(ctx, J->pac, J->bns->l_pac))) bmh_tls_die(bmh_last_error(ctx), rc);
	qa_seed_setup(ctx, J->opt, (const ref_bwt_t *)J->bwt, so);
	qa_chain_opt(J->opt, co);
	if ((rc = bmh_ctx_set_refidx(ctx, (const bmh_refidx_t *)J->bns)) || (rc = bmh_ctx_set_refnames(ctx, (const bmh_refidx_t *)J->bns)) ||
	    (rc = bmh_ctx_set_region_long(ctx, qa_region_long())))
		bmh_tls_die(bmh_last_error(ctx), rc);
	return ctx;
}

static void qa_pairs_sam_bounds(const qa_pairs_sam_job_t *J, int k, int *lo, int *hi)
{
	const int64_t lo64 = (int64_t)k * J->batch, hi64 = lo64 + J->batch < J->n ? lo64 + J->batch : J->n;
	*lo = (int)lo64, *hi = (int)hi64;
}

static void qa_pairs_sam_codes(const qa_pairs_sam_job_t *J, int lo, int hi)
{
	int b, i;
	for (b = lo; b < hi; ++b) { /* bwamem.c:1093-1094 */
		ref_bseq1_t *s = &J->seqs[b];
		for (i = 0; i < s->l_seq; ++i) s->seq[i] = s->seq[i] < 4 ? s->seq[i] : (char)nst_nt4_table[(int)s->seq[i]];
	}
}

/* a finished batch: its text into the reads' strings, its numbers into the run's */
static void qa_pairs_sam_done(const qa_pairs_sam_job_t *J, bmh_ctx_t *ctx, int lo, int hi, char *text, int64_t *text_off)
{
	bmh_pairs_sam_stats_t ps;
	bmh_phase2_text_stats_t pt;
	int c;
	bmh_last_pairs_sam_stats(ctx, &ps);
	bmh_last_phase2_text_stats(ctx, &pt);
	bmh_pool_put(ctx);
	qa_text_to_strings(hi - lo, J->seqs + lo, text, text_off);
	{
		const int64_t got[8] = {1, ps.pairs, ps.regions, ps.regions_out, ps.n_sw, pt.redone, pt.lines, pt.text_bytes};
		for (c = 0; c < 8; ++c) __sync_fetch_and_add(&g_pairs_sam_cnt[c], (long long)(got[c] > 0 ? got[c] : 0));
	}
}

static void qa_pairs_sam_pass1(void *data, int k, int tid)
{
	const qa_pairs_sam_job_t *J = (const qa_pairs_sam_job_t *)data;
	bmh_smem_opt_t so;
	bmh_chain_opt_t co;
	bmh_pairs_parked_info_t info;
	bmh_ctx_t *ctx;
	int lo, hi, rc;
	(void)tid;
	qa_pairs_sam_bounds(J, k, &lo, &hi);
	if (hi <= lo) return;
	qa_pairs_sam_codes(J, lo, hi);
	ctx = qa_pairs_sam_ctx(J, &so, &co);
	if ((rc = bmh_pairs_sam_begin(ctx, &so, &co, J->opt->min_seed_len, J->sopt, (const bmh_refidx_t *)J->bns, hi - lo, (bmh_seq_t *)(J->seqs + lo),
	                              J->cand + (lo >> 1), &J->parked[k])))
		bmh_tls_die(bmh_last_error(ctx), rc); /* no other route for the batch */
	bmh_pool_put(ctx);
	if (bmh_pairs_parked_info(J->parked[k], &info) == BMH_OK) __sync_fetch_and_add(&g_pairs_sam_parked, (long long)info.bytes);
}

static void qa_pairs_sam_pass2(void *data, int k, int tid)
{
	const qa_pairs_sam_job_t *J = (const qa_pairs_sam_job_t *)data;
	bmh_smem_opt_t so;
	bmh_chain_opt_t co;
	bmh_matesw_opt_t mo;
	bmh_ctx_t *ctx;
	int64_t *text_off;
	char *text = 0;
	int lo, hi, rc;
	(void)tid;
	qa_pairs_sam_bounds(J, k, &lo, &hi);
	if (hi <= lo) return;
	if (!(text_off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)(hi - lo) + 1)))) bmh_tls_die("out of memory for the batch's text offsets", BMH_E_NOMEM);
	ctx = qa_pairs_sam_ctx(J, &so, &co);
	mo.pen_unpaired = J->opt->pen_unpaired, mo.max_matesw = J->opt->max_matesw, mo.min_seed_len = J->opt->min_seed_len, mo.rsv = 0;
	if ((rc = bmh_pairs_sam_finish(ctx, J->parked[k], &mo, J->sopt, (const bmh_refidx_t *)J->bns, J->pac, J->pes, J->n_processed + lo, hi - lo,
	                               (bmh_seq_t *)(J->seqs + lo), bwa_rg_id, &text, text_off)))
		bmh_tls_die(bmh_last_error(ctx), rc);
	J->parked[k] = 0; /* consumed */
	qa_pairs_sam_done(J, ctx, lo, hi, text, text_off);
}

static void qa_pairs_sam_one(void *data, int k, int tid)
{
	const qa_pairs_sam_job_t *J = (const qa_pairs_sam_job_t *)data;
	bmh_smem_opt_t so;
	bmh_chain_opt_t co;
	bmh_matesw_opt_t mo;
	bmh_ctx_t *ctx;
	int64_t *text_off;
	char *text = 0;
	int lo, hi, rc;
	(void)tid;
	qa_pairs_sam_bounds(J, k, &lo, &hi);
	if (hi <= lo) return;
	qa_pairs_sam_codes(J, lo, hi);
	if (!(text_off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)(hi - lo) + 1)))) bmh_tls_die("out of memory for the batch's text offsets", BMH_E_NOMEM);
	ctx = qa_pairs_sam_ctx(J, &so, &co);
	mo.pen_unpaired = J->opt->pen_unpaired, mo.max_matesw = J->opt->max_matesw, mo.min_seed_len = J->opt->min_seed_len, mo.rsv = 0;
	if ((rc = bmh_pairs_sam_device(ctx, &so, &co, J->opt->min_seed_len, &mo, J->sopt, (const bmh_refidx_t *)J->bns, J->pac, J->pes, 0, J->n_processed + lo,
	                               hi - lo, (bmh_seq_t *)(J->seqs + lo), bwa_rg_id, &text, text_off)))
		bmh_tls_die(bmh_last_error(ctx), rc);
	qa_pairs_sam_done(J, ctx, lo, hi, text, text_off);
}

/* why a paired-end chunk keeps the default route with the switch on, or null.  A parked block is bound to its device and the pool does
 * not pick contexts by device, so a run spread over several GPUs keeps it too. */
static const char *qa_pairs_sam_off(const ref_mem_opt_t *opt, int n, const bmh_pestat_t *pes0)
{
	const char *list = getenv("BMH_DEVICES");
	if (opt->flag & REF_MEM_F_NOPAIRING) return "-P: no pairing";
	if (opt->flag & REF_MEM_F_NO_RESCUE) return "-S: the session always runs mate rescue";
	if (n < 2) return "no pair";
	if (n & 1) return "an odd number of reads";
	if (getenv("BMH_BATCH_EXACT") && ((opt->batch_size > 0 ? opt->batch_size : 1) & 1)) return "BMH_BATCH_EXACT=1 with an odd batch size";
	if (!pes0 && opt->max_ins >= (1 << 30)) return "max_ins >= 2^30";
	if (list && *list) { /* distinct ordinals */
		long first = -1;
		const char *p = list;
		while (*p) {
			char *end;
			const long v = strtol(p, &end, 10);
			if (end == p) break;
			if (first < 0) first = v;
			else if (v != first) return "more than one device in BMH_DEVICES";
			if (*end != ',') break;
			p = end + 1;
		}
	}
	return 0;
}

static void qa_pairs_sam_chunk(const ref_mem_opt_t *opt, const void *bwt, const ref_bntseq_head_t *bns, const uint8_t *pac, int64_t n_processed, int n,
                               ref_bseq1_t *seqs, const bmh_pestat_t *pes0)
{
	/* threads as in the single-end route: a thread inside either call sleeps on several waits per batch */
	const int nt = qa_threads("BMH_PS_THREADS", opt->n_threads + opt->n_threads / 2);
	double t_[4];
	qa_pairs_sam_job_t J;
	bmh_pestat_t pes[4];
	bmh_params_t p;
	bmh_sam_opt_t so;
	int nb;
	t_[0] = realtime();
	qa_sam_opt(opt, &so);
	qa_params(opt, &p);
	J.opt = opt, J.bwt = bwt, J.bns = bns, J.pac = pac, J.n_processed = n_processed, J.n = n, J.seqs = seqs, J.params = &p, J.sopt = &so;
	J.batch = qa_even_batch(opt, n, nt);
	J.batch += J.batch & 1; /* no pair straddles two batches */
	J.pes = pes0, J.cand = 0, J.parked = 0;
	nb = (int)(((int64_t)n + J.batch - 1) / J.batch);
	g_pairs_sam_parked = 0;
	if (pes0) {
		kt_for(nt, qa_pairs_sam_one, &J, nb);
		t_[1] = t_[2] = t_[3] = realtime();
	} else {
		int rc;
		J.cand = (uint32_t *)calloc((size_t)(n >> 1), sizeof(uint32_t));
		J.parked = (bmh_pairs_parked_t **)calloc((size_t)nb, sizeof(bmh_pairs_parked_t *));
		if (!J.cand || !J.parked) bmh_tls_die("out of memory for the insert-size words", BMH_E_NOMEM);
		kt_for(nt, qa_pairs_sam_pass1, &J, nb);
		t_[1] = realtime();
		if ((rc = bmh_pestat_from_candidates(&so, n >> 1, J.cand, pes, bwa_verbose))) bmh_tls_die("the device's insert-size words are inconsistent", rc);
		J.pes = pes;
		t_[2] = realtime();
		kt_for(nt, qa_pairs_sam_pass2, &J, nb);
		t_[3] = realtime();
		free(J.cand), free(J.parked);
	}
	if (getenv("BMH_VERBOSE")) {
		fprintf(stderr, "[bwamem_hip] paired-end reads to SAM text in one session so far: %lld batches, %lld pairs, %lld regions, %lld after rescue, %lld ksw_align2 calls, "
		        "%lld redone on the host, %lld lines, %lld bytes, %lld bytes parked at the barrier\n",
		        g_pairs_sam_cnt[0], g_pairs_sam_cnt[1], g_pairs_sam_cnt[2], g_pairs_sam_cnt[3], g_pairs_sam_cnt[4], g_pairs_sam_cnt[5], g_pairs_sam_cnt[6],
		        g_pairs_sam_cnt[7], g_pairs_sam_parked);
		if (pes0)
			fprintf(stderr, "[bwamem_hip] chunk of %d reads: pairs to SAM text in one session per batch under the given table, %d batches of up to %d reads, %.3f s\n", n, nb,
			        J.batch, t_[1] - t_[0]);
		else
			fprintf(stderr, "[bwamem_hip] chunk of %d reads: pairs to SAM text in parked sessions, %d batches of up to %d reads: pass 1 %.3f s, table %.3f s, pass 2 %.3f s\n", n,
			        nb, J.batch, t_[1] - t_[0], t_[2] - t_[1], t_[3] - t_[2]);
	}
}

void mem_process_seqs(const ref_mem_opt_t *opt, const void *bwt, const ref_bntseq_head_t *bns, const uint8_t *pac,
                      int64_t n_processed, int n, ref_bseq1_t *seqs, const bmh_pestat_t *pes0)
{
	const int pe = (opt->flag & REF_MEM_F_PE) != 0;
	const int rescue = pe && !(opt->flag & REF_MEM_F_NO_RESCUE);
	qa_worker_t w;
	bmh_pestat_t pes[4];
	bmh_params_t p;
	bmh_sam_opt_t so;
	bmh_read_t *reads;
	qa_slice_job_t J;
	double ctime, rtime, t_[4], t_pes;
	const char *why_host = 0; /* BMH_PESTAT_DEVICE=1: why this chunk keeps the host's bmh_pestat, or null */
	int i, nt2, n_host_pestat = 0, p1_batch[2] = {0, 0}; /* phase 1's batch size: as evened out, and as run */
	ctime = cputime(), rtime = realtime();
	t_[0] = rtime;
	if (n_processed == 0 && g_t_loaded > 0 && getenv("BMH_VERBOSE"))
		fprintf(stderr, "[bwamem_hip] the first chunk starts %.3f s after the shim was loaded\n", rtime - g_t_loaded);
	if (qa_reads_sam_device()) { /* a single-end chunk: bases to SAM strings, one device session per batch; nothing below runs */
		if (!pe) {
			qa_reads_sam_chunk(opt, bwt, bns, pac, n_processed, n, seqs);
			goto processed;
		}
		if (getenv("BMH_VERBOSE")) fprintf(stderr, "[bwamem_hip] single-end reads to SAM text in one session: off for this chunk (paired-end reads)\n");
	}
	if (qa_pairs_sam_device()) { /* a paired-end chunk: bases to SAM strings, the sessions parked at the insert-size barrier; nothing below runs */
		const char *why_off = pe ? qa_pairs_sam_off(opt, n, pes0) : "single-end reads";
		if (!why_off) {
			qa_pairs_sam_chunk(opt, bwt, bns, pac, n_processed, n, seqs, pes0);
			goto processed;
		}
		if (getenv("BMH_VERBOSE")) fprintf(stderr, "[bwamem_hip] paired-end reads to SAM text in one session: off for this chunk (%s)\n", why_off);
	}
	w.opt = opt, w.bwt = bwt, w.bns = bns, w.pac = pac, w.seqs = seqs;
	w.regs = (bmh_alnreg_v *)malloc((size_t)n * sizeof(bmh_alnreg_v));
	qa_sam_opt(opt, &so);
	w.cand = 0, w.sopt = &so;
	g_pes_removed = 0;
	if (qa_pestat_device()) { /* the pair walk in phase 1: a paired-end chunk whose statistics are not given, in batches that split no pair */
		const int odd_exact = getenv("BMH_BATCH_EXACT") && ((opt->batch_size > 0 ? opt->batch_size : 1) & 1);
		why_host = !pe ? "single-end reads" : pes0 ? "the insert-size statistics are given" : (n & 1) ? "an odd number of reads" : n < 2 ? "no pair"
		           : odd_exact ? "BMH_BATCH_EXACT=1 with an odd batch size" : opt->max_ins >= (1 << 30) ? "max_ins >= 2^30" : 0;
		if (!why_host && !(w.cand = (uint32_t *)calloc((size_t)(n >> 1), sizeof(uint32_t)))) bmh_tls_die("out of memory for the insert-size words", BMH_E_NOMEM);
	}
	{ /* bwamem.c:1313, with the batch size evened out (qa_even_batch) */
		const int nt = qa_threads("BMH_P1_THREADS", opt->n_threads);
		int b = qa_even_batch(opt, n, nt);
		p1_batch[0] = b;
		if (w.cand && (b & 1)) ++b; /* no pair straddles two batches; reads are independent, so the regions do not change */
		p1_batch[1] = b;
		kt_for_batch(nt, qa_worker1_batched, &w, n, b);
	}
	t_[1] = realtime();
	if (pe) {                                                                /* bwamem.c:1314-1317 */
		if (pes0) memcpy(pes, pes0, 4 * sizeof(bmh_pestat_t));
		else if (w.cand) { /* the words came down with the regions: what is left of mem_pestat is a pass over a flat array */
			int rc = bmh_pestat_from_candidates(&so, n >> 1, w.cand, pes, bwa_verbose);
			if (rc) bmh_tls_die("the device's insert-size words are inconsistent", rc);
		} else bmh_pestat(&so, bns->l_pac, n, w.regs, pes, bwa_verbose), ++n_host_pestat;
	}
	t_pes = realtime();
	/* reads are base codes by now (bwamem.c:1093-1094) */
	reads = (bmh_read_t *)malloc(sizeof(bmh_read_t) * (size_t)n);
	for (i = 0; i < n; ++i) reads[i].l_seq = seqs[i].l_seq, reads[i].seq = (const uint8_t *)seqs[i].seq;
	qa_params(opt, &p);
	{
		const char *pr = getenv("BMH_PAC_RESIDENT");
		J.resident = !(pr && pr[0] == '0');
	}
	J.opt = opt, J.bns = bns, J.pac = pac, J.n = n, J.seqs = seqs, J.regs = w.regs, J.reads = reads, J.params = &p, J.pes = pes;
	J.sopt = &so, J.n_processed = n_processed;
	/* Phase 2 and mate rescue are host code with a GPU batch in the middle of every slice; half again as many threads as -t
	 * keep the cores busy while some of them sleep on the GPU (measured at -t 16 on 16 cores: a chunk's rescue + phase 2
	 * 0.105 -> 0.080 s; twice as many is no better; phase 1 does not gain). */
	nt2 = qa_threads("BMH_P2_THREADS", opt->n_threads + opt->n_threads / 2);
	J.n_slices = qa_threads("BMH_P2_SLICES", nt2);
	if (rescue) { /* the whole chunk's mate rescue (the block of mem_sam_pe at bwamem_pair.c:251-263), one bmh_matesw_batch per slice */
		g_msw_calls = g_msw_rounds_max = g_msw_bytes = g_msw_dedup_calls = g_msw_active = 0;
		kt_for(nt2, qa_matesw_slice, &J, J.n_slices);
		if (getenv("BMH_VERBOSE")) {
			fprintf(stderr, "[bwamem_hip] mate rescue: %d pairs, %lld ksw_align2 calls in %lld GPU rounds, %lld pool bytes\n", n >> 1,
			        g_msw_calls, g_msw_rounds_max, g_msw_bytes);
			if (qa_matesw_device()) /* (active: pairs rescue made at least one ksw_align2 call for) */
				fprintf(stderr, "[bwamem_hip] mate rescue on the device: %lld active pairs, %lld host dedup callbacks\n", g_msw_active, g_msw_dedup_calls);
		}
	}
	t_[2] = realtime();
	kt_for(nt2, qa_sam_slice, &J, J.n_slices); /* bwamem.c:1318-1319 */
	t_[3] = realtime();
	free(reads);
	if (getenv("BMH_VERBOSE")) {
		if (qa_regs_device()) {
			fprintf(stderr, "[bwamem_hip] seeding batch thread-seconds so far: bmh_seed_chain_regs_batch (seeding + chaining + regions on the device) %.3f\n",
			        g_seedchain_us * 1e-6);
			fprintf(stderr, "[bwamem_hip] phase 1 thread-seconds so far: wait %.3f, seeding + chaining + regions batch %.3f\n", g_p1_us[0] * 1e-6,
			        g_p1_us[1] * 1e-6);
		} else if (qa_chain_device()) {
			fprintf(stderr, "[bwamem_hip] seeding batch thread-seconds so far: bmh_seed_chain_batch (seeding + chaining on the device) %.3f\n",
			        g_seedchain_us * 1e-6);
			fprintf(stderr, "[bwamem_hip] phase 1 thread-seconds so far: wait %.3f, seeding + chaining batch %.3f, chaining on the host %.3f, wait %.3f, extension batch %.3f\n",
			        g_p1_us[0] * 1e-6, g_p1_us[1] * 1e-6, g_p1_us[2] * 1e-6, g_p1_us[3] * 1e-6, g_p1_us[4] * 1e-6);
		} else {
			fprintf(stderr, "[bwamem_hip] seeding batch thread-seconds so far: bmh_smem_batch %.3f, look-up keys %.3f, bmh_sa_batch %.3f\n",
			        g_seed_us[0] * 1e-6, g_seed_us[1] * 1e-6, g_seed_us[2] * 1e-6);
			fprintf(stderr, "[bwamem_hip] phase 1 thread-seconds so far: wait %.3f, seeding batch %.3f, chaining on the host %.3f, wait %.3f, extension batch %.3f\n",
			        g_p1_us[0] * 1e-6, g_p1_us[1] * 1e-6, g_p1_us[2] * 1e-6, g_p1_us[3] * 1e-6, g_p1_us[4] * 1e-6);
		}
		fprintf(stderr, "[bwamem_hip] phase 1 so far: %lld chains %s, %lld seeds extended (+%lld speculated in vain), %lld short-chain Smith-Watermans batched\n",
		        g_p1_cnt[0],
		        qa_regs_device()    ? "and regions from bmh_seed_chain_regs_batch on the device"
		        : qa_chain_device() ? "from bmh_seed_chain_batch on the device"
		                            : "from bmh_chain_reads",
		        g_p1_cnt[1], g_p1_cnt[2], g_p1_cnt[3]);
		if (qa_dedup_device())
			fprintf(stderr, "[bwamem_hip] region de-duplication so far: %lld regions de-duplicated on the device, %lld kept, %lld host bmh_sort_and_dedup calls in phase 1\n",
			        g_dedup_cnt[0], g_dedup_cnt[1], g_dedup_cnt[2]);
		if (qa_pestat_device()) {
			if (w.cand) {
				long long nc = 0;
				for (i = 0; i < n >> 1; ++i) nc += w.cand[i] != 0;
				fprintf(stderr, "[bwamem_hip] insert-size candidates from the device: %d pairs, %lld candidates, %lld exact matches removed on the device, %d host bmh_pestat calls\n",
				        n >> 1, nc, g_pes_removed, n_host_pestat);
				fprintf(stderr, "[bwamem_hip] insert-size candidates from the device: %d phase-1 batches of up to %d reads (evened out to %d%s)\n",
				        (n + p1_batch[1] - 1) / p1_batch[1], p1_batch[1], p1_batch[0],
				        p1_batch[1] != p1_batch[0] ? ", rounded up to an even number so that no pair straddles two batches" : "");
			} else
				fprintf(stderr, "[bwamem_hip] insert-size candidates from the device: off for this chunk (%s), %d host bmh_pestat calls\n", why_host, n_host_pestat);
		}
		if (rescue) fprintf(stderr, "[bwamem_hip] mate rescue driver so far: %.3f thread-s in %s\n", g_msw_us * 1e-6, qa_matesw_device() ? "bmh_matesw_device" : "bmh_matesw_batch");
		fprintf(stderr, "[bwamem_hip] phase 2 thread-seconds so far: wait %.3f, bmh_sam_batch %.3f\n", g_sam_us[0] * 1e-6, g_sam_us[1] * 1e-6);
		if (qa_decide_device())
			fprintf(stderr, "[bwamem_hip] phase 2 decisions on the device: %lld units, %lld host fall-backs\n", g_decide_cnt[0], g_decide_cnt[1]);
		if (qa_wanted_device())
			fprintf(stderr, "[bwamem_hip] phase 2 alignments planned on the device: %lld regions, %lld fixed, %lld redone on the host\n",
			        g_wanted_cnt[0], g_wanted_cnt[1], g_wanted_cnt[2]);
		if (qa_phase2_device())
			fprintf(stderr, "[bwamem_hip] phase 2 on the device in one session: %lld units, %lld regions, %lld fixed, %lld redone on the host, %lld host fall-backs\n",
			        g_phase2_cnt[0], g_phase2_cnt[1], g_phase2_cnt[2], g_phase2_cnt[3], g_phase2_cnt[4]);
		if (qa_phase2_text_device())
			fprintf(stderr, "[bwamem_hip] phase 2 and SAM text on the device in one session: %lld units, %lld regions, %lld redone on the host, %lld lines, %lld bytes, %lld host fall-backs\n",
			        g_phase2_text_cnt[0], g_phase2_text_cnt[1], g_phase2_text_cnt[2], g_phase2_text_cnt[3], g_phase2_text_cnt[4], g_phase2_text_cnt[5]);
		if (qa_region_long()) {
			long long ld = 0, rh = 0;
			bmh_reg2cigar_totals_(&ld, &rh);
			fprintf(stderr, "[bwamem_hip] long region records so far: %lld regions finished on the device, %lld redone with host copies\n", ld, rh);
		}
		if (qa_samtext_device())
			fprintf(stderr, "[bwamem_hip] SAM text on the device: %lld reads, %lld lines, %lld bytes\n", g_samtext_cnt[0], g_samtext_cnt[1], g_samtext_cnt[2]);
		if (bmh_pool_wide()) { /* BMH_WIDE_EXT=1 */
			fprintf(stderr, "[bwamem_hip] wide extension so far: %lld extension tasks on the int32 kernel\n", bmh_pool_wide_tasks());
			fprintf(stderr, "[bwamem_hip] wide Smith-Waterman so far: %lld ksw_align2 tasks on the long-query kernel\n", bmh_pool_swl_tasks());
		}
		fprintf(stderr, "[bwamem_hip] long global alignments so far: %lld ksw_global2 tasks on the band-ring kernel\n", bmh_pool_glong_tasks());
		fprintf(stderr, "[bwamem_hip] chunk of %d reads: phase 1 %.3f s, pestat %.3f s + mate rescue %.3f s, phase 2 (marking, pairing, global alignments, SAM) %.3f s\n", n,
		        t_[1] - t_[0], t_pes - t_[1], t_[2] - t_pes, t_[3] - t_[2]);
	}
	free(w.regs);
	free(w.cand);
processed:
	if (bwa_verbose >= 3)
		fprintf(stderr, "[M::%s] Processed %d reads in %.3f CPU sec, %.3f real sec\n", __func__, n, cputime() - ctime, realtime() - rtime);
}
