// api.hip -- the C-ABI of libbwamem_hip.so (include/bwamem_hip.h): contexts, parameter upload,
// host-buffer and device-resident batch entry points, static multi-GPU sharding.
// No CPU fallback lives here: if HIP is unusable every compute entry point returns an error.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <numeric>
#include <optional>
#include <vector>

#include "bmh_ctx.h"
#include "decide.h"
#include "wanted.h"
#include "samtext.h"
#include "../host/handoff_core.h"
#include "../host/pestat_core.h"

namespace bmh {

bmh_gate_fn g_gate_enter = nullptr, g_gate_leave = nullptr;
int g_wait_blocking = 0;

int set_hip_error(bmh_ctx *ctx, hipError_t e, const char *what)
{
	if (ctx) {
		ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
	}
	return BMH_E_HIP;
}

int ensure(bmh_ctx *ctx, DevBuf &b, size_t bytes)
{
	if (bytes <= b.cap) return BMH_OK;
	// growing means hipFree + hipMalloc, and both synchronise the whole device -- with many host threads in flight a
	// workspace that creeps up by a few per cent per batch stalls everybody again and again.  So: generous steps.
	size_t cap = std::max(bytes + bytes / 4, b.cap * 2);
	cap = (cap + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
	if (b.p) BMH_HIP(ctx, hipFree(b.p));
	b.p = nullptr, b.cap = 0;
	hipError_t e = hipMalloc(&b.p, cap);
	if (e != hipSuccess) {
		set_hip_error(ctx, e, "hipMalloc(workspace)");
		return BMH_E_NOMEM;
	}
	b.cap = cap;
	return BMH_OK;
}

int ensure_host(bmh_ctx *ctx, DevBuf &b, size_t bytes)
{
	if (bytes <= b.cap) return BMH_OK;
	size_t cap = std::max(bytes + bytes / 4, b.cap * 2); // pinned allocations are slow and synchronise too: see ensure()
	cap = (cap + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
	if (b.p) BMH_HIP(ctx, hipHostFree(b.p));
	b.p = nullptr, b.cap = 0;
	hipError_t e = hipHostMalloc(&b.p, cap, hipHostMallocDefault);
	if (e != hipSuccess) {
		set_hip_error(ctx, e, "hipHostMalloc(staging)");
		return BMH_E_NOMEM;
	}
	b.cap = cap;
	return BMH_OK;
}

static void free_buf(DevBuf &b)
{
	if (b.p) (void)hipFree(b.p);
	b.p = nullptr, b.cap = 0;
}

// wait for the context's stream, then read and clear the device error flag
static int fetch_err(bmh_ctx *ctx)
{
	const hipError_t c = hipMemcpyAsync(ctx->h_err, ctx->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream)); // (also when the copy could not be enqueued)
	if (c != hipSuccess) return set_hip_error(ctx, c, "hipMemcpyAsync(error flag)");
	int e = *ctx->h_err;
	if (e != 0) {
		BMH_HIP(ctx, hipMemsetAsync(ctx->d_err, 0, sizeof(int), ctx->stream));
		BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
		ctx->last_error = "a task was outside the supported range (see bwamem_hip.h)";
	}
	return e;
}

// The callers' host buffers are pageable.  Up to kStageMax bytes per direction and call they travel through the
// context's pinned staging buffers -- one memcpy on the host, then a DMA that does not depend on the runtime's own
// (slow, process-wide serialised) path for pageable memory; larger transfers go the direct way, and so do all the
// transfers of a Stager that stage() was not called for.
constexpr size_t kStageMax = (size_t)64 << 20;
// where a phase 2 session counts its bytes and the host's waits: h2d_bytes, d2h_bytes and waits of the statistics record it reports to
// (ctx->p2, ctx->stx or ctx->pt).  Null: nothing is counted (the batch calls, the stand-alone passes A and B)
struct StagerCount {
	int64_t *h2d = nullptr, *d2h = nullptr;
	int32_t *waits = nullptr;
};
struct Stager {
	bmh_ctx *ctx;
	bool wide; // an extension batch: end() adds what the int32 kernel received to ctx->wide_total
	bool up = false, down = false;
	StagerCount cnt;
	size_t up_used = 0, down_used = 0;
	struct Pending {
		void *dst;
		size_t off, bytes;
	} pend[4];
	int n_pend = 0;
	explicit Stager(bmh_ctx *c = nullptr, bool count_wide = false) : ctx(c), wide(count_wide) {}
	int stage(size_t up_bytes, size_t down_bytes)
	{
		int rc;
		up = up_bytes <= kStageMax, down = down_bytes <= kStageMax;
		if (up && (rc = ensure_host(ctx, ctx->h_up, up_bytes + 256))) return rc;
		if (down && (rc = ensure_host(ctx, ctx->h_down, down_bytes + 256))) return rc;
		return BMH_OK;
	}
	int h2d(void *d_dst, const void *src, size_t bytes)
	{
		if (up) {
			uint8_t *h = (uint8_t *)ctx->h_up.p + up_used;
			memcpy(h, src, bytes);
			up_used += (bytes + 63) & ~(size_t)63, src = h;
		}
		if (cnt.h2d) *cnt.h2d += (int64_t)bytes;
		BMH_HIP(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
		return BMH_OK;
	}
	int d2h(void *dst, const void *d_src, size_t bytes)
	{
		void *to = dst;
		if (down && n_pend < 4) {
			to = (uint8_t *)ctx->h_down.p + down_used;
			pend[n_pend++] = Pending{dst, down_used, bytes};
			down_used += (bytes + 63) & ~(size_t)63;
		}
		if (cnt.d2h) *cnt.d2h += (int64_t)bytes;
		BMH_HIP(ctx, hipMemcpyAsync(to, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
		return BMH_OK;
	}
	// a wait the session made itself, behind a download of `bytes` that did not go through d2h()
	void waited(size_t bytes) { if (cnt.waits) ++*cnt.waits, *cnt.d2h += (int64_t)bytes; }
	// The one way out of a call that has enqueued work on ctx's stream, rc being how far it got: wait for the stream and read
	// and clear the device error flag whatever happened, then -- only if everything was enqueued -- copy what was staged to
	// the caller and count the int32 kernel's tasks.  Returns rc, else the device's verdict.
	int end(int rc)
	{
		waited(0);
		if (rc) { // (the flag's text must not replace why the call failed)
			std::string why = std::move(ctx->last_error);
			(void)fetch_err(ctx);
			ctx->last_error = std::move(why);
			return rc;
		}
		rc = fetch_err(ctx);
		for (int k = 0; k < n_pend; ++k) memcpy(pend[k].dst, (const uint8_t *)ctx->h_down.p + pend[k].off, pend[k].bytes);
		if (wide && ctx->wide_last) {
			unsigned long long c = 0;
			BMH_HIP(ctx, hipMemcpyAsync(&c, ctx->d_wide_stat, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
			BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
			ctx->wide_total += (long long)c;
		}
		return rc;
	}
};

// A global batch's CIGAR pool: the device copy holds `words` words at the caller's offsets, words [lo, lo + n) come back to dst
struct CigarDown {
	size_t words;
	uint32_t *dst;
	size_t lo, n;
};

// One host-buffer batch on st.ctx up to its last download, leaving through st.end(): the pool (unless null: the one
// bmh_upload_pool() left on the device) and the tasks up, launch(ctx, d_pool, d_tasks, d_res), the results and the CIGAR
// words down.  Through the pinned staging buffers if `staged`, else copied directly (the sharded calls).
template <class Task, class Result, class Launch>
static int enqueue_batch(Stager &st, bool staged, const uint8_t *pool, size_t pool_bytes, const Task *tasks, int64_t n, Result *results,
                         Launch launch, const CigarDown *cig = nullptr)
{
	bmh_ctx *c = st.ctx;
	const size_t tb = (size_t)n * sizeof(Task), rb = (size_t)n * sizeof(Result);
	int rc;
	if (pool) {
		c->pool_resident = false;
		if ((rc = ensure(c, c->d_pool, pool_bytes + 16))) return rc;
	}
	if ((rc = ensure(c, c->d_tasks, tb)) || (rc = ensure(c, c->d_res, rb)) || (cig && (rc = ensure(c, c->d_cigar, (cig->words + 4) * 4))))
		return rc;
	if (staged && (rc = st.stage((pool ? pool_bytes + 64 : 0) + tb, rb + (cig ? 64 + cig->n * 4 : 0)))) return rc;
	if (pool && (rc = st.h2d(c->d_pool.p, pool, pool_bytes))) return rc;
	if ((rc = st.h2d(c->d_tasks.p, tasks, tb))) return rc;
	if ((rc = launch(c, (const uint8_t *)c->d_pool.p, (const Task *)c->d_tasks.p, (Result *)c->d_res.p))) return rc;
	if ((rc = st.d2h(results, c->d_res.p, rb))) return rc;
	if (cig && cig->n && (rc = st.d2h(cig->dst, (const uint32_t *)c->d_cigar.p + cig->lo, cig->n * 4))) return rc;
	return BMH_OK;
}

} // namespace bmh

using namespace bmh;

extern "C" {

int bmh_version(void) { return BMH_VERSION; }

void bmh_set_wait_mode(int blocking) { bmh::g_wait_blocking = blocking != 0; }

int bmh_set_device_gate(bmh_gate_fn enter, bmh_gate_fn leave)
{
	if ((enter == nullptr) != (leave == nullptr)) return BMH_E_ARG;
	g_gate_enter = enter, g_gate_leave = leave;
	return BMH_OK;
}

const char *bmh_strerror(int code)
{
	switch (code) {
	case BMH_OK: return "ok";
	case BMH_E_NODEVICE: return "no usable HIP device";
	case BMH_E_HIP: return "HIP runtime error";
	case BMH_E_ARG: return "invalid argument";
	case BMH_E_RANGE: return "task outside the supported range";
	case BMH_E_NOMEM: return "out of memory";
	case BMH_E_CIGAR_CAP: return "CIGAR longer than the reserved slot range";
	default: return "unknown error";
	}
}

const char *bmh_last_error(const bmh_ctx_t *ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int bmh_device_count(int *n)
{
	int c = 0;
	if (!n) return BMH_E_ARG;
	if (hipGetDeviceCount(&c) != hipSuccess) {
		*n = 0;
		return BMH_E_NODEVICE;
	}
	*n = c;
	return BMH_OK;
}

int bmh_ctx_create(bmh_ctx_t **out, int device)
{
	if (!out) return BMH_E_ARG;
	*out = nullptr;
	int c = 0;
	if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) return BMH_E_NODEVICE;
	if (device < 0 || device >= c) return BMH_E_ARG;
	bmh_ctx *ctx = new (std::nothrow) bmh_ctx();
	if (!ctx) return BMH_E_NOMEM;
	ctx->device = device;
	hipError_t e;
	if ((e = hipSetDevice(device)) == hipSuccess && g_wait_blocking) { // (also covers hipMemcpy / hipFree; refused on an active device by some runtimes: not an error)
		if (hipSetDeviceFlags(hipDeviceScheduleBlockingSync) != hipSuccess) (void)hipGetLastError();
	}
	if (e != hipSuccess || (e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipMalloc((void **)&ctx->d_err, 16)) != hipSuccess || (e = hipMemset(ctx->d_err, 0, 16)) != hipSuccess ||
	    (e = hipHostMalloc((void **)&ctx->h_err, sizeof(int), hipHostMallocDefault)) != hipSuccess ||
	    (e = hipEventCreate(&ctx->ev0)) != hipSuccess || (e = hipEventCreate(&ctx->ev1)) != hipSuccess ||
	    (e = hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming)) != hipSuccess ||
	    (e = hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming)) != hipSuccess ||
	    (e = hipEventCreateWithFlags(&ctx->ev_join2, hipEventDisableTiming)) != hipSuccess ||
	    (e = hipEventCreateWithFlags(&ctx->ev_wait, hipEventDisableTiming | hipEventBlockingSync)) != hipSuccess) {
		fprintf(stderr, "[bwamem_hip] context creation failed: %s\n", hipGetErrorString(e));
		bmh_ctx_destroy(ctx);
		return BMH_E_NODEVICE;
	}
	for (int b = 0; b <= kExtBinsMax; ++b)
		if (hipEventCreate(&ctx->ev_bin[b]) != hipSuccess || hipEventCreate(&ctx->ev_bin_end[b]) != hipSuccess) {
			bmh_ctx_destroy(ctx);
			return BMH_E_NODEVICE;
		}
	for (int b = 0; b < 5; ++b)
		if (hipEventCreate(&ctx->ev_sround[b]) != hipSuccess) {
			bmh_ctx_destroy(ctx);
			return BMH_E_NODEVICE;
		}
	for (int b = 0; b < 4; ++b)
		if (hipEventCreate(&ctx->ev_gbin[b]) != hipSuccess) {
			bmh_ctx_destroy(ctx);
			return BMH_E_NODEVICE;
		}
	ctx->stream = ctx->own_stream;
	(void)hipDeviceGetAttribute(&ctx->ncu, hipDeviceAttributeMultiprocessorCount, device);
	if (ctx->ncu <= 0) ctx->ncu = 256;
	if (const char *m = getenv("BMH_EXT_PERSIST")) ctx->ext_persist = atoi(m) != 0;
	if (const char *m = getenv("BMH_EXT_SPLIT96")) ctx->ext_split96 = atoi(m) != 0; // (A/B knob)
	if (const char *m = getenv("BMH_EXT_GRID_MULT")) ctx->ext_grid_mult = atoi(m) > 0 ? atoi(m) : ctx->ext_grid_mult;
	if (const char *m = getenv("BMH_EXT_STOP")) ctx->ext_stop = atoi(m) != 0; // (A/B knob)
	if (const char *m = getenv("BMH_EXT_NARROW")) ctx->ext_narrow = atoi(m) != 0; // (A/B knob)
	if (const char *m = getenv("BMH_EXT_BANDKEY")) ctx->ext_bandkey = atoi(m) != 0; // (A/B knob)
	if (const char *m = getenv("BMH_EXT_SMALL")) ctx->small_batch = atoi(m) >= 0 ? atoi(m) : ctx->small_batch;
	if (getenv("BMH_EXT_MODE")) ctx->ext_mode_forced = true;
	if (const char *m = getenv("BMH_EXT_MODE")) ctx->force_kernel = !strcmp(m, "lds") ? 1 : !strcmp(m, "reg") ? 2 : !strcmp(m, "grp") ? 3 : !strcmp(m, "lanex4") ? 4 : !strcmp(m, "wide") ? 5 : 0;
	if (const char *m = getenv("BMH_GLB_MODE")) ctx->glb_mode = !strcmp(m, "wave") ? 1 : 0;
	if (const char *m = getenv("BMH_SW_MODE")) ctx->sw_mode = !strcmp(m, "generic") ? 1 : 0;
	if (const char *m = getenv("BMH_SW_WAVE")) ctx->sw_wave = atoi(m) != 0;
	if (const char *m = getenv("BMH_GL_FAST")) ctx->glb_fast = atoi(m) != 0;
	if (const char *m = getenv("BMH_GLB_C32")) ctx->glb_c32 = atoi(m) != 0; // (A/B knob)
	if (const char *m = getenv("BMH_GLB_NARROW")) ctx->glb_narrow = atoi(m) != 0; // (A/B knob)
	if (const char *m = getenv("BMH_GLB_EXACT")) ctx->glb_exact = atoi(m) >= 7 ? 7 : atoi(m) >= 3 ? 3 : 0; // (A/B knob)
	if (const char *m = getenv("BMH_GRID_MULT")) ctx->grid_mult = atoi(m) > 0 ? atoi(m) : 1;
	if (const char *m = getenv("BMH_EXT_SCHED")) ctx->ext_sched = atoi(m) >= 0 && atoi(m) <= 4 ? atoi(m) : -1;
	*out = ctx;
	return BMH_OK;
}

static void pac_release(bmh_ctx_t *ctx);
void free_bwt_binding(void *p); // fmindex.hip

int bmh_ctx_destroy(bmh_ctx_t *ctx)
{
	if (!ctx) return BMH_OK;
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) (void)stream_wait(ctx, ctx->stream);
	free_buf(ctx->d_pool), free_buf(ctx->d_tasks), free_buf(ctx->d_res), free_buf(ctx->d_order);
	free_buf(ctx->d_cigar), free_buf(ctx->d_scratch), free_buf(ctx->d_bins), free_buf(ctx->d_gband), free_buf(ctx->d_ext_rows), free_buf(ctx->d_eband), free_buf(ctx->d_zslab), free_buf(ctx->d_sw), free_buf(ctx->d_swrm);
	free_buf(ctx->d_seedws), free_buf(ctx->d_region), free_buf(ctx->d_chain), free_buf(ctx->d_wide_slab), free_buf(ctx->d_c2r);
	if (ctx->d_wide_stat) (void)hipFree(ctx->d_wide_stat);
	if (ctx->d_swl_stat) (void)hipFree(ctx->d_swl_stat);
	free_buf(ctx->d_swl), free_buf(ctx->d_dedup), free_buf(ctx->d_msw), free_buf(ctx->d_decide), free_buf(ctx->d_logk);
	free(ctx->h_logk);
	free_buf(ctx->d_refidx), free_buf(ctx->d_wanted);
	if (ctx->h_wstat) (void)hipHostFree(ctx->h_wstat);
	free_buf(ctx->d_refnames), free_buf(ctx->d_samtext), free_buf(ctx->d_sam_out);
	if (ctx->h_ststat) (void)hipHostFree(ctx->h_ststat);
	if (ctx->h_ptstat) (void)hipHostFree(ctx->h_ptstat);
	for (auto &e : ctx->ev_gather)
		if (e) (void)hipEventDestroy(e);
	for (auto &e : ctx->ev_samtext)
		if (e) (void)hipEventDestroy(e);
	for (auto &e : ctx->ev_wanted)
		if (e) (void)hipEventDestroy(e);
	for (auto &e : ctx->ev_decide)
		if (e) (void)hipEventDestroy(e);
	for (auto &e : ctx->ev_chain)
		if (e) (void)hipEventDestroy(e);
	for (auto &e : ctx->ev_dedup)
		if (e) (void)hipEventDestroy(e);
	free_buf(ctx->d_rlong), free_buf(ctx->d_lcig), free_buf(ctx->d_lmd);
	for (auto &e : ctx->ev_rlong)
		if (e) (void)hipEventDestroy(e);
	free_buf(ctx->d_pestat);
	for (auto &e : ctx->ev_pestat)
		if (e) (void)hipEventDestroy(e);
	for (auto &e : ctx->ev_plan)
		if (e) (void)hipEventDestroy(e);
	free_buf(ctx->d_mswt), free_buf(ctx->d_mswin), free_buf(ctx->d_pbase);
	for (auto &e : ctx->ev_mswt)
		if (e) (void)hipEventDestroy(e);
	for (auto &h : ctx->hint) {
		if (h.ev) (void)hipEventDestroy(h.ev);
		if (h.h) (void)hipHostFree(h.h);
	}
	pac_release(ctx);
	if (ctx->bwt_bind) free_bwt_binding(ctx->bwt_bind);
	if (ctx->d_err) (void)hipFree(ctx->d_err);
	if (ctx->h_err) (void)hipHostFree(ctx->h_err);
	if (ctx->h_up.p) (void)hipHostFree(ctx->h_up.p);
	if (ctx->h_down.p) (void)hipHostFree(ctx->h_down.p);
	if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
	if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
	for (int b = 0; b <= kExtBinsMax; ++b)
	{
		if (ctx->ev_bin[b]) (void)hipEventDestroy(ctx->ev_bin[b]);
		if (ctx->ev_bin_end[b]) (void)hipEventDestroy(ctx->ev_bin_end[b]);
	}
	for (int b = 0; b < 4; ++b)
		if (ctx->ev_gbin[b]) (void)hipEventDestroy(ctx->ev_gbin[b]);
	for (int b = 0; b < 2; ++b)
		if (ctx->ev_glong[b]) (void)hipEventDestroy(ctx->ev_glong[b]);
	for (int b = 0; b < 2; ++b)
		if (ctx->ev_swl[b]) (void)hipEventDestroy(ctx->ev_swl[b]);
	for (int b = 0; b < 5; ++b)
		if (ctx->ev_sround[b]) (void)hipEventDestroy(ctx->ev_sround[b]);
	if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
	if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
	if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
	if (ctx->ev_join2) (void)hipEventDestroy(ctx->ev_join2);
	if (ctx->ev_wait) (void)hipEventDestroy(ctx->ev_wait);
	if (ctx->aux2_stream) (void)hipStreamDestroy(ctx->aux2_stream);
	if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
	delete ctx;
	return BMH_OK;
}

int bmh_ctx_set_params(bmh_ctx_t *ctx, const bmh_params_t *p)
{
	if (!ctx || !p) return BMH_E_ARG;
	// o_ins>=0: the scan form of F needs it.  e>=1: the reference's extension divides by e (ksw.c:401,404); ksw_global2 does
	// not, so a zero gap extension gives parameters that bmh_global_batch and bmh_global_batch_device alone take (glb_params without
	// have_params: every other call finds the context as it is before the first bmh_ctx_set_params)
	if (p->e_del < 0 || p->e_ins < 0 || p->o_ins < 0 || p->o_del < 0) {
		ctx->last_error = "need e_del>=0, e_ins>=0, o_del>=0, o_ins>=0";
		return BMH_E_RANGE;
	}
	ctx->params = *p;
	DevParams &d = ctx->dev;
	d.o_del = p->o_del, d.e_del = p->e_del, d.o_ins = p->o_ins, d.e_ins = p->e_ins, d.zdrop = p->zdrop;
	d.max_mat = 0; // ksw.c:399-400 starts the maximum at 0
	int mn = 0;
	for (int i = 0; i < 25; ++i) d.max_mat = std::max(d.max_mat, (int)p->mat[i]), mn = std::min(mn, (int)p->mat[i]);
	d.bias = -mn;
	{
		int8_t lo = 127;
		for (int i = 0; i < 25; ++i) lo = std::min(lo, p->mat[i]);
		d.sw_shift = (uint8_t)(256 - (uint8_t)lo);
	}
	uint8_t bytes[28] = {0};
	memcpy(bytes, p->mat, 25);
	memcpy(d.matw, bytes, 28);
	ctx->have_params = p->e_del >= 1 && p->e_ins >= 1, ctx->glb_params = true;
	return BMH_OK;
}

// The reference is immutable and large (hg38: 0.78 GB), and the reference program drives phase 1 from many host
// threads, each with its own context: one device copy per (device, host buffer) is shared by all of them.
struct PacShare {
	int device;
	const uint8_t *h;
	long long l_pac;
	void *d;
	int refs;
};
static std::mutex g_pac_mu;
static std::vector<PacShare> g_pacs;

static void pac_release(bmh_ctx_t *ctx)
{
	if (!ctx->h_pac) return;
	std::lock_guard<std::mutex> lk(g_pac_mu);
	for (size_t i = 0; i < g_pacs.size(); ++i)
		if (g_pacs[i].device == ctx->device && g_pacs[i].h == ctx->h_pac && g_pacs[i].l_pac == ctx->dev.l_pac) {
			if (--g_pacs[i].refs == 0) {
				(void)hipFree(g_pacs[i].d);
				g_pacs.erase(g_pacs.begin() + (long)i);
			}
			break;
		}
	ctx->h_pac = nullptr, ctx->dev.pac = nullptr, ctx->dev.l_pac = 0;
}

int bmh_ctx_set_pac(bmh_ctx_t *ctx, const uint8_t *pac, int64_t l_pac)
{
	if (!ctx || !pac || l_pac <= 0) return BMH_E_ARG;
	if (ctx->h_pac == pac && ctx->dev.l_pac == l_pac) return BMH_OK; // already resident
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	pac_release(ctx);
	std::lock_guard<std::mutex> lk(g_pac_mu);
	for (auto &e : g_pacs)
		if (e.device == ctx->device && e.h == pac && e.l_pac == l_pac) {
			++e.refs;
			ctx->h_pac = pac, ctx->dev.pac = (const uint8_t *)e.d, ctx->dev.l_pac = l_pac;
			return BMH_OK;
		}
	const size_t bytes = (size_t)(l_pac / 4 + 1);
	void *d = nullptr;
	if (hipMalloc(&d, bytes + 16) != hipSuccess) {
		(void)hipGetLastError();
		ctx->last_error = "hipMalloc of " + std::to_string(bytes) + " bytes for the reference failed";
		return BMH_E_NOMEM;
	}
	if (hipMemcpy(d, pac, bytes, hipMemcpyHostToDevice) != hipSuccess) {
		(void)hipFree(d);
		ctx->last_error = "uploading the reference failed";
		return BMH_E_HIP;
	}
	g_pacs.push_back({ctx->device, pac, (long long)l_pac, d, 1});
	ctx->h_pac = pac, ctx->dev.pac = (const uint8_t *)d, ctx->dev.l_pac = l_pac;
	return BMH_OK;
}

// does the context hold exactly this reference?  (internal hook for the C drivers)
int bmh_ctx_has_pac_(const bmh_ctx_t *ctx, const uint8_t *pac, int64_t l_pac)
{
	return ctx && pac && ctx->h_pac == pac && ctx->dev.l_pac == l_pac;
}

int bmh_ctx_set_stream(bmh_ctx_t *ctx, void *s)
{
	if (!ctx) return BMH_E_ARG;
	ctx->stream = s ? (hipStream_t)s : ctx->own_stream;
	return BMH_OK;
}

int bmh_ctx_set_qcap(bmh_ctx_t *ctx, int qcap)
{
	if (!ctx || qcap < 1 || qcap > 65535) return BMH_E_ARG;
	ctx->qcap = qcap;
	return BMH_OK;
}

int bmh_ctx_set_wide_extension(bmh_ctx_t *ctx, int enable)
{
	if (!ctx) return BMH_E_ARG;
	if (enable && !ctx->d_wide_stat) {
		BMH_HIP(ctx, hipSetDevice(ctx->device));
		BMH_HIP(ctx, hipMalloc((void **)&ctx->d_wide_stat, sizeof(unsigned long long)));
		BMH_HIP(ctx, hipMemsetAsync(ctx->d_wide_stat, 0, sizeof(unsigned long long), ctx->stream));
		BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	}
	ctx->wide_ext = enable != 0;
	return BMH_OK;
}

int bmh_ctx_set_wide_sw(bmh_ctx_t *ctx, int enable)
{
	if (!ctx) return BMH_E_ARG;
	if (enable && !ctx->d_swl_stat) {
		BMH_HIP(ctx, hipSetDevice(ctx->device));
		BMH_HIP(ctx, hipMalloc((void **)&ctx->d_swl_stat, sizeof(unsigned long long)));
		BMH_HIP(ctx, hipMemsetAsync(ctx->d_swl_stat, 0, sizeof(unsigned long long), ctx->stream));
		BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	}
	ctx->wide_sw = enable != 0;
	return BMH_OK;
}

int bmh_sw_wide_stats(const bmh_ctx_t *cctx, int64_t *tasks, float *ms)
{
	if (!cctx || !tasks || !ms) return BMH_E_ARG;
	bmh_ctx *ctx = const_cast<bmh_ctx *>(cctx); // (waits for the stream; the context's settings are not touched)
	*tasks = 0, *ms = ctx->timing ? (float)ctx->swl_ms_sum : -1.f;
	if (!ctx->d_swl_stat) return BMH_OK; // (never turned on)
	unsigned long long c = 0;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, hipMemcpyAsync(&c, ctx->d_swl_stat, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	*tasks = (int64_t)c;
	return BMH_OK;
}

int bmh_extend_wide_stats(const bmh_ctx_t *cctx, int64_t *tasks, float *ms)
{
	if (!cctx || !tasks || !ms) return BMH_E_ARG;
	bmh_ctx *ctx = const_cast<bmh_ctx *>(cctx); // (waits for the stream; the context's settings are not touched)
	*tasks = 0, *ms = -1.f;
	if (!ctx->wide_last) return BMH_OK;
	unsigned long long c = 0;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, hipMemcpyAsync(&c, ctx->d_wide_stat, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	*tasks = (int64_t)c;
	if (ctx->timing) *ms = (float)ctx->wide_ms_sum;
	return BMH_OK;
}

int bmh_global_long_stats(const bmh_ctx_t *cctx, int64_t *tasks, float *ms)
{
	if (!cctx || !tasks || !ms) return BMH_E_ARG;
	bmh_ctx *ctx = const_cast<bmh_ctx *>(cctx); // (waits for the stream; the context's settings are not touched)
	unsigned long long c = 0;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, hipMemcpyAsync(&c, ctx->d_err + 2, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	*tasks = (int64_t)c, *ms = ctx->timing ? (float)ctx->glong_ms_sum : -1.f;
	return BMH_OK;
}

int bmh_ctx_sync(bmh_ctx_t *ctx)
{
	if (!ctx) return BMH_E_ARG;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	return fetch_err(ctx);
}

int bmh_set_kernel_timing(bmh_ctx_t *ctx, int enable)
{
	if (!ctx) return BMH_E_ARG;
	ctx->timing = enable != 0;
	ctx->ev_valid = false;
	return BMH_OK;
}

int bmh_last_kernel_ms(bmh_ctx_t *ctx, float *ms)
{
	if (!ctx || !ms) return BMH_E_ARG;
	*ms = -1.f;
	if (!ctx->ev_valid) return BMH_OK;
	BMH_HIP(ctx, hipEventSynchronize(ctx->ev1));
	BMH_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
	return BMH_OK;
}

int bmh_last_extend_bin_ms(bmh_ctx_t *ctx, float ms[6])
{
	if (!ctx || !ms) return BMH_E_ARG;
	for (int b = 0; b < kExtBins; ++b) ms[b] = -1.f;
	if (!ctx->ev_bin_valid) return BMH_OK;
	BMH_HIP(ctx, hipEventSynchronize(ctx->ev1)); // recorded after both streams joined
	for (int b = 0; b < kExtBins; ++b) BMH_HIP(ctx, hipEventElapsedTime(&ms[b], ctx->ev_bin[b], ctx->ev_bin_end[b]));
	return BMH_OK;
}

int bmh_extend_bin_ms_sum(bmh_ctx_t *ctx, double ms[6], long long *launches, int reset)
{
	if (!ctx || !ms) return BMH_E_ARG;
	for (int b = 0; b < kExtBins; ++b) ms[b] = ctx->ext_bin_ms_sum[b];
	if (launches) *launches = ctx->ext_bin_launches;
	if (reset) {
		for (int b = 0; b < kExtBins; ++b) ctx->ext_bin_ms_sum[b] = 0.0;
		ctx->ext_bin_launches = 0;
	}
	return BMH_OK;
}

int bmh_last_seedext_round_ms(bmh_ctx_t *ctx, float ms[4])
{
	if (!ctx || !ms) return BMH_E_ARG;
	ms[0] = ms[1] = ms[2] = ms[3] = -1.f;
	if (!ctx->ev_sround_valid) return BMH_OK;
	BMH_HIP(ctx, hipEventSynchronize(ctx->ev_sround[4]));
	for (int b = 0; b < 4; ++b) BMH_HIP(ctx, hipEventElapsedTime(&ms[b], ctx->ev_sround[b], ctx->ev_sround[b + 1]));
	return BMH_OK;
}

int bmh_last_global_bin_ms(bmh_ctx_t *ctx, float ms[3])
{
	if (!ctx || !ms) return BMH_E_ARG;
	ms[0] = ms[1] = ms[2] = -1.f;
	if (!ctx->ev_gbin_valid) return BMH_OK;
	BMH_HIP(ctx, hipEventSynchronize(ctx->ev_gbin[3]));
	for (int b = 0; b < 3; ++b) BMH_HIP(ctx, hipEventElapsedTime(&ms[b], ctx->ev_gbin[b], ctx->ev_gbin[b + 1]));
	return BMH_OK;
}

int bmh_last_global_bands(bmh_ctx_t *ctx, uint8_t *bands, int64_t n)
{
	if (!ctx || !bands || n <= 0 || n != ctx->gband_n || !ctx->d_gband.p) return BMH_E_ARG;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	BMH_HIP(ctx, hipMemcpy(bands, ctx->d_gband.p, (size_t)n, hipMemcpyDeviceToHost));
	return BMH_OK;
}

int bmh_last_global_bin_counts(bmh_ctx_t *ctx, uint32_t counts[8])
{
	if (!ctx || !counts || !ctx->gbins_valid || !ctx->d_bins.p) return BMH_E_ARG;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	BMH_HIP(ctx, hipMemcpy(counts, ctx->d_bins.p, kSortBins * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return BMH_OK;
}

int bmh_ctx_set_extend_rows(bmh_ctx_t *ctx, int64_t cap)
{
	if (!ctx || cap < 0 || cap > 0xffffffffLL) return BMH_E_ARG;
	ctx->ext_rows_cap = cap, ctx->ext_rows_n = 0;
	return BMH_OK;
}

int bmh_last_extend_rows(bmh_ctx_t *ctx, uint16_t *rows, int64_t n)
{
	if (!ctx || !rows || n <= 0 || n > ctx->ext_rows_n || !ctx->d_ext_rows.p) return BMH_E_ARG;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	BMH_HIP(ctx, hipMemcpy(rows, ctx->d_ext_rows.p, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost));
	return BMH_OK;
}

int bmh_last_extend_bands(bmh_ctx_t *ctx, uint8_t *bands, int64_t n)
{
	if (!ctx || !bands || n <= 0 || n != ctx->eband_n || !ctx->d_eband.p) return BMH_E_ARG;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	BMH_HIP(ctx, hipMemcpy(bands, ctx->d_eband.p, (size_t)n, hipMemcpyDeviceToHost));
	return BMH_OK;
}

// ------------------------------------------------------------------ extend

int bmh_extend_batch_device(bmh_ctx_t *ctx, const uint8_t *d_pool, const bmh_ext_task_t *d_tasks, int64_t n,
                            bmh_ext_result_t *d_res, const uint32_t *d_order)
{
	if (!ctx || n < 0 || (n > 0 && (!d_pool || !d_tasks || !d_res))) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	if (n > 0xffffffffLL) return BMH_E_ARG;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	return launch_extend(ctx, d_pool, d_tasks, n, d_res, d_order, ctx->qcap);
}

static int validate_ext(bmh_ctx *ctx, const bmh_ext_task_t *t, int64_t n, size_t pool_bytes, int *qmax)
{
	int qm = 1;
	for (int64_t k = 0; k < n; ++k) {
		const bmh_ext_task_t &x = t[k];
		const bool qr = x.flags & BMH_F_QREV, tr = x.flags & BMH_F_TREV, tp = x.flags & BMH_F_TPAC;
		const uint64_t qlo = qr ? x.q_off - (x.qlen ? x.qlen - 1 : 0) : x.q_off, thi_len = x.tlen;
		const uint64_t tlo = tr ? x.t_off - (x.tlen ? x.tlen - 1 : 0) : x.t_off;
		const uint64_t tspace = tp ? (uint64_t)(ctx->dev.l_pac << 1) : (uint64_t)pool_bytes;
		if (tp && !ctx->dev.pac) {
			ctx->last_error = "task " + std::to_string(k) + " has BMH_F_TPAC but no reference was uploaded (bmh_ctx_set_pac)";
			return BMH_E_ARG;
		}
		if ((qr && x.qlen && x.q_off + 1 < x.qlen) || (tr && x.tlen && x.t_off + 1 < x.tlen) || qlo + x.qlen > pool_bytes ||
		    tlo + thi_len > tspace) {
			ctx->last_error = "task " + std::to_string(k) + " reads outside the sequence pool";
			return BMH_E_ARG;
		}
		const int h0 = x.h0 < 0 ? 0 : x.h0;
		if (!ctx->wide_ext && (int64_t)h0 + (int64_t)x.qlen * ctx->dev.max_mat > kScoreLimit) {
			ctx->last_error = "task " + std::to_string(k) + ": h0 + qlen*max(mat) exceeds the 16-bit score range";
			return BMH_E_RANGE;
		}
		if (ctx->wide_ext && (int64_t)h0 + (int64_t)x.qlen * ctx->dev.max_mat > kWideScoreLimit) {
			ctx->last_error = "task " + std::to_string(k) + ": h0 + qlen*max(mat) exceeds the wide extension's score range (2^24)";
			return BMH_E_RANGE;
		}
		qm = std::max(qm, (int)x.qlen);
	}
	*qmax = qm;
	return BMH_OK;
}

int bmh_extend_batch(bmh_ctx_t *ctx, const uint8_t *pool, size_t pool_bytes, const bmh_ext_task_t *tasks, int64_t n,
                     bmh_ext_result_t *results)
{
	if (!ctx || n < 0 || (n > 0 && (!tasks || !results))) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	if (n == 0) return BMH_OK;
	if (n > 0xffffffffLL) return BMH_E_ARG;
	if (!pool && !ctx->pool_resident) return BMH_E_ARG; // (null: the pool left on the device by bmh_upload_pool())
	int qmax = 1, rc;
	if ((rc = validate_ext(ctx, tasks, n, pool ? pool_bytes : ctx->pool_bytes, &qmax))) return rc;
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Stager st(ctx, true);
	// launch order: the dispatcher sorts the tasks on the device (bin, length bucket, row estimate)
	return st.end(enqueue_batch(st, true, pool, pool_bytes, tasks, n, results, [&](bmh_ctx *c, auto p, auto t, auto r) {
		return launch_extend(c, p, t, n, r, nullptr, qmax);
	}));
}

int bmh_upload_pool(bmh_ctx_t *ctx, const uint8_t *pool, size_t bytes)
{
	if (!ctx || !pool) return BMH_E_ARG;
	int rc;
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	ctx->pool_resident = false;
	if ((rc = ensure(ctx, ctx->d_pool, bytes + 16))) return rc;
	Stager st(ctx);
	if ((rc = st.stage(bytes, 0)) || (rc = st.h2d(ctx->d_pool.p, pool, bytes))) return rc;
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream)); // `pool` may be freed by the caller on return
	ctx->pool_resident = true, ctx->pool_bytes = bytes;
	return BMH_OK;
}

// internal hooks for host/chain2aln_batch.c (C cannot see inside bmh_ctx)
const bmh_params_t *bmh_ctx_params_(const bmh_ctx_t *ctx) { return ctx && ctx->have_params ? &ctx->params : nullptr; }
// ... and for host/tls_ctx.c: tasks the int32 extension kernel received over this context's host-buffer calls
int64_t bmh_ctx_wide_tasks_(const bmh_ctx_t *ctx) { return ctx ? ctx->wide_total : 0; }
int64_t bmh_ctx_glong_tasks_(const bmh_ctx_t *ctx)
{
	int64_t t = 0;
	float ms;
	return ctx && bmh_global_long_stats(ctx, &t, &ms) == BMH_OK ? t : 0;
}
int64_t bmh_ctx_swl_tasks_(const bmh_ctx_t *ctx)
{
	int64_t t = 0;
	float ms;
	return ctx && bmh_sw_wide_stats(ctx, &t, &ms) == BMH_OK ? t : 0;
}
void bmh_ctx_set_driver_stats_(bmh_ctx_t *ctx, const bmh_driver_stats_t *st)
{
	if (ctx && st) ctx->dstats = *st;
}

// ------------------------------------------------------------------ fused per-seed extension (row a5)

int bmh_seedext_batch_device(bmh_ctx_t *ctx, const uint8_t *d_pool, const bmh_seed_task_t *d_tasks, int64_t n,
                             bmh_seed_result_t *d_res)
{
	if (!ctx || n < 0 || (n > 0 && (!d_pool || !d_tasks || !d_res))) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	if (n > 0x7fffffffLL) return BMH_E_ARG;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	return launch_seedext(ctx, d_pool, d_tasks, n, d_res, ctx->qcap);
}

static int validate_seeds(bmh_ctx *ctx, const bmh_seed_task_t *t, int64_t n, size_t pool_bytes, int *qmax)
{
	int qm = 1;
	const int smax = std::max(ctx->dev.max_mat, ctx->params.a);
	for (int64_t k = 0; k < n; ++k) {
		const bmh_seed_task_t &x = t[k];
		const int64_t rq = (int64_t)x.l_query - x.qbeg - x.len, rt = (int64_t)x.wlen - x.rbeg - x.len;
		const bool tp = x.flags & BMH_F_TPAC;
		if (tp && !ctx->dev.pac) {
			ctx->last_error = "seed " + std::to_string(k) + " has BMH_F_TPAC but no reference was uploaded (bmh_ctx_set_pac)";
			return BMH_E_ARG;
		}
		if (x.l_query < 1 || x.qbeg < 0 || x.len < 1 || rq < 0 || x.rbeg < 0 || rt < 0 || x.wlen < 0) {
			ctx->last_error = "seed " + std::to_string(k) + " does not lie inside its read and window";
			return BMH_E_ARG;
		}
		const uint64_t tspace = tp ? (uint64_t)(ctx->dev.l_pac << 1) : (uint64_t)pool_bytes;
		if (x.q_off + (uint64_t)x.l_query > pool_bytes || x.t_off + (uint64_t)x.wlen > tspace) {
			ctx->last_error = "seed " + std::to_string(k) + " reads outside the sequence pool";
			return BMH_E_ARG;
		}
		if (x.qbeg > 65535 || rq > 65535 || x.rbeg > 65535 || rt > 65535) {
			ctx->last_error = "seed " + std::to_string(k) + ": flank longer than 65535";
			return BMH_E_RANGE;
		}
		if (!ctx->wide_ext && (int64_t)x.l_query * smax > kScoreLimit) {
			ctx->last_error = "seed " + std::to_string(k) + ": l_query*max(max(mat), a) exceeds the 16-bit score range";
			return BMH_E_RANGE;
		}
		if (ctx->wide_ext && (int64_t)x.l_query * smax > kWideScoreLimit) {
			ctx->last_error = "seed " + std::to_string(k) + ": l_query*max(max(mat), a) exceeds the wide extension's score range (2^24)";
			return BMH_E_RANGE;
		}
		qm = std::max(qm, std::max(x.qbeg, (int)rq));
	}
	*qmax = qm;
	return BMH_OK;
}

int bmh_seedext_submit(bmh_ctx_t *ctx, const bmh_seed_task_t *tasks, int64_t n)
{
	if (!ctx || n < 0 || (n > 0 && !tasks)) return BMH_E_ARG;
	if (!ctx->have_params || !ctx->pool_resident || ctx->seed_pending_n >= 0) return BMH_E_ARG;
	if (n > 0x7fffffffLL) return BMH_E_ARG;
	int qmax = 1, rc;
	if ((rc = validate_seeds(ctx, tasks, n, ctx->pool_bytes, &qmax))) return rc;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	const size_t tb = (size_t)n * sizeof(bmh_seed_task_t), rb = (size_t)n * sizeof(bmh_seed_result_t);
	if ((rc = ensure(ctx, ctx->d_tasks, tb + 64)) || (rc = ensure(ctx, ctx->d_res, rb + 64))) return rc;
	if ((rc = ensure_host(ctx, ctx->h_up, tb + 256)) || (rc = ensure_host(ctx, ctx->h_down, rb + 256))) return rc;
	if (n > 0) {
		memcpy(ctx->h_up.p, tasks, tb);
		uint8_t *cnt = (uint8_t *)ctx->h_down.p + ((rb + 63) & ~(size_t)63);
		Stager st(ctx); // (not staged: both ends are pinned already)
		rc = st.h2d(ctx->d_tasks.p, ctx->h_up.p, tb);
		if (!rc)
			rc = launch_seedext(ctx, (const uint8_t *)ctx->d_pool.p, (const bmh_seed_task_t *)ctx->d_tasks.p, n, (bmh_seed_result_t *)ctx->d_res.p,
			                    qmax);
		if (!rc) rc = st.d2h(ctx->h_down.p, ctx->d_res.p, rb);
		if (!rc) rc = st.d2h(cnt, seedext_counters(ctx), 16);
		if (!rc && ctx->wide_last) rc = st.d2h(cnt + 16, ctx->d_wide_stat, 8); // (behind the four list lengths: what the wide bin received)
		if (rc) return st.end(rc); // (on success bmh_seedext_wait waits)
	}
	ctx->seed_pending_n = n;
	return BMH_OK;
}

int bmh_seedext_wait(bmh_ctx_t *ctx, bmh_seed_result_t *results)
{
	if (!ctx || ctx->seed_pending_n < 0 || (ctx->seed_pending_n > 0 && !results)) return BMH_E_ARG;
	const int64_t n = ctx->seed_pending_n;
	ctx->seed_pending_n = -1;
	if (n == 0) return BMH_OK;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	const int rc = fetch_err(ctx); // synchronises
	const size_t rb = (size_t)n * sizeof(bmh_seed_result_t);
	memcpy(results, ctx->h_down.p, rb);
	const uint32_t *c = (const uint32_t *)((const uint8_t *)ctx->h_down.p + ((rb + 63) & ~(size_t)63));
	ctx->sstats.seeds = n, ctx->sstats.left_tasks = c[0], ctx->sstats.left_retries = c[1], ctx->sstats.right_tasks = c[2],
	ctx->sstats.right_retries = c[3];
	if (ctx->wide_last) {
		unsigned long long w;
		memcpy(&w, c + 4, sizeof(w));
		ctx->wide_total += (long long)w;
	}
	return rc;
}

int bmh_seedext_batch(bmh_ctx_t *ctx, const uint8_t *pool, size_t pool_bytes, const bmh_seed_task_t *tasks, int64_t n,
                      bmh_seed_result_t *results)
{
	if (!ctx || n < 0 || (n > 0 && (!tasks || !results))) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	if (n == 0) return BMH_OK;
	int rc;
	if (pool && (rc = bmh_upload_pool(ctx, pool, pool_bytes))) return rc;
	GateGuard gate;
	if ((rc = bmh_seedext_submit(ctx, tasks, n))) return rc;
	return bmh_seedext_wait(ctx, results);
}

int bmh_seedext_stats(const bmh_ctx_t *ctx, bmh_seedext_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->sstats;
	return BMH_OK;
}

// ------------------------------------------------------------------ global

struct GlbShape {
	int qmax = 1, tmax = 1, wmax = 0, wraw = 0; // (qmax, tmax, wmax: of the tasks with qlen <= kGlbLdsQcap)
	GlbLongShape lg;                            // ... and of the longer ones, bin 4's
	size_t cig_lo = ~(size_t)0, cig_hi = 0; // the words of the CIGAR pool the tasks may write
};
static int validate_glb(bmh_ctx *ctx, const bmh_glb_task_t *tasks, int64_t n, size_t pool_bytes, bool have_cigar_pool, size_t cigar_words, GlbShape *o)
{
	GlbShape g;
	for (int64_t k = 0; k < n; ++k) {
		const bmh_glb_task_t &x = tasks[k];
		if (x.q_off + x.qlen > pool_bytes || x.t_off + x.tlen > pool_bytes || x.w < 0 ||
		    (x.cigar_cap && (!have_cigar_pool || (size_t)x.cigar_off + x.cigar_cap > cigar_words))) {
			ctx->last_error = "global task " + std::to_string(k) + " has out-of-range offsets";
			return BMH_E_ARG;
		}
		if (x.qlen <= kGlbLdsQcap) {
			g.qmax = std::max(g.qmax, (int)x.qlen), g.tmax = std::max(g.tmax, (int)x.tlen);
			g.wmax = std::max(g.wmax, std::min(x.w, (int)x.qlen)); // only min(qlen,2w+1) columns are ever stored
		} else { // (a superset of what the device sends to bin 4: it only sizes that launch)
			g.lg.qmax = std::max(g.lg.qmax, (int)x.qlen), g.lg.tmax = std::max(g.lg.tmax, (int)x.tlen);
			g.lg.wmax = std::max(g.lg.wmax, std::min(x.w, (int)x.qlen)), ++g.lg.n;
		}
		g.wraw = std::max(g.wraw, x.w); // ... but the device bins the tasks by their w as given
		if (x.cigar_cap) g.cig_lo = std::min(g.cig_lo, (size_t)x.cigar_off), g.cig_hi = std::max(g.cig_hi, (size_t)x.cigar_off + x.cigar_cap);
	}
	*o = g;
	return BMH_OK;
}

int bmh_global_batch_device(bmh_ctx_t *ctx, const uint8_t *d_pool, const bmh_glb_task_t *d_tasks, int64_t n,
                            bmh_glb_result_t *d_res, uint32_t *d_cigar, const uint32_t *d_order)
{
	if (!ctx || n < 0 || (n > 0 && (!d_pool || !d_tasks || !d_res))) return BMH_E_ARG;
	if (!ctx->glb_params) return BMH_E_ARG;
	if (n > 0xffffffffLL) return BMH_E_ARG;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	// no host view of the tasks: size for the context's capacity hint (square band-limited matrix); a capacity past the LDS
	// row's sends the longer tasks to bin 4, sized by the same hints
	const int whint = std::max(ctx->params.w * 4, 100), q2 = std::min(ctx->qcap, kGlbLdsQcap);
	GlbLongShape lg;
	if (ctx->qcap > kGlbLdsQcap) lg.qmax = ctx->qcap, lg.tmax = ctx->qcap + 2 * ctx->params.w + 64, lg.wmax = whint, lg.n = n;
	return launch_global(ctx, d_pool, d_tasks, n, d_res, d_cigar, d_order, q2, q2 + 2 * ctx->params.w + 64, whint, whint, &lg);
}

int bmh_global_batch(bmh_ctx_t *ctx, const uint8_t *pool, size_t pool_bytes, const bmh_glb_task_t *tasks, int64_t n,
                     bmh_glb_result_t *results, uint32_t *cigar_pool, size_t cigar_words)
{
	if (!ctx || n < 0 || (n > 0 && (!tasks || !results))) return BMH_E_ARG;
	if (!ctx->glb_params) return BMH_E_ARG;
	if (n == 0) return BMH_OK;
	if (n > 0xffffffffLL) return BMH_E_ARG;
	if (!pool && !ctx->pool_resident) return BMH_E_ARG; // (null: the pool left on the device by bmh_upload_pool())
	GlbShape gs;
	int rc;
	if ((rc = validate_glb(ctx, tasks, n, pool ? pool_bytes : ctx->pool_bytes, cigar_pool != nullptr, cigar_words, &gs))) return rc;
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Stager st(ctx);
	const CigarDown cig{cigar_words, cigar_pool, 0, cigar_words};
	return st.end(enqueue_batch(
	    st, true, pool, pool_bytes, tasks, n, results,
	    [&](bmh_ctx *c, auto p, auto t, auto r) { return launch_global(c, p, t, n, r, (uint32_t *)c->d_cigar.p, nullptr, gs.qmax, gs.tmax, gs.wmax, gs.wraw, &gs.lg); },
	    &cig));
}

// ------------------------------------------------------------------ the region record (bwa_gen_cigar2 around ksw_global2)

// where region_cigar_round left the round's arrays on the device, for the long round behind it
struct RegionRoundDev {
	const bmh_region_req_t *reqs;
	bmh_region_res_t *res;
	const uint32_t *cig;
};

// bmh_region_cigar_batch: checks, one enqueue, one wait.  `what` names the caller in the error text.
static int region_cigar_round(bmh_ctx_t *ctx, const char *what, const uint8_t *readpool, size_t readpool_bytes, size_t opool_bytes,
                              const bmh_region_req_t *reqs, int64_t n_req, const bmh_glb_task_t *tasks, int64_t n_tasks, size_t task_cigar_words,
                              int cig_cap, int md_cap, bmh_region_res_t *results, uint32_t *cigar_out, char *md_out, RegionRoundDev *dev)
{
	if (!ctx || n_req < 0 || n_tasks < 0 || cig_cap < 1 || md_cap < 1) return BMH_E_ARG;
	if (n_req > 0 && (!readpool || !reqs || !results || !cigar_out || !md_out)) return BMH_E_ARG;
	if (n_tasks > 0 && !tasks) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	if (!ctx->dev.pac) {
		ctx->last_error = std::string(what) + " needs the resident reference (bmh_ctx_set_pac)";
		return BMH_E_ARG;
	}
	if (n_req == 0) return BMH_OK;
	if (n_req > 0x7fffffffLL || n_tasks > 0xffffffffLL) return BMH_E_ARG;
	const int64_t l_pac = ctx->dev.l_pac;
	for (int64_t k = 0; k < n_req; ++k) { // every byte the kernels will address
		const bmh_region_req_t &r = reqs[k];
		bool ok = r.ql >= 1 && r.tl >= 1 && r.ql <= 65535 && r.tl <= 65535 && r.q_src + (uint64_t)r.ql <= readpool_bytes &&
		          r.o_off + (uint64_t)r.ql + (uint64_t)r.tl <= opool_bytes && r.rb >= 0 && r.rb + r.tl <= l_pac << 1 &&
		          !(r.rb < l_pac && r.rb + r.tl > l_pac);
		const int nt = r.truesc == INT32_MIN ? 1 : 3;
		if (ok && r.task[0] >= 0)
			for (int t = 0; t < nt; ++t) ok = ok && r.task[t] >= 0 && r.task[t] < n_tasks;
		if (ok && r.task[0] < 0) ok = r.ql == r.tl;
		if (!ok) {
			ctx->last_error = "region " + std::to_string(k) + " is outside its pools, the reference or the task list";
			return BMH_E_ARG;
		}
	}
	GlbShape gs;
	int rc;
	if (n_tasks > 0 && (rc = validate_glb(ctx, tasks, n_tasks, opool_bytes, true, task_cigar_words, &gs))) return rc;
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Stager st(ctx);
	rc = st.end([&]() -> int {
		// device pool = [oriented copies | the query windows as uploaded]
		const size_t rpool_off = (opool_bytes + 16 + 63) & ~(size_t)63;
		ctx->pool_resident = false;
		if ((rc = ensure(ctx, ctx->d_pool, rpool_off + readpool_bytes + 16))) return rc;
		if ((rc = ensure(ctx, ctx->d_tasks, (size_t)std::max<int64_t>(n_tasks, 1) * sizeof(bmh_glb_task_t)))) return rc;
		if ((rc = ensure(ctx, ctx->d_res, (size_t)std::max<int64_t>(n_tasks, 1) * sizeof(bmh_glb_result_t)))) return rc;
		if ((rc = ensure(ctx, ctx->d_cigar, (task_cigar_words + 4) * 4))) return rc;
		const size_t req_b = ((size_t)n_req * sizeof(bmh_region_req_t) + 255) & ~(size_t)255;
		const size_t res_b = ((size_t)n_req * sizeof(bmh_region_res_t) + 255) & ~(size_t)255;
		const size_t cig_b = ((size_t)n_req * (size_t)cig_cap * 4 + 255) & ~(size_t)255;
		const size_t md_b = ((size_t)n_req * (size_t)md_cap + 255) & ~(size_t)255;
		if ((rc = ensure(ctx, ctx->d_region, req_b + res_b + cig_b + md_b))) return rc;
		uint8_t *d_reg = (uint8_t *)ctx->d_region.p;
		bmh_region_req_t *d_reqs = (bmh_region_req_t *)d_reg;
		bmh_region_res_t *d_rres = (bmh_region_res_t *)(d_reg + req_b);
		uint32_t *d_cout = (uint32_t *)(d_reg + req_b + res_b);
		char *d_md = (char *)(d_reg + req_b + res_b + cig_b);
		if ((rc = st.stage(readpool_bytes + 64 + (size_t)n_req * sizeof(bmh_region_req_t) + 64 + (size_t)n_tasks * sizeof(bmh_glb_task_t) + 64,
		                   res_b + cig_b + md_b)))
			return rc;
		if ((rc = st.h2d((uint8_t *)ctx->d_pool.p + rpool_off, readpool, readpool_bytes))) return rc;
		if ((rc = st.h2d(d_reqs, reqs, (size_t)n_req * sizeof(bmh_region_req_t)))) return rc;
		if (n_tasks > 0 && (rc = st.h2d(ctx->d_tasks.p, tasks, (size_t)n_tasks * sizeof(bmh_glb_task_t)))) return rc;
		if ((rc = launch_region_orient(ctx, (uint8_t *)ctx->d_pool.p, rpool_off, d_reqs, n_req))) return rc;
		if (n_tasks > 0 && (rc = launch_global(ctx, (const uint8_t *)ctx->d_pool.p, (const bmh_glb_task_t *)ctx->d_tasks.p, n_tasks,
		                                       (bmh_glb_result_t *)ctx->d_res.p, (uint32_t *)ctx->d_cigar.p, nullptr, gs.qmax, gs.tmax, gs.wmax, gs.wraw, &gs.lg)))
			return rc;
		if ((rc = launch_region_finish(ctx, (const uint8_t *)ctx->d_pool.p, d_reqs, n_req, (const bmh_glb_task_t *)ctx->d_tasks.p,
		                               (const bmh_glb_result_t *)ctx->d_res.p, (const uint32_t *)ctx->d_cigar.p, d_rres, d_cout, cig_cap, d_md, md_cap)))
			return rc;
		if (dev) dev->reqs = d_reqs, dev->res = d_rres, dev->cig = d_cout;
		if ((rc = st.d2h(results, d_rres, (size_t)n_req * sizeof(bmh_region_res_t)))) return rc;
		if ((rc = st.d2h(cigar_out, d_cout, (size_t)n_req * (size_t)cig_cap * 4))) return rc;
		return st.d2h(md_out, d_md, (size_t)n_req * (size_t)md_cap);
	}());
	return rc == BMH_E_CIGAR_CAP ? BMH_OK : rc; // a task that outgrew its slots is reported per region (BMH_REGION_CIGAR_CUT)
}

int bmh_region_cigar_batch(bmh_ctx_t *ctx, const uint8_t *readpool, size_t readpool_bytes, size_t opool_bytes, const bmh_region_req_t *reqs,
                           int64_t n_req, const bmh_glb_task_t *tasks, int64_t n_tasks, size_t task_cigar_words, int cig_cap, int md_cap,
                           bmh_region_res_t *results, uint32_t *cigar_out, char *md_out)
{
	return region_cigar_round(ctx, "bmh_region_cigar_batch", readpool, readpool_bytes, opool_bytes, reqs, n_req, tasks, n_tasks, task_cigar_words,
	                          cig_cap, md_cap, results, cigar_out, md_out, nullptr);
}

// ---- ... and the regions that round flags, finished behind it (region_long.hip).  The round's device arrays stay where they are:
// d_pool (the oriented copies), d_tasks, d_res and d_region are read, the long round's own buffers are d_rlong, d_lcig and d_lmd.
enum { kLongGuard = BMH_REGION_LONG_GUARD }; // bytes behind each dense pool, set before the kernels run and brought back with it: they must come back as set

static int region_long_round(bmh_ctx_t *ctx, const RegionRoundDev &D, const bmh_region_req_t *reqs, int64_t n_req, const bmh_glb_task_t *tasks,
                             int cig_cap, const bmh_region_res_t *rr, int64_t n_long, int64_t n_cut, uint64_t words, RegionLongEnt *ent,
                             uint32_t **cig_, char **md_, uint64_t *md_bytes_)
{
	GlbShape gs; // the host's maxima over the flagged regions' tries: the rerun's tasks are among them
	for (int64_t k = 0; k < n_req; ++k) {
		if (!(rr[k].flags & BMH_REGION_CIGAR_CUT) || reqs[k].task[0] < 0) continue;
		for (int t = 0; t < (reqs[k].truesc == INT32_MIN ? 1 : 3); ++t) {
			const bmh_glb_task_t &x = tasks[reqs[k].task[t]];
			if (x.qlen <= kGlbLdsQcap) {
				gs.qmax = std::max(gs.qmax, (int)x.qlen), gs.tmax = std::max(gs.tmax, (int)x.tlen);
				gs.wmax = std::max(gs.wmax, std::min(x.w, (int)x.qlen));
			} else {
				gs.lg.qmax = std::max(gs.lg.qmax, (int)x.qlen), gs.lg.tmax = std::max(gs.lg.tmax, (int)x.tlen);
				gs.lg.wmax = std::max(gs.lg.wmax, std::min(x.w, (int)x.qlen));
			}
			gs.wraw = std::max(gs.wraw, x.w);
		}
		if (reqs[k].ql > kGlbLdsQcap) ++gs.lg.n;
	}
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	uint32_t *h_cig = nullptr;
	char *h_md = nullptr;
	Stager st(ctx);
	int rc = [&]() -> int {
		int rc;
		const size_t nb = (size_t)((n_req + 255) / 256) + 1; // block sums of the widest scan, and its total
		const size_t o_ent = (nb * sizeof(RegionLongSum) + 255) & ~(size_t)255;
		const size_t o_task = o_ent + (((size_t)n_long * sizeof(RegionLongEnt) + 255) & ~(size_t)255);
		const size_t o_res = o_task + (((size_t)std::max<int64_t>(n_cut, 1) * sizeof(bmh_glb_task_t) + 255) & ~(size_t)255);
		const size_t total = o_res + (size_t)std::max<int64_t>(n_cut, 1) * sizeof(bmh_glb_result_t);
		if ((rc = ensure(ctx, ctx->d_rlong, total)) || (rc = ensure(ctx, ctx->d_lcig, (size_t)words * 4 + kLongGuard))) return rc;
		uint8_t *dl = (uint8_t *)ctx->d_rlong.p;
		RegionLongSum *d_bsum = (RegionLongSum *)dl;
		RegionLongEnt *d_ent = (RegionLongEnt *)(dl + o_ent);
		bmh_glb_task_t *d_lt = (bmh_glb_task_t *)(dl + o_task);
		bmh_glb_result_t *d_lr = (bmh_glb_result_t *)(dl + o_res);
		uint32_t *d_lcig = (uint32_t *)ctx->d_lcig.p;
		const uint8_t *d_pool = (const uint8_t *)ctx->d_pool.p;
		const bool tm = ctx->timing;
		if (tm)
			for (auto &e : ctx->ev_rlong)
				if (!e) BMH_HIP(ctx, hipEventCreate(&e));
		if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_rlong[0], ctx->stream));
		BMH_HIP(ctx, hipMemsetAsync(d_lcig + words, 0xA5, kLongGuard, ctx->stream));
		if ((rc = launch_region_long_list(ctx, D.reqs, D.res, n_req, (const bmh_glb_result_t *)ctx->d_res.p, d_bsum, d_ent, n_long))) return rc;
		if ((rc = launch_region_long_tasks(ctx, d_ent, n_long, d_bsum, (const bmh_glb_task_t *)ctx->d_tasks.p, d_lt, n_cut, words))) return rc;
		if (n_cut > 0 && (rc = launch_global(ctx, d_pool, d_lt, n_cut, d_lr, d_lcig, nullptr, gs.qmax, gs.tmax, gs.wmax, gs.wraw, &gs.lg))) return rc;
		if ((rc = launch_region_long_sizes(ctx, d_pool, D.reqs, d_ent, n_long, d_lr, D.cig, cig_cap, d_lcig, d_bsum))) return rc;
		if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_rlong[1], ctx->stream));
		// first wait: the MD pool's size
		const size_t nbe = (size_t)((n_long + 255) / 256);
		if ((rc = ensure_host(ctx, ctx->h_down, 256))) return rc;
		BMH_HIP(ctx, hipMemcpyAsync(ctx->h_down.p, d_bsum + nbe, sizeof(RegionLongSum), hipMemcpyDeviceToHost, ctx->stream));
		BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
		const uint64_t md_bytes = ((const RegionLongSum *)ctx->h_down.p)->a;
		if (md_bytes > (uint64_t)n_long * (3ull * 131070 + 16)) { // (more than any walk can write: the device's error word says why)
			ctx->last_error = "the long round's MD sizes are not credible";
			return BMH_E_ARG;
		}
		if ((rc = ensure(ctx, ctx->d_lmd, (size_t)md_bytes + kLongGuard))) return rc;
		char *d_lmd = (char *)ctx->d_lmd.p;
		h_cig = (uint32_t *)malloc((size_t)words * 4 + kLongGuard);
		h_md = (char *)malloc((size_t)md_bytes + kLongGuard);
		if (!h_cig || !h_md) return BMH_E_NOMEM;
		if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_rlong[2], ctx->stream));
		BMH_HIP(ctx, hipMemsetAsync(d_lmd + md_bytes, 0xA5, kLongGuard, ctx->stream));
		if ((rc = launch_region_long_md(ctx, d_pool, D.reqs, d_ent, n_long, d_lcig, d_bsum, d_lmd, md_bytes))) return rc;
		if (tm) BMH_HIP(ctx, hipEventRecord(ctx->ev_rlong[3], ctx->stream));
		// second wait: the download
		if ((rc = st.stage(0, (size_t)n_long * sizeof(RegionLongEnt) + (size_t)words * 4 + (size_t)md_bytes + 2 * kLongGuard + 256))) return rc;
		if ((rc = st.d2h(ent, d_ent, (size_t)n_long * sizeof(RegionLongEnt)))) return rc;
		if ((rc = st.d2h(h_cig, d_lcig, (size_t)words * 4 + kLongGuard))) return rc;
		if ((rc = st.d2h(h_md, d_lmd, (size_t)md_bytes + kLongGuard))) return rc;
		*md_bytes_ = md_bytes;
		return BMH_OK;
	}();
	rc = st.end(rc);
	if (!rc && ctx->timing) {
		float m0 = 0.f, m1 = 0.f;
		hipError_t e = hipEventElapsedTime(&m0, ctx->ev_rlong[0], ctx->ev_rlong[1]);
		if (e == hipSuccess) e = hipEventElapsedTime(&m1, ctx->ev_rlong[2], ctx->ev_rlong[3]);
		if (e != hipSuccess) rc = set_hip_error(ctx, e, "hipEventElapsedTime(long round)");
		ctx->rlong_ms = m0 + m1;
	}
	if (rc) {
		free(h_cig), free(h_md);
		return rc;
	}
	*cig_ = h_cig, *md_ = h_md;
	return BMH_OK;
}

int bmh_region_cigar_batch_long(bmh_ctx_t *ctx, const uint8_t *readpool, size_t readpool_bytes, size_t opool_bytes, const bmh_region_req_t *reqs,
                                int64_t n_req, const bmh_glb_task_t *tasks, int64_t n_tasks, size_t task_cigar_words, int cig_cap, int md_cap,
                                bmh_region_res_t *results, uint32_t *cigar_out, char *md_out, bmh_region_long_t **longs, int64_t *n_long,
                                uint32_t **long_cigar, char **long_md)
{
	if (!ctx || !longs || !n_long || !long_cigar || !long_md) return BMH_E_ARG;
	if (n_req < 0 || n_tasks < 0 || cig_cap < 1 || md_cap < 1) return BMH_E_ARG;
	if (n_req > 0 && (!readpool || !reqs || !results || !cigar_out || !md_out)) return BMH_E_ARG;
	if (n_tasks > 0 && !tasks) return BMH_E_ARG;
	// the round's outputs go to the caller only once the whole call has succeeded
	const size_t rb = (size_t)n_req * sizeof(bmh_region_res_t), cb = (size_t)n_req * (size_t)cig_cap * 4, mb = (size_t)n_req * (size_t)md_cap;
	bmh_region_res_t *rr = (bmh_region_res_t *)malloc(rb + 1);
	uint32_t *tc = (uint32_t *)malloc(cb + 4);
	char *tmd = (char *)malloc(mb + 1);
	RegionLongEnt *ent = nullptr;
	bmh_region_long_t *lg = nullptr;
	uint32_t *h_cig = nullptr;
	char *h_md = nullptr;
	int64_t nl = 0, n_cut = 0;
	uint64_t words = 0, md_bytes = 0;
	RegionRoundDev D{nullptr, nullptr, nullptr};
	int rc = rr && tc && tmd ? BMH_OK : BMH_E_NOMEM;
	if (!rc)
		rc = region_cigar_round(ctx, "bmh_region_cigar_batch_long", readpool, readpool_bytes, opool_bytes, reqs, n_req, tasks, n_tasks,
		                        task_cigar_words, cig_cap, md_cap, rr, tc, tmd, &D);
	for (int64_t k = 0; !rc && k < n_req; ++k)
		if (rr[k].flags) {
			++nl, words += (uint64_t)(rr[k].n_cigar > 0 ? rr[k].n_cigar : 0);
			if (rr[k].flags & BMH_REGION_CIGAR_CUT) ++n_cut;
		}
	if (!rc && words > 0xffffffffull) { // the rerun's tasks address the pool through the uint32 cigar_off
		ctx->last_error = "the flagged regions' CIGARs have " + std::to_string(words) + " words: more than one call's pool can address";
		rc = BMH_E_RANGE;
	}
	if (!rc && nl > 0) {
		ent = (RegionLongEnt *)malloc((size_t)nl * sizeof(RegionLongEnt));
		lg = (bmh_region_long_t *)malloc((size_t)nl * sizeof(bmh_region_long_t));
		if (!ent || !lg) rc = BMH_E_NOMEM;
		if (!rc) rc = region_long_round(ctx, D, reqs, n_req, tasks, cig_cap, rr, nl, n_cut, words, ent, &h_cig, &h_md, &md_bytes);
		for (int64_t e = 0; !rc && e < nl; ++e) { // the entries are the flagged regions in ascending order, each inside the two pools
			const RegionLongEnt &x = ent[e];
			if (x.bad || x.region < 0 || x.region >= n_req || (e > 0 && x.region <= ent[e - 1].region) || !rr[x.region].flags ||
			    x.n_cigar != rr[x.region].n_cigar || x.cigar_off + (uint64_t)x.n_cigar > words || x.md_len < 0 ||
			    x.md_off + (uint64_t)x.md_len > md_bytes) {
				ctx->last_error = "the long round's entry " + std::to_string(e) + " is inconsistent";
				rc = BMH_E_ARG;
			}
		}
		for (int g = 0; !rc && g < kLongGuard; ++g)
			if (((const uint8_t *)h_cig)[words * 4 + g] != 0xA5 || ((const uint8_t *)h_md)[md_bytes + g] != 0xA5) {
				ctx->last_error = "the long round wrote behind one of its pools";
				rc = BMH_E_HIP;
			}
	}
	if (rc) {
		free(rr), free(tc), free(tmd), free(ent), free(lg), free(h_cig), free(h_md);
		return rc;
	}
	for (int64_t e = 0; e < nl; ++e) {
		const RegionLongEnt &x = ent[e];
		bmh_region_res_t &r = rr[x.region];
		r.NM = x.NM, r.md_len = x.md_len, r.flags |= BMH_REGION_LONG;
		lg[e].region = x.region, lg[e].cigar_off = x.cigar_off, lg[e].md_off = x.md_off;
	}
	if (n_req > 0) memcpy(results, rr, rb), memcpy(cigar_out, tc, cb), memcpy(md_out, tmd, mb);
	*longs = lg, *n_long = nl, *long_cigar = h_cig, *long_md = h_md;
	ctx->rlong_regions = nl, ctx->rlong_words = (long long)words, ctx->rlong_md = (long long)md_bytes;
	if (nl == 0 || !ctx->timing) ctx->rlong_ms = nl == 0 && ctx->timing ? 0.f : -1.f;
	free(rr), free(tc), free(tmd), free(ent);
	return BMH_OK;
}

int bmh_last_region_long_stats(const bmh_ctx_t *ctx, int64_t *regions, int64_t *cigar_words, int64_t *md_bytes, float *kernel_ms)
{
	if (!ctx || !regions || !cigar_words || !md_bytes || !kernel_ms) return BMH_E_ARG;
	*regions = ctx->rlong_regions, *cigar_words = ctx->rlong_words, *md_bytes = ctx->rlong_md, *kernel_ms = ctx->rlong_ms;
	return BMH_OK;
}

int bmh_ctx_set_region_long(bmh_ctx_t *ctx, int on)
{
	if (!ctx) return BMH_E_ARG;
	ctx->region_long = on != 0;
	return BMH_OK;
}

// internal hooks for host/reg2cigar_batch.c: the switch, and the counts of its last call
int bmh_ctx_region_long_(const bmh_ctx_t *ctx) { return ctx && ctx->region_long; }
void bmh_ctx_set_reg2cigar_stats_(bmh_ctx_t *ctx, int64_t regions, int64_t long_device, int64_t redone_host)
{
	if (ctx) ctx->r2c_regions = regions, ctx->r2c_long_device = long_device, ctx->r2c_redone_host = redone_host;
}

int bmh_last_reg2cigar_stats(const bmh_ctx_t *ctx, int64_t *regions, int64_t *long_device, int64_t *redone_host)
{
	if (!ctx || !regions || !long_device || !redone_host) return BMH_E_ARG;
	*regions = ctx->r2c_regions, *long_device = ctx->r2c_long_device, *redone_host = ctx->r2c_redone_host;
	return BMH_OK;
}

// ------------------------------------------------------------------ local Smith-Waterman (ksw_align2)

int bmh_sw_batch_device(bmh_ctx_t *ctx, const uint8_t *d_pool, const bmh_sw_task_t *d_tasks, int64_t n,
                        bmh_sw_result_t *d_res)
{
	if (!ctx || n < 0 || (n > 0 && (!d_pool || !d_tasks || !d_res))) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	if (n > 0xffffffffLL) return BMH_E_ARG;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	return launch_sw(ctx, d_pool, d_tasks, n, d_res, -1, -1, -1);
}

static int validate_sw(bmh_ctx *ctx, const bmh_sw_task_t *tasks, int64_t n, size_t pool_bytes, int *qmax_, int *tmax_, int *qmin_)
{
	int qmax = 1, tmax = 1, qmin = 65535;
	const bool wraps = sw_byte_gaps_wrap(ctx->params);
	for (int64_t k = 0; k < n; ++k) {
		const bmh_sw_task_t &x = tasks[k];
		qmin = std::min(qmin, (int)x.qlen);
		const bool qr = x.flags & BMH_F_QREV, tr = x.flags & BMH_F_TREV, tp = x.flags & BMH_F_TPAC;
		const uint64_t qlo = qr ? x.q_off - (x.qlen ? x.qlen - 1 : 0) : x.q_off;
		const uint64_t tlo = tr ? x.t_off - (x.tlen ? x.tlen - 1 : 0) : x.t_off;
		const uint64_t tspace = tp ? (uint64_t)(ctx->dev.l_pac << 1) : (uint64_t)pool_bytes;
		if (tp && !ctx->dev.pac) {
			ctx->last_error = "task " + std::to_string(k) + " has BMH_F_TPAC but no reference was uploaded (bmh_ctx_set_pac)";
			return BMH_E_ARG;
		}
		if ((qr && x.qlen && x.q_off + 1 < x.qlen) || (tr && x.tlen && x.t_off + 1 < x.tlen) || qlo + x.qlen > pool_bytes ||
		    tlo + x.tlen > tspace || x.tlen > 0x7fffffffu) {
			ctx->last_error = "Smith-Waterman task " + std::to_string(k) + " reads outside the sequence pool";
			return BMH_E_ARG;
		}
		// (with bmh_ctx_set_wide_sw on, word mode takes any query: sw_long_kernel restates ksw_i16's saturation)
		const bool wide = ctx->wide_sw && !(x.xtra & BMH_SW_XBYTE);
		if (x.qlen < 1 || (!wide && (int64_t)x.qlen * ctx->dev.max_mat >= kScoreLimit)) {
			ctx->last_error = "Smith-Waterman task " + std::to_string(k) + ": qlen must be >= 1 and qlen*max(mat) below the 16-bit score range";
			return BMH_E_RANGE;
		}
		if (wraps && (x.xtra & BMH_SW_XBYTE)) {
			ctx->last_error = "Smith-Waterman task " + std::to_string(k) + ": byte mode needs o_del+e_del and o_ins+e_ins below 256";
			return BMH_E_RANGE;
		}
		qmax = std::max(qmax, (int)x.qlen), tmax = std::max(tmax, (int)x.tlen);
	}
	*qmax_ = qmax, *tmax_ = tmax, *qmin_ = qmin;
	return BMH_OK;
}

int bmh_sw_batch(bmh_ctx_t *ctx, const uint8_t *pool, size_t pool_bytes, const bmh_sw_task_t *tasks, int64_t n,
                 bmh_sw_result_t *results)
{
	if (!ctx || n < 0 || (n > 0 && (!tasks || !results))) return BMH_E_ARG;
	if (!ctx->have_params) return BMH_E_ARG;
	if (n == 0) return BMH_OK;
	if (n > 0xffffffffLL) return BMH_E_ARG;
	if (!pool && !ctx->pool_resident) return BMH_E_ARG; // (null: the pool left on the device by bmh_upload_pool())
	int qmax = 1, tmax = 1, qmin = 65535, rc;
	if ((rc = validate_sw(ctx, tasks, n, pool ? pool_bytes : ctx->pool_bytes, &qmax, &tmax, &qmin))) return rc;
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Stager st(ctx);
	return st.end(enqueue_batch(st, true, pool, pool_bytes, tasks, n, results, [&](bmh_ctx *c, auto p, auto t, auto r) {
		return launch_sw(c, p, t, n, r, qmax, tmax, qmin);
	}));
}

// ------------------------------------------------------------------ static shards of one batch over several contexts
// One contiguous slice of the tasks per context (one context per GPU), every device given the whole sequence pool (offsets stay
// valid); no collective, no device-to-device traffic.  The same split as kt_for_batch's ranges (reference kthread_batch.c:44-56,
// bwamem.c:1313).  Every shard is validated on the host before anything is enqueued anywhere, so a refused call has no effect;
// then, inside one device gate, each shard's batch is enqueued with direct copies on its context's stream before any of them is
// waited for, and every context served leaves through Stager::end, whatever happened.  Returns the first error.
} // extern "C"
template <class Validate, class Enqueue>
static int run_sharded(bmh_ctx_t *const *ctxs, int n_ctx, int64_t n, Validate validate, Enqueue enqueue)
{
	if (!ctxs || n_ctx < 1 || n < 0) return BMH_E_ARG;
	for (int g = 0; g < n_ctx; ++g)
		if (!ctxs[g] || !ctxs[g]->have_params) return BMH_E_ARG;
	if (n == 0) return BMH_OK;
	const auto lo = [=](int g) { return n * g / n_ctx; };
	int rc;
	for (int g = 0; g < n_ctx; ++g)
		if (lo(g + 1) > lo(g) && (rc = validate(ctxs[g], (size_t)g, lo(g), lo(g + 1) - lo(g)))) return rc;
	GateGuard gate;
	std::vector<Stager> st((size_t)n_ctx);
	int failed = BMH_OK, g = 0;
	for (; g < n_ctx && !failed; ++g)
		if (lo(g + 1) > lo(g)) {
			st[(size_t)g] = Stager(ctxs[g]);
			const hipError_t e = hipSetDevice(ctxs[g]->device);
			failed = e != hipSuccess ? set_hip_error(ctxs[g], e, "hipSetDevice") : enqueue(st[(size_t)g], (size_t)g, lo(g), lo(g + 1) - lo(g));
		}
	int first = failed;
	for (int h = 0; h < g; ++h) // (g - 1: the context whose enqueue failed, if one did)
		if (lo(h + 1) > lo(h)) {
			const hipError_t e = hipSetDevice(ctxs[h]->device);
			rc = st[(size_t)h].end(h == g - 1 ? failed : BMH_OK);
			if (!first) first = e != hipSuccess ? set_hip_error(ctxs[h], e, "hipSetDevice") : rc;
		}
	return first;
}

extern "C" {
int bmh_extend_batch_sharded(bmh_ctx_t *const *ctxs, int n_ctx, const uint8_t *pool, size_t pool_bytes, const bmh_ext_task_t *tasks, int64_t n,
                             bmh_ext_result_t *results)
{
	if (n > 0 && (!pool || !tasks || !results)) return BMH_E_ARG;
	std::vector<int> qmax((size_t)std::max(n_ctx, 0));
	return run_sharded(
	    ctxs, n_ctx, n, [&](bmh_ctx *c, size_t g, int64_t lo, int64_t m) { return validate_ext(c, tasks + lo, m, pool_bytes, &qmax[g]); },
	    [&](Stager &st, size_t g, int64_t lo, int64_t m) {
		    st.wide = true;
		    return enqueue_batch(st, false, pool, pool_bytes, tasks + lo, m, results + lo, [&](bmh_ctx *c, auto p, auto t, auto r) {
			    return launch_extend(c, p, t, m, r, nullptr, qmax[g]);
		    });
	    });
}

int bmh_seedext_batch_sharded(bmh_ctx_t *const *ctxs, int n_ctx, const uint8_t *pool, size_t pool_bytes, const bmh_seed_task_t *tasks,
                              int64_t n, bmh_seed_result_t *results)
{
	if (n > 0 && (!pool || !tasks || !results)) return BMH_E_ARG;
	std::vector<int> qmax((size_t)std::max(n_ctx, 0));
	return run_sharded(
	    ctxs, n_ctx, n,
	    [&](bmh_ctx *c, size_t g, int64_t lo, int64_t m) { return m > 0x7fffffffLL ? BMH_E_ARG : validate_seeds(c, tasks + lo, m, pool_bytes, &qmax[g]); },
	    [&](Stager &st, size_t g, int64_t lo, int64_t m) {
		    return enqueue_batch(st, false, pool, pool_bytes, tasks + lo, m, results + lo, [&](bmh_ctx *c, auto p, auto t, auto r) {
			    return launch_seedext(c, p, t, m, r, qmax[g]);
		    });
	    });
}

int bmh_sw_batch_sharded(bmh_ctx_t *const *ctxs, int n_ctx, const uint8_t *pool, size_t pool_bytes, const bmh_sw_task_t *tasks, int64_t n,
                         bmh_sw_result_t *results)
{
	if (n > 0 && (!pool || !tasks || !results)) return BMH_E_ARG;
	struct SwShape {
		int qmax = 1, tmax = 1, qmin = 65535;
	};
	std::vector<SwShape> shape((size_t)std::max(n_ctx, 0));
	return run_sharded(
	    ctxs, n_ctx, n,
	    [&](bmh_ctx *c, size_t g, int64_t lo, int64_t m) {
		    SwShape &s = shape[g];
		    return validate_sw(c, tasks + lo, m, pool_bytes, &s.qmax, &s.tmax, &s.qmin);
	    },
	    [&](Stager &st, size_t g, int64_t lo, int64_t m) {
		    return enqueue_batch(st, false, pool, pool_bytes, tasks + lo, m, results + lo, [&](bmh_ctx *c, auto p, auto t, auto r) {
			    return launch_sw(c, p, t, m, r, shape[g].qmax, shape[g].tmax, shape[g].qmin);
		    });
	    });
}

int bmh_global_batch_sharded(bmh_ctx_t *const *ctxs, int n_ctx, const uint8_t *pool, size_t pool_bytes, const bmh_glb_task_t *tasks, int64_t n,
                             bmh_glb_result_t *results, uint32_t *cigar_pool, size_t cigar_words)
{
	if (n > 0 && (!pool || !tasks || !results)) return BMH_E_ARG;
	// a shard's CIGAR words come back into a buffer of its own first: the ranges of two shards may interleave in the caller's pool, and a
	// device only holds what its own tasks wrote
	std::vector<std::vector<uint32_t>> back((size_t)std::max(n_ctx, 0));
	std::vector<GlbShape> shape((size_t)std::max(n_ctx, 0));
	const int rc = run_sharded(
	    ctxs, n_ctx, n,
	    [&](bmh_ctx *c, size_t g, int64_t lo, int64_t m) {
		    return m > 0xffffffffLL ? BMH_E_ARG : validate_glb(c, tasks + lo, m, pool_bytes, cigar_pool != nullptr, cigar_words, &shape[g]);
	    },
	    [&](Stager &st, size_t g, int64_t lo, int64_t m) {
		    const GlbShape &gs = shape[g];
		    back[g].resize(gs.cig_hi > gs.cig_lo ? gs.cig_hi - gs.cig_lo : 0);
		    const CigarDown cig{cigar_words, back[g].data(), gs.cig_lo, back[g].size()};
		    return enqueue_batch(
		        st, false, pool, pool_bytes, tasks + lo, m, results + lo,
		        [&](bmh_ctx *c, auto p, auto t, auto r) { return launch_global(c, p, t, m, r, (uint32_t *)c->d_cigar.p, nullptr, gs.qmax, gs.tmax, gs.wmax, gs.wraw, &gs.lg); },
		        &cig);
	    });
	if (rc && rc != BMH_E_CIGAR_CAP && rc != BMH_E_RANGE) return rc; // (a flagged task: the other tasks' results are still delivered)
	for (int g = 0; g < n_ctx && n > 0; ++g) {
		const int64_t lo = n * g / n_ctx, hi = n * (g + 1) / n_ctx;
		if (back[(size_t)g].empty()) continue;
		for (int64_t k = lo; k < hi; ++k) {
			const bmh_glb_task_t &x = tasks[k];
			const size_t nw = std::min<size_t>((size_t)std::max(results[k].n_cigar, 0), x.cigar_cap);
			if (nw) memcpy(cigar_pool + x.cigar_off, back[(size_t)g].data() + ((size_t)x.cigar_off - shape[(size_t)g].cig_lo), nw * 4);
		}
	}
	return rc;
}

int bmh_ctx_reserve_staging(bmh_ctx_t *ctx, size_t upload_bytes, size_t download_bytes)
{
	if (!ctx) return BMH_E_ARG;
	int rc;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = ensure_host(ctx, ctx->h_up, upload_bytes)) || (rc = ensure_host(ctx, ctx->h_down, download_bytes))) return rc;
	return BMH_OK;
}

int bmh_ctx_reserve_device(bmh_ctx_t *ctx, size_t pool_bytes, int64_t max_tasks, size_t cigar_words)
{
	if (!ctx || max_tasks < 0) return BMH_E_ARG;
	int rc;
	const size_t N = (size_t)max_tasks;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	if (ctx->glb_narrow && (1 + (size_t)kSortBins) * N + 16 > ctx->d_gband.cap) ctx->gband_n = 0; // (growing drops the last launch's bands)
	if ((16 + (size_t)kSortBins * kSortKeysHost + (N + 1) / 2 + 1 + (size_t)kSortBins * N) * 4 > ctx->d_bins.cap) ctx->gbins_valid = false; // (... and its bin sizes)
	if ((rc = ensure(ctx, ctx->d_pool, pool_bytes + 16)) || (rc = ensure(ctx, ctx->d_tasks, N * 40 + 64)) || (rc = ensure(ctx, ctx->d_res, N * 32 + 64)) ||
	    (rc = ensure(ctx, ctx->d_cigar, (cigar_words + 4) * 4)) ||
	    (rc = ensure(ctx, ctx->d_bins, (16 + (size_t)kSortBins * kSortKeysHost + (N + 1) / 2 + 1 + (size_t)kSortBins * N) * 4)) ||
	    (ctx->glb_narrow && (rc = ensure(ctx, ctx->d_gband, (1 + (size_t)kSortBins) * N + 16))))
		return rc;
	return BMH_OK;
}

int bmh_ctx_reserve_kernels(bmh_ctx_t *ctx, int seed_reads, int seed_read_len, int64_t global_tasks, int global_rows)
{
	if (!ctx || seed_reads < 0 || seed_read_len < 0 || global_tasks < 0 || global_rows < 0) return BMH_E_ARG;
	int rc;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	if (seed_reads > 0) { // the SMEM kernels' interval stacks (fmindex.hip): three per lane, read length + 2 entries of 32 bytes each
		const size_t grid = std::min<size_t>(((size_t)seed_reads + 63) / 64, 1024 * 4);
		if ((rc = ensure(ctx, ctx->d_sw, grid * 3 * ((size_t)seed_read_len + 2) * 64 * 32))) return rc;
	}
	if (global_tasks > 0) { // the lane kernels' direction slab (global_lane.hip): resident waves x rows x 8 blocks x 256 bytes
		const size_t grid = std::min<size_t>(((size_t)global_tasks + 63) / 64, (size_t)std::max(ctx->ncu, 1) * 4 * 2);
		if ((rc = ensure(ctx, ctx->d_zslab, grid * (size_t)std::min(global_rows, 512) * 8 * 256))) return rc; // (global_narrow.hip: four times the waves, two blocks each: the same)
	}
	return BMH_OK;
}

// ------------------------------------------------------------------ mem_sort_and_dedup

int bmh_sort_dedup_batch(bmh_ctx_t *ctx, int n_reads, bmh_alnreg_v *regs, float mask_level_redun)
{
	if (!ctx || n_reads < 0 || (n_reads > 0 && !regs)) return BMH_E_ARG;
	size_t total = 0;
	for (int r = 0; r < n_reads; ++r) {
		if (regs[r].n && !regs[r].a) return BMH_E_ARG;
		if (regs[r].n > 0x7fffffffu - total) {
			ctx->last_error = "bmh_sort_dedup_batch: more than 2^31-1 regions in the batch";
			return BMH_E_ARG;
		}
		total += regs[r].n;
	}
	if (total == 0) { // nothing to launch
		ctx->dedup_in = ctx->dedup_out = 0, ctx->dedup_ms = -1.f;
		return BMH_OK;
	}
	// one upload: [removed, padding | off[n_reads + 1] | cnt[n_reads] | the regions], laid out the same on both sides
	const size_t nr = (size_t)n_reads, o_off = 64, o_cnt = o_off + (nr + 1) * 8, o_reg = (o_cnt + nr * 8 + 63) & ~(size_t)63;
	const size_t b_reg = total * sizeof(bmh_alnreg_t), b_up = o_reg + b_reg, b_down = b_up - o_cnt;
	std::vector<uint8_t> up, down;
	try {
		up.resize(b_up), down.resize(b_down);
	} catch (const std::bad_alloc &) {
		ctx->last_error = "bmh_sort_dedup_batch: out of host memory";
		return BMH_E_NOMEM;
	}
	memset(up.data(), 0, o_off);
	unsigned long long *off = (unsigned long long *)(up.data() + o_off), *cnt = (unsigned long long *)(up.data() + o_cnt);
	size_t at = 0;
	for (int r = 0; r < n_reads; ++r) {
		off[r] = at, cnt[r] = regs[r].n;
		if (regs[r].n) memcpy(up.data() + o_reg + at * sizeof(bmh_alnreg_t), regs[r].a, regs[r].n * sizeof(bmh_alnreg_t));
		at += regs[r].n;
	}
	off[n_reads] = at;
	memset(up.data() + o_cnt + nr * 8, 0, o_reg - (o_cnt + nr * 8));
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Stager st(ctx);
	unsigned long long removed = 0;
	int rc = [&]() -> int {
		int e;
		if ((e = ensure(ctx, ctx->d_dedup, b_up)) || (e = st.stage(b_up, b_down + 64))) return e;
		uint8_t *d = (uint8_t *)ctx->d_dedup.p;
		if ((e = st.h2d(d, up.data(), b_up))) return e;
		if ((e = launch_region_dedup(ctx, (bmh_alnreg_t *)(d + o_reg), (const unsigned long long *)(d + o_off), (unsigned long long *)(d + o_cnt), n_reads,
		                             (unsigned long long)total, mask_level_redun, (unsigned long long *)d, ctx->d_err)))
			return e;
		if ((e = st.d2h(down.data(), d + o_cnt, b_down)) || (e = st.d2h(&removed, d, 8))) return e;
		return BMH_OK;
	}();
	if ((rc = st.end(rc))) return rc;
	// the survivors lie at the start of each slice; a and m stay the caller's
	const unsigned long long *kept = (const unsigned long long *)down.data();
	const uint8_t *ra = down.data() + (o_reg - o_cnt);
	for (int r = 0; r < n_reads; ++r) {
		if (regs[r].n <= 1) continue;
		if (kept[r] > regs[r].n) { // cannot happen
			ctx->last_error = "bmh_sort_dedup_batch: the device's counts are inconsistent";
			return BMH_E_ARG;
		}
		memcpy(regs[r].a, ra + (size_t)off[r] * sizeof(bmh_alnreg_t), (size_t)kept[r] * sizeof(bmh_alnreg_t));
		regs[r].n = (size_t)kept[r];
	}
	ctx->dedup_in = (long long)total, ctx->dedup_out = (long long)(total - removed), ctx->dedup_ms = -1.f;
	if (ctx->timing) BMH_HIP(ctx, hipEventElapsedTime(&ctx->dedup_ms, ctx->ev_dedup[0], ctx->ev_dedup[1]));
	return BMH_OK;
}

int bmh_ctx_set_regs_dedup(bmh_ctx_t *ctx, int on, float mask_level_redun)
{
	if (!ctx) return BMH_E_ARG;
	ctx->regs_dedup = on != 0, ctx->regs_dedup_mask = mask_level_redun;
	return BMH_OK;
}

int bmh_last_dedup_stats(const bmh_ctx_t *ctx, int64_t *regions_in, int64_t *regions_out, float *kernel_ms)
{
	if (!ctx) return BMH_E_ARG;
	if (regions_in) *regions_in = ctx->dedup_in;
	if (regions_out) *regions_out = ctx->dedup_out;
	if (kernel_ms) *kernel_ms = ctx->dedup_ms;
	return BMH_OK;
}

// ------------------------------------------------------------------ mem_pestat's pair walk (pestat.hip)

int bmh_pestat_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, int64_t l_pac, int n, const bmh_alnreg_v *regs, uint32_t *cand)
{
	if (!ctx || !o || l_pac < 0 || n < 0 || (n > 0 && !regs) || (n > 1 && !cand)) return BMH_E_ARG;
	const int np = n >> 1, n_reads = np << 1; // an odd n ignores the last read, as the reference's n>>1 does
	size_t total = 0;
	for (int r = 0; r < n_reads; ++r) {
		if (regs[r].n && !regs[r].a) return BMH_E_ARG;
		if (regs[r].n > 0x7fffffffu - total) {
			ctx->last_error = "bmh_pestat_device: more than 2^31-1 regions in the batch";
			return BMH_E_ARG;
		}
		total += regs[r].n;
	}
	if (o->max_ins > BMH_PS_MAX_INS) {
		ctx->last_error = "bmh_pestat_device: max_ins must be below 2^30, the word carries the orientation above it";
		return BMH_E_RANGE;
	}
	if (np) memset(cand, 0, (size_t)np * sizeof(uint32_t));
	if (total == 0) return BMH_OK; // nothing to launch: no pair of empty vectors is a candidate
	// device block: [the words | off[n_reads + 1] | cnt[n_reads] | the regions]; everything behind the words goes up in one copy
	const size_t nr = (size_t)n_reads, o_off = ((size_t)np * 4 + 63) & ~(size_t)63, o_cnt = o_off + (nr + 1) * 8, o_reg = (o_cnt + nr * 8 + 63) & ~(size_t)63;
	const size_t b_up = o_reg - o_off + total * sizeof(bmh_alnreg_t);
	std::vector<uint8_t> up;
	try {
		up.resize(b_up);
	} catch (const std::bad_alloc &) {
		ctx->last_error = "bmh_pestat_device: out of host memory";
		return BMH_E_NOMEM;
	}
	unsigned long long *off = (unsigned long long *)up.data(), *cnt = (unsigned long long *)(up.data() + (o_cnt - o_off));
	size_t at = 0;
	for (int r = 0; r < n_reads; ++r) {
		off[r] = at, cnt[r] = regs[r].n;
		if (regs[r].n) memcpy(up.data() + (o_reg - o_off) + at * sizeof(bmh_alnreg_t), regs[r].a, regs[r].n * sizeof(bmh_alnreg_t));
		at += regs[r].n;
	}
	off[n_reads] = at;
	memset(up.data() + (o_cnt - o_off) + nr * 8, 0, o_reg - (o_cnt + nr * 8));
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Stager st(ctx);
	const int rc = [&]() -> int {
		int e;
		if ((e = ensure(ctx, ctx->d_pestat, o_off + b_up)) || (e = st.stage(b_up, (size_t)np * 4 + 64))) return e;
		uint8_t *d = (uint8_t *)ctx->d_pestat.p;
		if ((e = st.h2d(d + o_off, up.data(), b_up))) return e;
		if ((e = launch_pestat_collect(ctx, (bmh_alnreg_t *)(d + o_reg), (const unsigned long long *)(d + o_off), (unsigned long long *)(d + o_cnt), nullptr, n_reads,
		                               (unsigned long long)total, *o, l_pac, 0, false, (uint32_t *)d, nullptr, ctx->d_err)))
			return e;
		return st.d2h(cand, d, (size_t)np * 4);
	}();
	return st.end(rc);
}

int bmh_ctx_set_regs_drop_exact(bmh_ctx_t *ctx, int on)
{
	if (!ctx) return BMH_E_ARG;
	ctx->regs_drop_exact = on != 0;
	return BMH_OK;
}

int bmh_ctx_set_pestat_collect(bmh_ctx_t *ctx, int on, const bmh_sam_opt_t *o)
{
	if (!ctx || (on && !o)) return BMH_E_ARG;
	ctx->pestat_collect = on != 0;
	if (on) ctx->pestat_opt = *o;
	return BMH_OK;
}

int bmh_last_pestat_candidates(bmh_ctx_t *ctx, uint32_t *cand, int64_t n_pairs, float *kernel_ms)
{
	if (!ctx) return BMH_E_ARG;
	if (ctx->regs_drop_exact && !ctx->pestat_collect) {
		ctx->last_error = "bmh_last_pestat_candidates: the collect switch is off (bmh_ctx_set_pestat_collect)";
		return BMH_E_ARG;
	}
	if (ctx->pestat_pairs < 0 || n_pairs != (int64_t)ctx->pestat_pairs || (n_pairs > 0 && !cand)) {
		ctx->last_error = ctx->pestat_pairs < 0 ? "bmh_last_pestat_candidates: no collecting call has been made on this context"
		                                        : "bmh_last_pestat_candidates: n_pairs is not the last collecting call's pair count";
		return BMH_E_ARG;
	}
	if (n_pairs) memcpy(cand, ctx->pestat_cand.data(), (size_t)n_pairs * sizeof(uint32_t));
	if (kernel_ms) *kernel_ms = ctx->pestat_ms;
	return BMH_OK;
}

int bmh_last_drop_exact_stats(const bmh_ctx_t *ctx, int64_t *removed)
{
	if (!ctx) return BMH_E_ARG;
	if (removed) *removed = ctx->drop_exact_removed;
	return BMH_OK;
}

// ------------------------------------------------------------------ pass A of phase 2 (decide.hip)

// the tables' entries, made by the compiler and libm of the host routines (host/sam_post.c)
void bmh_pp_fill_log_(double *logk, int64_t k0, int64_t k1);
void bmh_pp_fill_term_(const bmh_sam_opt_t *o, const bmh_pestat_t *pes, const int64_t term_off[4], double *term);

// What the tables of a pass A on the device must reach (bwamem_hip.h), before anything is uploaded: BMH_E_RANGE and *why where one
// would pass 2^20 entries or an index is negative.  plan: the regions' part of it (host/handoff_core.h), from a walk over the caller's
// vectors (decide_table_sizes below) or from table_plan_kernel where the regions are on the device; pair_kmax: what the pairs add, 0 = none
static int decide_tables_from_plan(const bmh_sam_opt_t *o, const bmh_pestat_t *pes, const bmh_ho_plan_t &plan, long long pair_kmax, long long *kmax_,
                                   long long *n_term_, int64_t term_off[4], const char **why)
{
	const bool pairing = (o->flag & BMH_MEM_F_PE) && !(o->flag & BMH_MEM_F_NOPAIRING);
	const long long kmax = std::max<long long>(plan.kmax, pair_kmax);
	long long n_term = 0;
	auto refuse = [&](const char *w) {
		*why = w;
		return BMH_E_RANGE;
	};
	if (plan.neg) return refuse("bmh_decide_device: a region asks for the logarithm of a negative number");
	if (kmax + 1 > BMH_HO_TAB_MAX) return refuse("bmh_decide_device: the log table would pass 2^20 entries");
	if (pairing)
		for (int d = 0; d < 4; ++d) {
			term_off[d] = n_term, n_term += bmh_pp_term_len(&pes[d]);
			if (n_term > BMH_HO_TAB_MAX) return refuse("bmh_decide_device: the pair table would pass 2^20 entries");
		}
	*kmax_ = kmax, *n_term_ = n_term;
	return BMH_OK;
}

// ... for the caller's vectors; *opool_cap (may be null): the sum of oriented_cap over all of them
static int decide_table_sizes(const bmh_sam_opt_t *o, const bmh_pestat_t *pes, int n, const bmh_alnreg_v *regs, long long *kmax_, long long *n_term_,
                              int64_t term_off[4], const char **why, size_t *opool_cap = nullptr)
{
	const bool pe = (o->flag & BMH_MEM_F_PE) != 0;
	bmh_ho_plan_t plan = BMH_HO_PLAN_INIT;
	int64_t pair_kmax = BMH_HO_PAIRS_INIT;
	for (int i = 0; i < n; ++i) {
		bmh_ho_read(o, regs[i].a, (int64_t)regs[i].n, &plan);
		// the paired-end clause as table_plan_kernel folds it: a first mate raises the fold to its pair's bmh_ho_pair_kmax(n0, n1)
		if (pe && bmh_ho_first_mate(i, n)) bmh_ho_pair((int64_t)regs[i].n, (int64_t)regs[i + 1].n, &pair_kmax);
	}
	if (opool_cap) *opool_cap = (size_t)plan.opool_cap;
	return decide_tables_from_plan(o, pes, plan, pair_kmax, kmax_, n_term_, term_off, why);
}

// the host's copy of the log table up to kmax, grown in powers of two; *want_log = the entries the device's copy must have
static int decide_host_log(bmh_ctx *ctx, long long kmax, long long *want_log_)
{
	long long want_log = ctx->logk_n;
	if (kmax + 1 > ctx->logk_n) {
		for (want_log = 1 << 17; want_log < kmax + 1; want_log <<= 1) {}
		if (want_log > ctx->logk_host_n) {
			double *t = (double *)realloc(ctx->h_logk, sizeof(double) * (size_t)want_log);
			if (!t) {
				ctx->last_error = "bmh_decide_device: out of host memory";
				return BMH_E_NOMEM;
			}
			bmh_pp_fill_log_(t, ctx->logk_host_n, want_log);
			ctx->h_logk = t, ctx->logk_host_n = want_log;
		}
	}
	*want_log_ = want_log;
	return BMH_OK;
}

// offsets into a device block: one section after the other, each 64-byte aligned
struct Block {
	size_t at = 0;
	size_t take(size_t bytes)
	{
		const size_t o = at;
		at += (bytes + 63) & ~(size_t)63;
		return o;
	}
};

struct HostBuf { // malloc'd (zero: calloc'd), freed on the way out
	uint8_t *p = nullptr;
	HostBuf() = default;
	explicit HostBuf(size_t bytes, bool zero = false) { alloc(bytes, zero); }
	~HostBuf() { free(p); }
	HostBuf(const HostBuf &) = delete;
	uint8_t *alloc(size_t bytes, bool zero = false) { return p = (uint8_t *)(zero ? calloc(bytes, 1) : malloc(bytes)); }
};

// the bases of a slice's reads
static size_t reads_total(int n, const bmh_read_t *reads)
{
	return std::accumulate(reads, reads + n, (size_t)0, [](size_t b, const bmh_read_t &r) { return b + (size_t)r.l_seq; });
}

// the flat copy of a slice in an upload block: every read's regions to entry roff[i] of reg and, n_want not NULL, its wanted indices to wk's
static void slice_copy_flat(int n, const bmh_alnreg_v *regs, const int64_t *roff, uint8_t *reg, const int32_t *n_want = nullptr, const int32_t *want_k = nullptr, uint8_t *wk = nullptr)
{
	for (int i = 0; i < n; ++i) {
		if (n_want && n_want[i]) memcpy(wk + (size_t)roff[i] * 4, want_k + roff[i], (size_t)n_want[i] * 4);
		if (regs[i].n) memcpy(reg + (size_t)roff[i] * sizeof(bmh_alnreg_t), regs[i].a, regs[i].n * sizeof(bmh_alnreg_t));
	}
}

// what the text calls answer for n == 0: an empty text, text_off[0] = 0
static int empty_text(char **text, int64_t *text_off)
{
	char *p = (char *)malloc(1);
	if (!p) return BMH_E_NOMEM;
	*text = p, text_off[0] = 0;
	return BMH_OK;
}

// the statistics of the phase 2 calls as a call that has done nothing leaves them
static void reset_decide_stats(bmh_ctx *ctx) { ctx->decide_units = 0, ctx->decide_fallbacks = 0, ctx->decide_ms = -1.f; }
static void reset_wanted_stats(bmh_ctx *ctx) { ctx->wanted_n = 0, ctx->wanted_fixed = 0, ctx->wanted_redone = 0, ctx->wanted_ms = -1.f; }
static void reset_phase2_stats(bmh_ctx *ctx)
{
	ctx->p2 = bmh_phase2_stats_t{};
	ctx->p2.decide_ms = ctx->p2.wanted_ms = -1.f;
}
static void reset_phase2_text_stats(bmh_ctx *ctx)
{
	ctx->pt = bmh_phase2_text_stats_t{};
	ctx->pt.decide_ms = ctx->pt.wanted_ms = ctx->pt.gather_ms = ctx->pt.size_ms = ctx->pt.emit_ms = -1.f;
}
static void reset_samtext_stats(bmh_ctx *ctx)
{
	ctx->stx = bmh_samtext_stats_t{};
	ctx->stx.size_ms = ctx->stx.emit_ms = -1.f;
}

// the tables a device call was prepared with: bns's sequence table and, where the call reads the reference, pac
static int need_resident(bmh_ctx *ctx, const char *who, const bmh_refidx_t *bns, const uint8_t *pac)
{
	if (pac && (!ctx->dev.pac || ctx->h_pac != pac || ctx->dev.l_pac != bns->l_pac)) {
		ctx->last_error = std::string(who) + " needs the resident reference (bmh_ctx_set_pac)";
		return BMH_E_ARG;
	}
	if (ctx->refidx_n == 0 || ctx->refidx_n != bns->n_seqs || ctx->refidx_l_pac != bns->l_pac) {
		ctx->last_error = std::string(who) + " needs the resident sequence table (bmh_ctx_set_refidx)";
		return BMH_E_ARG;
	}
	return BMH_OK;
}

// what decide_table_sizes and decide_host_log found for one slice
struct DecideTables {
	long long kmax = 1, n_term = 0, want_log = 0;
	int64_t term_off[4] = {0, 0, 0, 0};
};

// Pass A's device block, the offsets at 0: [offsets | opt + pes | read offsets | WantedHdr | pair table | regions] up, [regions | reg_mapq |
// want_k | n_want | pd] down (the regions come last in the upload so that the download is one copy), then decide_kernel's two scratch
// arrays.  The read offsets and the WantedHdr are pass B's, there for the fused session and empty without it.
struct DecideBlock {
	size_t hdr, soff, whdr, term, reg, mq, wk, nw, pd, z, v, end;
	size_t up() const { return mq; }
	size_t down() const { return z - reg; }
};

static DecideBlock decide_block(size_t n, size_t total, size_t n_term, bool pe, bool with_pass_b)
{
	Block b;
	DecideBlock L;
	b.take((n + 1) * 8);
	L.hdr = b.take(sizeof(DecideHdr));
	L.soff = b.take(with_pass_b ? (n + 1) * 8 : 0), L.whdr = b.take(with_pass_b ? sizeof(WantedHdr) : 0);
	L.term = b.take(n_term * 8), L.reg = b.take(total * sizeof(bmh_alnreg_t));
	L.mq = b.take(total * 4), L.wk = b.take(total * 4), L.nw = b.take(n * 4), L.pd = b.take(pe ? (n >> 1) * sizeof(bmh_pairdec_t) : 0);
	L.z = b.take(total * 4), L.v = b.take(pe ? total * sizeof(bmh_pair64_t) : 0), L.end = b.at;
	return L;
}

// pass A's sections of the upload: offsets, DecideHdr, pair table, regions (roff NULL: neither the offsets nor the regions, which
// are on the device already)
static void decide_fill(uint8_t *up, const DecideBlock &L, const bmh_sam_opt_t *o, const bmh_pestat_t *pes, const DecideTables &T, int n,
                        const bmh_alnreg_v *regs, const int64_t *roff)
{
	if (roff) memcpy(up, roff, ((size_t)n + 1) * 8);
	DecideHdr *hdr = (DecideHdr *)(up + L.hdr);
	memset(hdr, 0, sizeof(*hdr));
	hdr->opt = *o;
	if (o->flag & BMH_MEM_F_PE) memcpy(hdr->pes, pes, sizeof(hdr->pes));
	if (T.n_term) bmh_pp_fill_term_(o, pes, T.term_off, (double *)(up + L.term));
	if (roff) slice_copy_flat(n, regs, roff, up + L.reg);
}

// Stages a session that moves up_bytes and down_bytes beside the log table, and brings the device's copy of the table to want_log
// entries.  ctx->logk_n says so only once the session has succeeded: the caller sets it.
static int decide_stage_log(bmh_ctx *ctx, Stager &st, long long want_log, size_t up_bytes, size_t down_bytes)
{
	const bool grow = want_log > ctx->logk_n;
	const size_t bytes = (size_t)want_log * 8;
	int e;
	if (grow) ctx->logk_n = 0; // (ensure may drop the old table)
	if ((e = ensure(ctx, ctx->d_logk, (size_t)std::max(want_log, 1LL) * 8)) || (e = st.stage(up_bytes + (grow ? bytes + 64 : 0), down_bytes))) return e;
	return grow ? st.h2d(ctx->d_logk.p, ctx->h_logk, bytes) : BMH_OK;
}

static DecideArgs decide_args(bmh_ctx *ctx, uint8_t *d, const DecideBlock &L, const DecideTables &T, size_t total, int64_t l_pac, int64_t id0, int n,
                              bool pe)
{
	DecideArgs A{};
	A.roff = (const unsigned long long *)d, A.hdr = (const DecideHdr *)(d + L.hdr);
	A.tab.logk = (const double *)ctx->d_logk.p, A.tab.term = (const double *)(d + L.term);
	memcpy(A.tab.term_off, T.term_off, sizeof(T.term_off));
	A.tab.n_log = T.want_log, A.tab.n_term = T.n_term;
	A.reg = (bmh_alnreg_t *)(d + L.reg), A.total = total;
	A.reg_mapq = (int32_t *)(d + L.mq), A.want_k = (int32_t *)(d + L.wk), A.n_want = (int32_t *)(d + L.nw), A.pd = (bmh_pairdec_t *)(d + L.pd);
	A.z = (int *)(d + L.z), A.v = (bmh_pair64_t *)(d + L.v);
	A.l_pac = l_pac, A.id0 = id0, A.n = n, A.pe = pe, A.err = ctx->d_err;
	return A;
}

// the wanted regions of the block as downloaded (down = its regions), or -1 where a read wants more than its vector holds (cannot happen)
static int64_t decide_want_count(const uint8_t *down, const DecideBlock &L, int n, const bmh_alnreg_v *regs)
{
	const int32_t *nw = (const int32_t *)(down + (L.nw - L.reg));
	int64_t sum = 0;
	for (int i = 0; i < n; ++i) {
		if (nw[i] < 0 || (size_t)nw[i] > regs[i].n) return -1;
		sum += nw[i];
	}
	return sum;
}

// all or nothing: the caller's vectors and outputs from the checked block, once nothing can fail any more
static void decide_commit(const uint8_t *down, const DecideBlock &L, bool pe, int n, bmh_alnreg_v *regs, const int64_t *roff, bmh_pairdec_t *pd,
                          int32_t *reg_mapq, int32_t *n_want, int32_t *want_k)
{
	const size_t nr = (size_t)n, total = (size_t)roff[n];
	const int32_t *nw = (const int32_t *)(down + (L.nw - L.reg)), *wk = (const int32_t *)(down + (L.wk - L.reg));
	for (int i = 0; i < n; ++i)
		if (regs[i].n) memcpy(regs[i].a, down + (size_t)roff[i] * sizeof(bmh_alnreg_t), regs[i].n * sizeof(bmh_alnreg_t));
	memcpy(reg_mapq, down + (L.mq - L.reg), total * 4), memcpy(n_want, nw, nr * 4);
	for (int i = 0; i < n; ++i) // (entries of want_k past a read's n_want stay the caller's)
		if (nw[i]) memcpy(want_k + roff[i], wk + roff[i], (size_t)nw[i] * 4);
	if (pe) memcpy(pd, down + (L.pd - L.reg), (nr >> 1) * sizeof(bmh_pairdec_t));
}

int bmh_decide_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t *pes, int64_t id0, int n, bmh_alnreg_v *regs,
                      const int64_t *roff, bmh_pairdec_t *pd, int32_t *reg_mapq, int32_t *n_want, int32_t *want_k)
{
	if (!ctx) return BMH_E_ARG;
	int rc = bmh_pp_check_args(o, pes, n, regs, roff, pd, reg_mapq, n_want, want_k);
	if (rc) return rc;
	if (n == 0) {
		reset_decide_stats(ctx);
		return BMH_OK;
	}
	const bool pe = (o->flag & BMH_MEM_F_PE) != 0;
	const size_t total = (size_t)roff[n];
	// what the tables must reach (bwamem_hip.h), before anything is uploaded
	DecideTables T;
	const char *why = nullptr;
	if (decide_table_sizes(o, pes, n, regs, &T.kmax, &T.n_term, T.term_off, &why)) {
		ctx->last_error = why;
		reset_decide_stats(ctx), ctx->decide_fallbacks = 1;
		return BMH_E_RANGE;
	}
	if ((rc = decide_host_log(ctx, T.kmax, &T.want_log))) return rc;
	const DecideBlock L = decide_block((size_t)n, total, (size_t)T.n_term, pe, false);
	HostBuf up(L.up()), down(L.down());
	if (!up.p || !down.p) {
		ctx->last_error = "bmh_decide_device: out of host memory";
		return BMH_E_NOMEM;
	}
	decide_fill(up.p, L, o, pes, T, n, regs, roff);
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Stager st(ctx);
	rc = [&]() -> int {
		int e;
		if ((e = ensure(ctx, ctx->d_decide, L.end)) || (e = decide_stage_log(ctx, st, T.want_log, L.up(), L.down() + 64))) return e;
		uint8_t *d = (uint8_t *)ctx->d_decide.p;
		if ((e = st.h2d(d, up.p, L.up())) || (e = launch_decide(ctx, decide_args(ctx, d, L, T, total, l_pac, id0, n, pe)))) return e;
		return st.d2h(down.p, d + L.reg, L.down());
	}();
	if ((rc = st.end(rc))) return rc;
	ctx->logk_n = T.want_log;
	if (decide_want_count(down.p, L, n, regs) < 0) {
		ctx->last_error = "bmh_decide_device: the device's counts are inconsistent";
		return BMH_E_ARG;
	}
	decide_commit(down.p, L, pe, n, regs, roff, pd, reg_mapq, n_want, want_k);
	reset_decide_stats(ctx), ctx->decide_units = pe ? n >> 1 : n;
	if (ctx->timing) BMH_HIP(ctx, hipEventElapsedTime(&ctx->decide_ms, ctx->ev_decide[0], ctx->ev_decide[1]));
	return BMH_OK;
}

int bmh_ctx_set_decide_device(bmh_ctx_t *ctx, int on)
{
	if (!ctx) return BMH_E_ARG;
	ctx->decide_device = on != 0;
	return BMH_OK;
}

int bmh_last_decide_stats(const bmh_ctx_t *ctx, int64_t *units, int64_t *fallbacks, float *kernel_ms)
{
	if (!ctx) return BMH_E_ARG;
	if (units) *units = ctx->decide_units;
	if (fallbacks) *fallbacks = ctx->decide_fallbacks;
	if (kernel_ms) *kernel_ms = ctx->decide_ms;
	return BMH_OK;
}

// bmh_sam_batch at its entry, before any check of its own: with the switch on the statistics are this call's from here on
__attribute__((visibility("hidden"))) void bmh_decide_stats_reset_(bmh_ctx_t *ctx)
{
	if (ctx && ctx->decide_device) reset_decide_stats(ctx);
	if (ctx && ctx->wanted_device) reset_wanted_stats(ctx);
	if (ctx && ctx->phase2_device) reset_phase2_stats(ctx);
	if (ctx && ctx->samtext_device) reset_samtext_stats(ctx);
	if (ctx && ctx->phase2_text_device) reset_phase2_text_stats(ctx);
}

// bmh_sam_batch's pass A (host/sam_post.c; not part of the interface)
__attribute__((visibility("hidden"))) int bmh_decide_routed_(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t *pes, int64_t id0,
                                                             int n, bmh_alnreg_v *regs, const int64_t *roff, bmh_pairdec_t *pd, int32_t *reg_mapq,
                                                             int32_t *n_want, int32_t *want_k)
{
	if (ctx && ctx->decide_device) {
		// (statistics of THIS call: a slice that never reaches the device call must not leave an earlier slice's on the context)
		reset_decide_stats(ctx);
		const int rc = bmh_decide_device(ctx, o, l_pac, pes, id0, n, regs, roff, pd, reg_mapq, n_want, want_k);
		if (rc != BMH_E_RANGE) return rc;
	}
	return bmh_decide_batch(o, l_pac, pes, id0, n, regs, roff, pd, reg_mapq, n_want, want_k);
}

// ------------------------------------------------------------------ pass B of phase 2 planned on the device (wanted.hip)

// the host form and its helpers (host/sam_post.c; not part of the interface)
int bmh_wanted_host_(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads, const bmh_alnreg_v *regs,
                     const int64_t *roff, const int32_t *n_want, const int32_t *want_k, int64_t n_w, int bands, bmh_wanted_res_t *wr, uint32_t **cig,
                     char **md, int64_t *n_fixed);
int bmh_wanted_deliver_(int64_t n_w, const bmh_wanted_res_t *wr, const uint32_t *cig, const char *md, bmh_wanted_res_t *results, uint32_t *cigar_pool,
                        size_t cigar_words, char *md_pool, size_t md_bytes);
int bmh_wanted_check_args_(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int n, const bmh_read_t *reads, const bmh_alnreg_v *regs,
                           const int64_t *roff, const int32_t *n_want, const int32_t *want_k, int64_t *n_w);

int bmh_ctx_set_refidx(bmh_ctx_t *ctx, const bmh_refidx_t *bns)
{
	if (!ctx) return BMH_E_ARG;
	if (!bns) {
		ctx->refidx_n = 0, ctx->refidx_l_pac = 0, ctx->h_refidx.clear();
		return BMH_OK;
	}
	if (bns->n_seqs <= 0 || !bns->anns || bns->l_pac <= 0) return BMH_E_ARG;
	std::vector<bmh_refspan_t> t((size_t)bns->n_seqs);
	for (int i = 0; i < bns->n_seqs; ++i) t[(size_t)i] = bmh_refspan_t{bns->anns[i].offset, bns->anns[i].len, 0};
	if (ctx->refidx_n == bns->n_seqs && ctx->refidx_l_pac == bns->l_pac && ctx->h_refidx.size() == t.size() &&
	    memcmp(ctx->h_refidx.data(), t.data(), t.size() * sizeof(bmh_refspan_t)) == 0)
		return BMH_OK; // already resident: the same records (16 bytes per sequence to compare, per slice)
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream)); // (nothing in flight reads the table while it is replaced)
	ctx->refidx_n = 0, ctx->h_refidx.clear();
	int rc;
	if ((rc = ensure(ctx, ctx->d_refidx, t.size() * sizeof(bmh_refspan_t)))) return rc;
	BMH_HIP(ctx, hipMemcpy(ctx->d_refidx.p, t.data(), t.size() * sizeof(bmh_refspan_t), hipMemcpyHostToDevice));
	ctx->refidx_n = bns->n_seqs, ctx->refidx_l_pac = bns->l_pac, ctx->h_refidx = std::move(t);
	return BMH_OK;
}

// bytes of MD coming back per region (BMH_RP_MD_SLOT, host/regplan_core.h); round 0's MD is not read
enum { kWantMdSlot = BMH_RP_MD_SLOT, kWantFixMdSlot = 4 };

// one round of the region kernels over what a status record describes (the two device forms of pass B)
static int wanted_run_round(bmh_ctx *ctx, const WantedArgs &A, const WantedStatus &s, int r, uint8_t *d_pool, size_t rpool_off, bmh_region_res_t *res,
                            uint32_t *cig, char *md, int md_cap)
{
	int e2;
	if (s.n_rec <= 0) return BMH_OK;
	GlbLongShape lg;
	lg.qmax = s.lqmax, lg.tmax = s.ltmax, lg.wmax = s.lwmax, lg.n = s.ln;
	if ((e2 = launch_region_orient(ctx, d_pool, rpool_off, A.req[r], s.n_rec))) return e2;
	if (s.n_tasks > 0 && (e2 = launch_global(ctx, d_pool, A.task[r], s.n_tasks, (bmh_glb_result_t *)ctx->d_res.p, (uint32_t *)ctx->d_cigar.p, nullptr,
	                                         std::max(s.qmax, 1), std::max(s.tmax, 1), s.wmax, s.wraw, &lg)))
		return e2;
	return launch_region_finish(ctx, d_pool, A.req[r], s.n_rec, A.task[r], (const bmh_glb_result_t *)ctx->d_res.p, (const uint32_t *)ctx->d_cigar.p, res, cig,
	                            BMH_RP_SMALL_CAP, md, md_cap);
}

// the status records: the only thing the host reads between launches.  The wanted regions are n_lo..n_hi: the count where the host
// knows it, 0..the capacity where pass A left the want list on the device.  The fused sessions' Stager counts the read.  The session
// through to the text (`one`) reads the record of the round just planned alone -- a refused region raises both records' error words,
// both carry n_w, and record 0 is still the host's from the first look -- so that its downloads stay the text's and three small records.
static int wanted_read_status(bmh_ctx *ctx, const uint8_t *d_stat, int64_t n_lo, int64_t n_hi, Stager &st, bool one, int round)
{
	const WantedStatus *hs = (const WantedStatus *)ctx->h_wstat;
	const size_t at = one ? (size_t)round * sizeof(WantedStatus) : 0, bytes = (one ? 1 : 2) * sizeof(WantedStatus);
	BMH_HIP(ctx, hipMemcpyAsync((uint8_t *)ctx->h_wstat + at, d_stat + at, bytes, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	st.waited(bytes);
	const bool both = !one || round == 1; // record 1 has been read
	if (hs[0].err || (both && hs[1].err)) {
		ctx->last_error = "bmh_wanted_cigar_device: a wanted region is outside its read, its vector or the reference, or nothing is left of it";
		return hs[0].err ? hs[0].err : hs[1].err;
	}
	if (hs[0].n_w < n_lo || hs[0].n_w > n_hi || hs[0].n_rec > hs[0].n_w || (both && hs[1].n_rec > hs[0].n_w)) { // cannot happen
		ctx->last_error = "bmh_wanted_cigar_device: the device's counts are inconsistent";
		return BMH_E_ARG;
	}
	return BMH_OK;
}

// ---- Pass B's device session, once.  Two callers feed it: bmh_wanted_cigar_device uploads the want list and the regions in a block of
// its own and knows the number of wanted regions; the fused session points at pass A's block, where decide_kernel left them, and
// knows only a capacity.  The reads, the WantedHdr, the work arrays, the launches, the downloads and the host's tail are the same.

// the oriented bytes a region the kernels accept can have: what a session's oriented pool is sized from before the first launch
static size_t oriented_cap(const bmh_alnreg_t *a) { return (size_t)bmh_ho_oriented_cap(a); }

// the sections of an upload that are pass B's in both forms: the reads as one pool with 16 zero bytes behind it, so[] = its n + 1 offsets
// (q_src = seq_off[read] + qb), and the parameters.  rpool NULL: the offsets and the parameters alone (the pool is made on the device)
static void wanted_fill(const bmh_ctx *ctx, int w, int n, const bmh_read_t *reads, uint64_t *so, WantedHdr *hdr, uint8_t *rpool)
{
	size_t b = 0;
	for (int i = 0; i < n; ++i) {
		so[i] = b;
		if (rpool && reads[i].l_seq) memcpy(rpool + b, reads[i].seq, (size_t)reads[i].l_seq);
		b += (size_t)reads[i].l_seq;
	}
	so[n] = b;
	if (rpool) memset(rpool + b, 0, 16);
	const bmh_params_t &p = ctx->params;
	memset(hdr, 0, sizeof(*hdr));
	hdr->opt = bmh_rp_opt_t{p.a, p.mat[0], p.o_del, p.e_del, p.o_ins, p.e_ins, p.w};
	hdr->fix_w = w;
}

// the work arrays, then what comes down, from where b stands in d_wanted; wc = the capacity in wanted regions
struct WantedBlock {
	size_t first, rec, key[4], sum[4], req[2], stat, res0, cig0, md0, res1, wres, cig1, md1, end;
};

static WantedBlock wanted_block(Block &b, size_t n, size_t wc)
{
	WantedBlock L;
	L.first = b.take((n + 1) * 8), L.rec = b.take(wc * sizeof(WantRec));
	for (int c = 0; c < 4; ++c) L.key[c] = b.take(wc * 4);
	for (int c = 0; c < 4; ++c) L.sum[c] = b.take(wc * 8);
	L.req[0] = b.take(wc * sizeof(bmh_region_req_t)), L.req[1] = b.take(wc * sizeof(bmh_region_req_t)), L.stat = b.take(2 * sizeof(WantedStatus));
	L.res0 = b.take(wc * sizeof(bmh_region_res_t)), L.cig0 = b.take(wc * BMH_RP_SMALL_CAP * 4), L.md0 = b.take(wc * kWantFixMdSlot);
	L.res1 = b.take(wc * sizeof(bmh_region_res_t)), L.wres = b.take(wc * sizeof(bmh_wanted_res_t));
	L.cig1 = b.take(wc * BMH_RP_SMALL_CAP * 4), L.md1 = b.take(wc * kWantMdSlot), L.end = b.at;
	return L;
}

// Every buffer the kernels write, sized before the first launch.  Device pool = [oriented copies | the reads as uploaded], as
// bmh_region_cigar_batch lays it out: *rpool_off = where the reads go.
static int wanted_reserve(bmh_ctx *ctx, size_t wc, size_t opool_cap, size_t reads_bytes, size_t wanted_bytes, size_t *rpool_off)
{
	int e;
	*rpool_off = (opool_cap + 16 + 63) & ~(size_t)63;
	ctx->pool_resident = false;
	if (!ctx->h_wstat) BMH_HIP(ctx, hipHostMalloc(&ctx->h_wstat, 2 * sizeof(WantedStatus), hipHostMallocDefault));
	if ((e = ensure(ctx, ctx->d_pool, *rpool_off + reads_bytes + 16)) || wc == 0) return e;
	if ((e = ensure(ctx, ctx->d_tasks, 4 * wc * sizeof(bmh_glb_task_t))) || (e = ensure(ctx, ctx->d_res, 3 * wc * sizeof(bmh_glb_result_t)))) return e;
	if ((e = ensure(ctx, ctx->d_cigar, (3 * wc * BMH_RP_SMALL_CAP + 4) * 4))) return e;
	return ensure(ctx, ctx->d_wanted, wanted_bytes);
}

// what a session brings down: the records in want order, and the CIGAR and MD slots of the main round's n_rec records
struct WantedDown {
	bmh_wanted_res_t *wres = nullptr;      // n_w; cigar_off = md_off = the record's slot; BMH_WANTED_HOST: no slot, the host redoes it
	uint8_t *cig = nullptr, *md = nullptr; // n_rec slots each, behind the records in the same malloc'd block
	int64_t n_w = 0, n_rec = 0, n_fix = 0; // wanted regions; records of the main round and of round 0
	bool stay = false;                     // the session through to the text: the counts alone, nothing comes down
	~WantedDown() { free(wres); }
};

struct WantedSizes { // what a pass B session is sized from
	size_t total, reads_bytes, wc, opool_cap; // regions, bases, the capacity in wanted regions, the oriented pool's bytes
	int n;
	int64_t l_pac;
};

// a session's inputs where they lie on the device: the offsets, the want list and the regions, the read offsets and the parameters
static WantedArgs wanted_inputs(const void *roff, const int32_t *n_want, const int32_t *want_k, const bmh_alnreg_t *reg, const uint8_t *seq_off, const uint8_t *hdr,
                                const WantedSizes &Z)
{
	WantedArgs A{};
	A.roff = (const unsigned long long *)roff, A.seq_off = (const unsigned long long *)seq_off, A.hdr = (const WantedHdr *)hdr;
	A.n_want = n_want, A.want_k = want_k, A.reg = reg;
	A.total = Z.total, A.reads_bytes = Z.reads_bytes, A.n = Z.n, A.l_pac = Z.l_pac, A.w_cap = Z.wc, A.opool_cap = Z.opool_cap;
	return A;
}

// The launches and the downloads.  A: the inputs as the caller set them -- roff, seq_off, hdr, n_want, want_k and reg where they lie on
// the device, total, reads_bytes, n, l_pac, w_cap, opool_cap; the rest is set here.  dw, L: the session's arrays; n_lo..n_hi: see
// wanted_read_status.  D's arrays (malloc'd here) are written behind st.end().
static int wanted_session(bmh_ctx *ctx, const char *who, Stager &st, WantedArgs A, uint8_t *dw, const WantedBlock &L, size_t rpool_off, int64_t n_lo,
                          int64_t n_hi, WantedDown &D)
{
	const WantedStatus *hs = (const WantedStatus *)ctx->h_wstat;
	uint8_t *d_pool = (uint8_t *)ctx->d_pool.p;
	int e;
	BMH_HIP(ctx, hipMemsetAsync(dw + L.stat, 0, 2 * sizeof(WantedStatus), ctx->stream));
	A.ref = (const bmh_refspan_t *)ctx->d_refidx.p, A.n_seqs = ctx->refidx_n;
	A.first = (unsigned long long *)(dw + L.first), A.rec = (WantRec *)(dw + L.rec);
	for (int c = 0; c < 4; ++c) A.key[c] = (uint32_t *)(dw + L.key[c]), A.sum[c] = (unsigned long long *)(dw + L.sum[c]);
	A.req[0] = (bmh_region_req_t *)(dw + L.req[0]), A.req[1] = (bmh_region_req_t *)(dw + L.req[1]);
	A.task[0] = (bmh_glb_task_t *)ctx->d_tasks.p, A.task[1] = A.task[0] + A.w_cap;
	A.fix_res = (const bmh_region_res_t *)(dw + L.res0), A.fix_cig = (const uint32_t *)(dw + L.cig0);
	A.main_res = (const bmh_region_res_t *)(dw + L.res1), A.wres = (bmh_wanted_res_t *)(dw + L.wres);
	A.status = (WantedStatus *)(dw + L.stat), A.err = ctx->d_err;
	if ((e = launch_wanted_begin(ctx, A)) || (e = wanted_read_status(ctx, dw + L.stat, n_lo, n_hi, st, D.stay, 0))) return e;
	if ((e = wanted_run_round(ctx, A, hs[0], 0, d_pool, rpool_off, (bmh_region_res_t *)(dw + L.res0), (uint32_t *)(dw + L.cig0), (char *)(dw + L.md0), kWantFixMdSlot)))
		return e;
	if ((e = launch_wanted_main(ctx, A)) || (e = wanted_read_status(ctx, dw + L.stat, n_lo, n_hi, st, D.stay, 1))) return e;
	if ((e = wanted_run_round(ctx, A, hs[1], 1, d_pool, rpool_off, (bmh_region_res_t *)(dw + L.res1), (uint32_t *)(dw + L.cig1), (char *)(dw + L.md1), kWantMdSlot)))
		return e;
	if ((e = launch_wanted_results(ctx, A))) return e;
	// every download behind the last kernel: the slots of the records the status names, not of the capacity.  One block for the three:
	// as allocations of their own glibc returned these few MB after every call, and each call paid the page faults again
	D.n_w = hs[1].n_w, D.n_rec = hs[1].n_rec, D.n_fix = hs[0].n_rec;
	if (D.stay) return BMH_OK;
	const size_t bw = (size_t)D.n_w * sizeof(bmh_wanted_res_t), bc = (size_t)D.n_rec * BMH_RP_SMALL_CAP * 4, bm = (size_t)D.n_rec * kWantMdSlot;
	if (!(D.wres = (bmh_wanted_res_t *)malloc(bw + bc + bm + 4))) {
		ctx->last_error = std::string(who) + ": out of host memory";
		return BMH_E_NOMEM;
	}
	D.cig = (uint8_t *)D.wres + bw, D.md = D.cig + bc;
	if (bw && (e = st.d2h(D.wres, dw + L.wres, bw))) return e;
	return bc && ((e = st.d2h(D.cig, dw + L.cig1, bc)) || (e = st.d2h(D.md, dw + L.md1, bm))) ? e : BMH_OK;
}

// the planning kernels' time of the session just ended to *ms (timing mode)
static int wanted_kernel_ms(bmh_ctx *ctx, float *ms)
{
	float a = 0.f, b = 0.f;
	if (!ctx->timing || !ctx->ev_wanted[3]) return BMH_OK;
	BMH_HIP(ctx, hipEventElapsedTime(&a, ctx->ev_wanted[0], ctx->ev_wanted[1]));
	BMH_HIP(ctx, hipEventElapsedTime(&b, ctx->ev_wanted[2], ctx->ev_wanted[3]));
	*ms = a + b;
	return BMH_OK;
}

// a region whose alignment outgrew its slots: its read, and its record with the coordinates as cut (a region whose fix is redone still has its own)
struct RedoRegion {
	int read;
	bmh_alnreg_t reg;
};
struct RedoOut { // what the redo makes: one record per region in the order given, cigar_off / md_off addressing cig / md
	std::vector<bmh_wanted_res_t> hw;
	uint32_t *cig = nullptr;
	char *md = nullptr;
	~RedoOut() { free(cig), free(md); }
};

// the host's redo: through the host form again (it enters the device gate itself), one region per read of a small slice of its own
static int wanted_redo_host(bmh_ctx *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, const bmh_read_t *reads, std::vector<RedoRegion> &rr, RedoOut &R)
{
	const size_t m = rr.size();
	R.hw.resize(m);
	if (!m) return BMH_OK;
	std::vector<bmh_alnreg_v> rv(m);
	std::vector<bmh_read_t> rd(m);
	std::vector<int64_t> ro(m + 1);
	std::vector<int32_t> one(m, 1), zero(m, 0);
	for (size_t t = 0; t < m; ++t) rv[t].n = rv[t].m = 1, rv[t].a = &rr[t].reg, rd[t] = reads[rr[t].read], ro[t] = (int64_t)t;
	ro[m] = (int64_t)m;
	return bmh_wanted_host_(ctx, bns, pac, w, (int)m, rd.data(), rv.data(), ro.data(), one.data(), zero.data(), (int64_t)m, 1, R.hw.data(), &R.cig, &R.md, nullptr);
}

// The host's tail.  What came down is checked; the regions flagged BMH_WANTED_HOST, whose alignments outgrew their slots, go through
// wanted_redo_host, (read, k) from the want list, the region's record from `arena` -- every read's regions flat at roff: the stand-alone
// form's upload, the fused session's sorted download -- with the coordinates as cut; then CIGAR and MD are packed in want order.  wr: D.n_w records, D.wres
// itself if the caller likes; *cig_ / *md_: malloc'd, the caller frees them.  The want list is the caller's or checked by the caller.  who: the public entry point.
static int wanted_tail(bmh_ctx *ctx, const char *who, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads,
                       const int64_t *roff, const int32_t *n_want, const int32_t *want_k, const bmh_alnreg_t *arena, const WantedDown &D,
                       bmh_wanted_res_t *wr, uint32_t **cig_, char **md_, int64_t *redone)
{
	std::vector<int64_t> redo; // their places in want order
	std::vector<RedoRegion> rr;
	const int64_t n_w = D.n_w;
	size_t cu = 0, mu = 0;
	int64_t j = 0;
	for (int i = 0; i < n; ++i)
		for (int q = 0; q < n_want[i]; ++q, ++j) {
			const bmh_wanted_res_t &x = D.wres[j];
			const int k = want_k[roff[i] + q];
			const bool host = (x.flags & BMH_WANTED_HOST) != 0;
			if (host ? k < 0 || k >= roff[i + 1] - roff[i]
			         : (int64_t)x.cigar_off >= D.n_rec || x.n_cigar < 0 || x.n_cigar > BMH_RP_SMALL_CAP || x.md_len > (uint32_t)kWantMdSlot) { // cannot happen
				ctx->last_error = std::string(who) + ": the device's records are inconsistent";
				return BMH_E_ARG;
			}
			if (host) {
				redo.push_back(j), rr.push_back(RedoRegion{i, arena[roff[i] + k]});
				bmh_alnreg_t &a = rr.back().reg;
				a.rb = x.rb, a.re = x.re, a.qb = x.qb, a.qe = x.qe;
			} else cu += (size_t)x.n_cigar, mu += (size_t)x.md_len + 1;
		}
	const size_t m = redo.size();
	RedoOut H;
	const int rc = wanted_redo_host(ctx, bns, pac, w, reads, rr, H);
	if (rc) return rc;
	for (const bmh_wanted_res_t &x : H.hw) cu += (size_t)x.n_cigar, mu += (size_t)x.md_len + 1;
	uint32_t *cig = (uint32_t *)malloc(4 * (cu + 4));
	char *md = (char *)malloc(mu + 4);
	if (!cig || !md) {
		free(cig), free(md);
		ctx->last_error = std::string(who) + ": out of host memory";
		return BMH_E_NOMEM;
	}
	cu = mu = 0;
	size_t t = 0;
	for (j = 0; j < n_w; ++j) { // packed in want order
		bmh_wanted_res_t x = D.wres[j];
		const uint32_t *sc;
		const char *sm;
		if (t < m && redo[t] == j) {
			const uint32_t fl = x.flags;
			x = H.hw[t], sc = H.cig + x.cigar_off, sm = H.md + x.md_off;
			x.flags |= fl | BMH_WANTED_HOST;
			++t;
		} else sc = (const uint32_t *)D.cig + (size_t)x.cigar_off * BMH_RP_SMALL_CAP, sm = (const char *)D.md + (size_t)x.md_off * kWantMdSlot;
		memcpy(cig + cu, sc, 4 * (size_t)x.n_cigar), memcpy(md + mu, sm, x.md_len), md[mu + x.md_len] = 0;
		x.cigar_off = (uint32_t)cu, x.md_off = (uint32_t)mu;
		cu += (size_t)x.n_cigar, mu += (size_t)x.md_len + 1;
		wr[j] = x;
	}
	*cig_ = cig, *md_ = md, *redone = (int64_t)m;
	return BMH_OK;
}

// the stand-alone form up to its own records and pools (*cig_ / *md_: malloc'd, the caller frees them), for the public call and bmh_sam_batch
static int wanted_device_run(bmh_ctx *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads, const bmh_alnreg_v *regs,
                             const int64_t *roff, const int32_t *n_want, const int32_t *want_k, int64_t n_w, bmh_wanted_res_t *wr, uint32_t **cig_, char **md_)
{
	*cig_ = nullptr, *md_ = nullptr;
	reset_wanted_stats(ctx);
	if (!ctx->have_params) return BMH_E_ARG;
	int rc = need_resident(ctx, "bmh_wanted_cigar_device", bns, pac);
	if (rc || n_w == 0) return rc;
	if (n_w > (1 << 28) || n > (1 << 28)) return BMH_E_ARG;
	const size_t nr = (size_t)n, total = (size_t)roff[n], wc = (size_t)n_w;
	const size_t reads_bytes = reads_total(n, reads);
	size_t opool_cap = 0;
	for (int i = 0; i < n; ++i)
		for (int q = 0; q < n_want[i]; ++q) {
			const int k = want_k[roff[i] + q];
			if (k >= 0 && (size_t)k < regs[i].n) opool_cap += oriented_cap(&regs[i].a[k]); // (another the kernel refuses)
		}
	// the device block: [offsets | read offsets | parameters | n_want | want_k | regions] up, then the session's arrays
	Block b;
	b.take((nr + 1) * 8);
	const size_t o_soff = b.take((nr + 1) * 8), o_hdr = b.take(sizeof(WantedHdr)), o_nw = b.take(nr * 4), o_wk = b.take(total * 4);
	const size_t o_reg = b.take(total * sizeof(bmh_alnreg_t)), b_up = b.at;
	const WantedBlock L = wanted_block(b, nr, wc);
	HostBuf up(b_up), rpool(reads_bytes + 16);
	if (!up.p || !rpool.p) {
		ctx->last_error = "bmh_wanted_cigar_device: out of host memory";
		return BMH_E_NOMEM;
	}
	memcpy(up.p, roff, (nr + 1) * 8);
	wanted_fill(ctx, w, n, reads, (uint64_t *)(up.p + o_soff), (WantedHdr *)(up.p + o_hdr), rpool.p);
	memcpy(up.p + o_nw, n_want, nr * 4);
	slice_copy_flat(n, regs, roff, up.p + o_reg, n_want, want_k, up.p + o_wk);
	const WantedSizes Z{total, reads_bytes, wc, opool_cap, n, bns->l_pac};
	WantedDown D;
	{ // the device section, inside the caller's gate (the redo enters it again through the host form)
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Stager st(ctx);
	rc = [&]() -> int {
		int e;
		size_t rpool_off;
		if ((e = wanted_reserve(ctx, wc, opool_cap, reads_bytes, L.end, &rpool_off)) || (e = st.stage(b_up + reads_bytes + 256, L.end - L.wres + 256))) return e;
		uint8_t *d = (uint8_t *)ctx->d_wanted.p;
		if ((e = st.h2d(d, up.p, b_up)) || (e = st.h2d((uint8_t *)ctx->d_pool.p + rpool_off, rpool.p, reads_bytes + 16))) return e;
		const WantedArgs A = wanted_inputs(d, (const int32_t *)(d + o_nw), (const int32_t *)(d + o_wk), (const bmh_alnreg_t *)(d + o_reg), d + o_soff, d + o_hdr, Z);
		return wanted_session(ctx, "bmh_wanted_cigar_device", st, A, d, L, rpool_off, n_w, n_w, D);
	}();
	rc = st.end(rc);
	if (rc == BMH_E_CIGAR_CAP) rc = BMH_OK; // a task that outgrew its slots is reported per region (BMH_REGION_CIGAR_CUT)
	if (rc || (rc = wanted_kernel_ms(ctx, &ctx->wanted_ms))) return rc;
	}
	int64_t redone = 0;
	rc = wanted_tail(ctx, "bmh_wanted_cigar_device", bns, pac, w, n, reads, roff, n_want, want_k, (const bmh_alnreg_t *)(up.p + o_reg), D, wr, cig_, md_, &redone);
	if (rc) return rc;
	ctx->wanted_n = n_w, ctx->wanted_fixed = D.n_fix, ctx->wanted_redone = redone;
	return BMH_OK;
}

int bmh_wanted_cigar_device(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads, const bmh_alnreg_v *regs,
                            const int64_t *roff, const int32_t *n_want, const int32_t *want_k, bmh_wanted_res_t *results, uint32_t *cigar_pool,
                            size_t cigar_words, char *md_pool, size_t md_bytes)
{
	int64_t n_w = 0;
	int rc = bmh_wanted_check_args_(ctx, bns, pac, n, reads, regs, roff, n_want, want_k, &n_w);
	if (rc) return rc;
	if (n_w > 0 && (!results || !cigar_pool || !md_pool)) return BMH_E_ARG;
	std::vector<bmh_wanted_res_t> wr((size_t)n_w);
	uint32_t *cig = nullptr;
	char *md = nullptr;
	rc = wanted_device_run(ctx, bns, pac, w, n, reads, regs, roff, n_want, want_k, n_w, wr.data(), &cig, &md);
	if (!rc && n_w > 0) rc = bmh_wanted_deliver_(n_w, wr.data(), cig, md, results, cigar_pool, cigar_words, md_pool, md_bytes);
	free(cig), free(md);
	return rc;
}

int bmh_ctx_set_wanted_device(bmh_ctx_t *ctx, int on)
{
	if (!ctx) return BMH_E_ARG;
	ctx->wanted_device = on != 0;
	return BMH_OK;
}

int bmh_last_wanted_stats(const bmh_ctx_t *ctx, int64_t *wanted, int64_t *fixed, int64_t *redone, float *kernel_ms)
{
	if (!ctx) return BMH_E_ARG;
	if (wanted) *wanted = ctx->wanted_n;
	if (fixed) *fixed = ctx->wanted_fixed;
	if (redone) *redone = ctx->wanted_redone;
	if (kernel_ms) *kernel_ms = ctx->wanted_ms;
	return BMH_OK;
}

// bmh_sam_batch's pass B (host/sam_post.c; not part of the interface)
__attribute__((visibility("hidden"))) int bmh_wanted_routed_(bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads,
                                                             const bmh_alnreg_v *regs, const int64_t *roff, const int32_t *n_want, const int32_t *want_k,
                                                             int64_t n_w, bmh_wanted_res_t *wr, uint32_t **cig, char **md)
{
	if (ctx && ctx->wanted_device) {
		int64_t chk = 0;
		int rc = bmh_wanted_check_args_(ctx, bns, pac, n, reads, regs, roff, n_want, want_k, &chk);
		if (rc || chk != n_w) return rc ? rc : BMH_E_ARG;
		return wanted_device_run(ctx, bns, pac, w, n, reads, regs, roff, n_want, want_k, n_w, wr, cig, md);
	}
	return bmh_wanted_host_(ctx, bns, pac, w, n, reads, regs, roff, n_want, want_k, n_w, 0, wr, cig, md, nullptr);
}

// ------------------------------------------------------------------ pass A and pass B of phase 2 as one device session

// what bmh_wanted_check_args_ refuses without reading the want list (the vectors and offsets are bmh_pp_check_args's already)
static int phase2_check_reads(const bmh_refidx_t *bns, const uint8_t *pac, int n, const bmh_read_t *reads)
{
	if (!bns || !pac || bns->l_pac <= 0 || bns->n_seqs <= 0 || !bns->anns || (n > 0 && !reads)) return BMH_E_ARG;
	for (int i = 0; i < n; ++i)
		if (reads[i].l_seq < 0 || (reads[i].l_seq > 0 && !reads[i].seq)) return BMH_E_ARG;
	return BMH_OK;
}

// what a fused session holds on the host until everything has succeeded: nothing of the caller's is written before decide_commit
struct Phase2Run {
	DecideBlock L;
	std::vector<uint8_t> down;        // pass A's block as downloaded: [regions | reg_mapq | want_k | n_want | pd], the regions sorted
	int64_t n_w = 0;
	bmh_wanted_res_t *wr = nullptr;   // want order; cigar_off / md_off address cig / md
	uint32_t *cig = nullptr;
	char *md = nullptr;
	~Phase2Run() { free(wr), free(cig), free(md); }
};

// What passes A and B of a fused session are sized from, pass A's tables, and the two blocks: pass A's with pass B's inputs in it, and
// pass B's arrays in a block of their own.  Z.wc = Z.total: the capacity of everything per wanted region, which bounds their number.
struct Phase2Plan {
	DecideTables T;
	DecideBlock LA;
	WantedBlock LB;
	WantedSizes Z;
	bool pe;
	int64_t id0;
};

// ... from the caller's vectors or, res, from what table_plan_kernel found.  The oriented pool is sized from the clamped lengths of every
// region: a sum the sort does not change, and a cut only shortens a region.  *why not NULL: the tables' refusal, before any upload.
static int phase2_plan(bmh_ctx *ctx, const bmh_sam_opt_t *o, const bmh_pestat_t *pes, int64_t l_pac, int64_t id0, int n, const bmh_read_t *reads, const bmh_alnreg_v *regs,
                       const ResidentRegs *res, size_t total, Phase2Plan &P, const char **why)
{
	DecideTables &T = P.T;
	size_t opool_cap = 0;
	int rc;
	*why = nullptr;
	if (res) {
		const bmh_ho_plan_t plan{res->kmax, res->opool_cap, res->total, res->neg ? 1 : 0, 0};
		rc = decide_tables_from_plan(o, pes, plan, res->pair_kmax, &T.kmax, &T.n_term, T.term_off, why); // (pair_kmax: 0 from a single-end call)
		opool_cap = (size_t)res->opool_cap;
	} else
		rc = decide_table_sizes(o, pes, n, regs, &T.kmax, &T.n_term, T.term_off, why, &opool_cap);
	if (rc || (rc = decide_host_log(ctx, T.kmax, &T.want_log))) return rc;
	P.pe = (o->flag & BMH_MEM_F_PE) != 0, P.id0 = id0;
	P.Z = WantedSizes{total, reads_total(n, reads), total, opool_cap, n, l_pac};
	P.LA = decide_block((size_t)n, total, (size_t)T.n_term, P.pe, true);
	Block b;
	P.LB = wanted_block(b, (size_t)n, P.Z.wc);
	return BMH_OK;
}

// Passes A and B of a fused session on the stream, up to and including wanted_session: the workspaces, the log table, upload(d, rpool)
// -- what the session sends or copies into pass A's block at d and pass B's reads pool at rpool, staged as up_bytes and down_bytes --
// then decide_kernel and, where there are regions, pass B on what it left in place: no wait, no copy in between.  gather: the reads
// pool is not uploaded but made on the device from the per-read pool that these arguments of pass C name.
static int phase2_enqueue_ab(bmh_ctx *ctx, const char *who, Stager &st, const Phase2Plan &P, size_t up_bytes, size_t down_bytes,
                             const std::function<int(uint8_t *, uint8_t *)> &upload, const SamtextArgs *gather, WantedDown &D)
{
	const WantedSizes &Z = P.Z;
	int e;
	size_t rpool_off;
	if ((e = ensure(ctx, ctx->d_decide, P.LA.end)) || (e = wanted_reserve(ctx, Z.wc, Z.opool_cap, Z.reads_bytes, P.LB.end, &rpool_off))) return e;
	if ((e = decide_stage_log(ctx, st, P.T.want_log, up_bytes, down_bytes))) return e;
	uint8_t *d = (uint8_t *)ctx->d_decide.p, *rpool = (uint8_t *)ctx->d_pool.p + rpool_off;
	if ((e = upload(d, rpool))) return e;
	BMH_HIP(ctx, hipMemsetAsync(d + P.LA.nw, 0, (size_t)Z.n * 4, ctx->stream)); // a unit decide_kernel refuses wants nothing
	const DecideArgs DA = decide_args(ctx, d, P.LA, P.T, Z.total, Z.l_pac, P.id0, Z.n, P.pe);
	if ((e = launch_decide(ctx, DA)) || !Z.wc) return e;
	if (gather) { // the bases of the per-read pool at seq_off[], 16 zero bytes behind them
		BMH_HIP(ctx, hipMemsetAsync(rpool + Z.reads_bytes, 0, 16, ctx->stream));
		if ((e = launch_reads_gather(ctx, *gather, (const unsigned long long *)(d + P.LA.soff), rpool, Z.reads_bytes))) return e;
	}
	const WantedArgs A = wanted_inputs(DA.roff, DA.n_want, DA.want_k, DA.reg, d + P.LA.soff, d + P.LA.whdr, Z);
	return wanted_session(ctx, who, st, A, (uint8_t *)ctx->d_wanted.p, P.LB, rpool_off, 0, (int64_t)Z.wc, D);
}

// The session up to its own records and pools, for the public call and bmh_sam_batch.  n > 0 and the arguments checked.  *tables: the
// BMH_E_RANGE is bmh_decide_device's refusal before any upload, not a kernel's.
static int phase2_device_run(bmh_ctx *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes, int64_t id0, int n,
                             const bmh_read_t *reads, const bmh_alnreg_v *regs, const int64_t *roff, Phase2Run &R, bool *tables)
{
	*tables = false;
	reset_phase2_stats(ctx), reset_decide_stats(ctx), reset_wanted_stats(ctx);
	if (!ctx->have_params) return BMH_E_ARG;
	int rc = need_resident(ctx, "bmh_phase2_device", bns, pac);
	if (rc) return rc;
	if (n > (1 << 28) || roff[n] > (1 << 28)) return BMH_E_ARG;
	Phase2Plan P;
	const char *why;
	if ((rc = phase2_plan(ctx, o, pes, bns->l_pac, id0, n, reads, regs, nullptr, (size_t)roff[n], P, &why))) {
		if (why) {
			ctx->last_error = why;
			ctx->decide_fallbacks = 1, ctx->p2.fallbacks = 1, *tables = true;
		}
		return rc;
	}
	const DecideBlock &LA = R.L = P.LA;
	const size_t reads_bytes = P.Z.reads_bytes, wc = P.Z.wc;
	const bool pe = P.pe;
	HostBuf up(LA.up()), rpool(reads_bytes + 16);
	if (!up.p || !rpool.p) {
		ctx->last_error = "bmh_phase2_device: out of host memory";
		return BMH_E_NOMEM;
	}
	R.down.resize(LA.down());
	decide_fill(up.p, LA, o, pes, P.T, n, regs, roff);
	wanted_fill(ctx, o->w, n, reads, (uint64_t *)(up.p + LA.soff), (WantedHdr *)(up.p + LA.whdr), rpool.p);
	WantedDown D;
	{ // the device section, inside the caller's gate (the redo enters it again through the host form)
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Stager st(ctx);
	st.cnt = {&ctx->p2.h2d_bytes, &ctx->p2.d2h_bytes, &ctx->p2.waits};
	auto upload = [&](uint8_t *d, uint8_t *d_rpool) {
		const int e = st.h2d(d, up.p, LA.up());
		return e ? e : st.h2d(d_rpool, rpool.p, reads_bytes + 16);
	};
	rc = phase2_enqueue_ab(ctx, "bmh_phase2_device", st, P, LA.up() + reads_bytes + 256, LA.down() + (P.LB.end - P.LB.wres) + 256, upload, nullptr, D);
	if (!rc) rc = st.d2h(R.down.data(), (uint8_t *)ctx->d_decide.p + LA.reg, LA.down());
	rc = st.end(rc);
	if (rc == BMH_E_CIGAR_CAP) rc = BMH_OK; // a task that outgrew its slots is reported per region (BMH_REGION_CIGAR_CUT)
	if (rc) return rc;
	ctx->logk_n = P.T.want_log;
	if (ctx->timing) {
		BMH_HIP(ctx, hipEventElapsedTime(&ctx->decide_ms, ctx->ev_decide[0], ctx->ev_decide[1]));
		if (wc && (rc = wanted_kernel_ms(ctx, &ctx->wanted_ms))) return rc;
	}
	}
	// the want list as pass A left it, checked against the vectors and the session's count; then pass B's tail over the downloaded,
	// sorted block (the caller's vectors are still unsorted)
	const uint8_t *down = R.down.data();
	const int64_t n_w = D.n_w;
	if (decide_want_count(down, LA, n, regs) != n_w) { // cannot happen
		ctx->last_error = "bmh_phase2_device: the device's counts are inconsistent";
		return BMH_E_ARG;
	}
	int64_t redone = 0;
	rc = wanted_tail(ctx, "bmh_phase2_device", bns, pac, o->w, n, reads, roff, (const int32_t *)(down + (LA.nw - LA.reg)), (const int32_t *)(down + (LA.wk - LA.reg)),
	                 (const bmh_alnreg_t *)down, D, D.wres, &R.cig, &R.md, &redone);
	if (rc) return rc;
	// the records were packed where they lay, at the start of the session's block: the slots behind them are given back, the rest handed on
	if (void *p = realloc(D.wres, (size_t)n_w * sizeof(bmh_wanted_res_t) + 4)) D.wres = (bmh_wanted_res_t *)p;
	R.wr = D.wres, D.wres = nullptr, R.n_w = n_w;
	ctx->decide_units = pe ? n >> 1 : n;
	ctx->wanted_n = n_w, ctx->wanted_fixed = D.n_fix, ctx->wanted_redone = redone;
	ctx->p2.units = ctx->decide_units, ctx->p2.wanted = n_w, ctx->p2.fixed = D.n_fix, ctx->p2.redone = redone;
	ctx->p2.sessions = 1, ctx->p2.decide_ms = ctx->decide_ms, ctx->p2.wanted_ms = ctx->wanted_ms;
	return BMH_OK;
}

int bmh_phase2_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes, int64_t id0, int n,
                      const bmh_read_t *reads, bmh_alnreg_v *regs, const int64_t *roff, bmh_pairdec_t *pd, int32_t *reg_mapq, int32_t *n_want,
                      int32_t *want_k, bmh_wanted_res_t *results, int64_t results_cap, int64_t *n_wanted, uint32_t *cigar_pool, size_t cigar_words,
                      char *md_pool, size_t md_bytes)
{
	if (!ctx || !n_wanted) return BMH_E_ARG;
	int rc = bmh_pp_check_args(o, pes, n, regs, roff, pd, reg_mapq, n_want, want_k);
	if (rc || (rc = phase2_check_reads(bns, pac, n, reads))) return rc;
	if (n == 0) {
		reset_phase2_stats(ctx);
		*n_wanted = 0;
		return BMH_OK;
	}
	if (results_cap < 0 || (roff[n] > 0 && (!results || !cigar_pool || !md_pool))) return BMH_E_ARG;
	Phase2Run R;
	bool tables;
	if ((rc = phase2_device_run(ctx, o, bns, pac, pes, id0, n, reads, regs, roff, R, &tables))) return rc;
	if (R.n_w > results_cap) return BMH_E_CIGAR_CAP;
	if (R.n_w && (rc = bmh_wanted_deliver_(R.n_w, R.wr, R.cig, R.md, results, cigar_pool, cigar_words, md_pool, md_bytes))) return rc;
	decide_commit(R.down.data(), R.L, (o->flag & BMH_MEM_F_PE) != 0, n, regs, roff, pd, reg_mapq, n_want, want_k);
	*n_wanted = R.n_w;
	return BMH_OK;
}

int bmh_ctx_set_phase2_device(bmh_ctx_t *ctx, int on)
{
	if (!ctx) return BMH_E_ARG;
	ctx->phase2_device = on != 0;
	return BMH_OK;
}

int bmh_last_phase2_stats(const bmh_ctx_t *ctx, bmh_phase2_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->p2;
	return BMH_OK;
}

// bmh_sam_batch's pass A and pass B as one session (host/sam_post.c; not part of the interface).  *done = 1: the outputs are the fused
// call's, *wr / *cig / *md malloc'd.  *done = 0 with BMH_OK: the switch is off, or the call refused the slice's tables before its
// upload (the statistics then say one fall-back, two sessions), and the caller goes through the two routed passes.
__attribute__((visibility("hidden"))) int bmh_phase2_routed_(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac,
                                                             const bmh_pestat_t *pes, int64_t id0, int n, const bmh_read_t *reads, bmh_alnreg_v *regs,
                                                             const int64_t *roff, bmh_pairdec_t *pd, int32_t *reg_mapq, int32_t *n_want, int32_t *want_k,
                                                             int64_t *n_w, bmh_wanted_res_t **wr, uint32_t **cig, char **md, int *done)
{
	*done = 0;
	if (!ctx || !ctx->phase2_device) return BMH_OK;
	int rc = bmh_pp_check_args(o, pes, n, regs, roff, pd, reg_mapq, n_want, want_k);
	if (rc || (rc = phase2_check_reads(bns, pac, n, reads))) return rc;
	Phase2Run R;
	bool tables;
	rc = phase2_device_run(ctx, o, bns, pac, pes, id0, n, reads, regs, roff, R, &tables);
	if (rc == BMH_E_RANGE && tables) {
		ctx->p2.sessions = 2;
		return BMH_OK;
	}
	if (rc) return rc;
	decide_commit(R.down.data(), R.L, (o->flag & BMH_MEM_F_PE) != 0, n, regs, roff, pd, reg_mapq, n_want, want_k);
	*wr = R.wr, *cig = R.cig, *md = R.md, R.wr = nullptr, R.cig = nullptr, R.md = nullptr;
	*n_w = R.n_w, *done = 1;
	return BMH_OK;
}

// ------------------------------------------------------------------ pass C of phase 2 on the device (samtext.hip)

// the argument check of the two forms (host/sam_post.c; not part of the interface)
int bmh_samtext_check_(const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs, const bmh_alnreg_v *regs,
                       const int64_t *roff, const bmh_pairdec_t *pd, const int32_t *reg_mapq, const int32_t *n_want, const int32_t *want_k,
                       const bmh_wanted_res_t *wr, const uint32_t *cig, const char *md, char **text, int64_t *text_off, int64_t *first, int64_t *lines,
                       size_t *cig_words, size_t *md_bytes);

// the names of bns as the device holds them: n_seqs + 1 offsets, then the bytes
static std::vector<char> refnames_block(const bmh_refidx_t *bns)
{
	const size_t ns = (size_t)bns->n_seqs;
	size_t bytes = 0;
	for (size_t i = 0; i < ns; ++i) bytes += strlen(bns->anns[i].name);
	std::vector<char> t((ns + 1) * 8 + bytes);
	uint64_t at = 0;
	for (size_t i = 0; i < ns; ++i) {
		const size_t l = strlen(bns->anns[i].name);
		memcpy(t.data() + i * 8, &at, 8);
		memcpy(t.data() + (ns + 1) * 8 + at, bns->anns[i].name, l);
		at += l;
	}
	memcpy(t.data() + ns * 8, &at, 8);
	return t;
}

int bmh_ctx_set_refnames(bmh_ctx_t *ctx, const bmh_refidx_t *bns)
{
	if (!ctx) return BMH_E_ARG;
	if (!bns) {
		ctx->refnames_n = 0, ctx->h_refnames.clear();
		return BMH_OK;
	}
	if (bns->n_seqs <= 0 || !bns->anns) return BMH_E_ARG;
	for (int i = 0; i < bns->n_seqs; ++i)
		if (!bns->anns[i].name) return BMH_E_ARG;
	std::vector<char> t = refnames_block(bns);
	if (ctx->refnames_n == bns->n_seqs && ctx->h_refnames == t) return BMH_OK; // already resident: the same names
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream)); // (nothing in flight reads the table while it is replaced)
	ctx->refnames_n = 0, ctx->h_refnames.clear();
	int rc;
	if ((rc = ensure(ctx, ctx->d_refnames, t.size()))) return rc;
	BMH_HIP(ctx, hipMemcpy(ctx->d_refnames.p, t.data(), t.size(), hipMemcpyHostToDevice));
	ctx->refnames_n = bns->n_seqs, ctx->h_refnames = std::move(t);
	return BMH_OK;
}

// the per-read pool of pass C's two device forms (SamtextRead, samtext.h): planned, then packed into zeroed memory
struct SamtextPool {
	std::vector<uint64_t> poff; // n + 1: read i's record; poff[n] = the pool's bytes
	std::vector<int32_t> l_name, l_com;
	bool bases = true; // false: the records hold no bases (a session whose bases are on the device already: SamtextArgs::bases)
	int plan(int n, const bmh_seq_t *seqs, bool with_bases = true)
	{
		bases = with_bases;
		const size_t nr = (size_t)n;
		poff.resize(nr + 1), l_name.resize(nr), l_com.resize(nr);
		size_t bytes = 0;
		for (size_t i = 0; i < nr; ++i) {
			const size_t ln = strlen(seqs[i].name), lc = seqs[i].comment ? strlen(seqs[i].comment) : 0;
			if (ln > 0x7fffffffu || lc > 0x7fffffffu) return BMH_E_ARG;
			l_name[i] = (int32_t)ln, l_com[i] = seqs[i].comment ? (int32_t)lc : -1;
			poff[i] = bytes;
			bytes += samtext_read_bytes(ln, (size_t)seqs[i].l_seq, seqs[i].qual != nullptr, l_com[i], bases);
		}
		poff[nr] = bytes;
		return BMH_OK;
	}
	void fill(int n, const bmh_seq_t *seqs, uint8_t *pool) const
	{
		for (size_t i = 0; i < (size_t)n; ++i) {
			const bmh_seq_t &s = seqs[i];
			uint8_t *b = pool + poff[i];
			const SamtextRead h{l_name[i], s.l_seq, s.qual != nullptr, l_com[i]};
			memcpy(b, &h, sizeof(h)), b += sizeof(h);
			memcpy(b, s.name, (size_t)h.l_name), b += h.l_name;
			if (bases && s.l_seq) memcpy(b, s.seq, (size_t)s.l_seq), b += s.l_seq;
			if (s.qual && s.l_seq) memcpy(b, s.qual, (size_t)s.l_seq), b += s.l_seq;
			if (h.l_comment > 0) memcpy(b, s.comment, (size_t)h.l_comment);
		}
	}
};

// the sequence names of bns as the context holds them
static int need_refnames(bmh_ctx *ctx, const char *who, const bmh_refidx_t *bns)
{
	if (ctx->refnames_n == 0 || ctx->refnames_n != bns->n_seqs || ctx->h_refnames != refnames_block(bns)) {
		ctx->last_error = std::string(who) + " needs the resident sequence names (bmh_ctx_set_refnames)";
		return BMH_E_ARG;
	}
	return BMH_OK;
}

// Pass C's device block, in two forms.  Stand-alone (bmh_sam_text_device): [roff | first | poff | SamtextHdr | rg_id | n_want | want_k |
// reg_mapq | pd | regions | records | CIGAR | MD | the per-read pool] up, then what the kernels make: the records, plans, sizes,
// offsets and the status.  Fused (the session through to the text): the want list, mapQ, verdicts, regions, records, CIGAR and MD lie
// in pass A's and pass B's blocks, so [SamtextHdr | rg_id | poff | the per-read pool] goes up, a SamtextFused sits behind the status
// and the list of the host's regions behind that.
struct SamtextBlock {
	size_t roff, first, poff, hdr, rg, nw, wk, mq, pd, reg, wr, cig, md, pool, up, alns, plan, size, toff, stat, list, end;
	size_t pool_bytes, stat_bytes; // the per-read pool; what the look brings down: the status, and the SamtextFused where there is one
	bool fused;
};

static SamtextBlock samtext_block(bool fused, size_t n, size_t total, size_t wc, size_t l_rg, size_t pool_bytes, bool pe, size_t cig_words, size_t md_bytes)
{
	Block b;
	SamtextBlock L{};
	if (!fused) L.roff = b.take((n + 1) * 8), L.first = b.take((n + 1) * 8), L.poff = b.take((n + 1) * 8);
	L.hdr = b.take(sizeof(SamtextHdr)), L.rg = b.take(l_rg);
	if (fused) L.poff = b.take((n + 1) * 8);
	else {
		L.nw = b.take(n * 4), L.wk = b.take(total * 4), L.mq = b.take(total * 4), L.pd = b.take(pe ? (n >> 1) * sizeof(bmh_pairdec_t) : 0);
		L.reg = b.take(total * sizeof(bmh_alnreg_t)), L.wr = b.take(wc * sizeof(bmh_wanted_res_t)), L.cig = b.take(cig_words * 4), L.md = b.take(md_bytes);
	}
	L.pool = b.take(pool_bytes), L.up = b.at, L.pool_bytes = pool_bytes, L.fused = fused;
	L.alns = b.take(wc * sizeof(bmh_st_aln_t)), L.plan = b.take(n * sizeof(bmh_st_plan_t)), L.size = b.take(n * 8), L.toff = b.take((n + 1) * 8);
	L.stat_bytes = sizeof(SamtextStatus) + (fused ? sizeof(SamtextFused) : 0);
	L.stat = b.take(L.stat_bytes), L.list = b.take(fused ? wc * sizeof(Phase2TextHost) : 0), L.end = b.at;
	return L;
}

// Pass C's arguments for the size kernels (text and text_cap are the emit's: samtext_emit_down) over its block at dt.  Fused: the want
// list, mapQ, verdicts and sorted regions where decide_kernel left them in pass A's block at d; first[] and the records where pass B's
// kernels left them in its block at dw, CIGAR and MD in the main round's slots there (and the overflow area behind the block)
static SamtextArgs samtext_args(bmh_ctx *ctx, uint8_t *dt, const SamtextBlock &L, size_t total, size_t n_w, size_t cig_words, size_t md_bytes, int n, bool pe,
                                int64_t l_pac, const uint8_t *d = nullptr, const DecideBlock *LA = nullptr, const uint8_t *dw = nullptr, const WantedBlock *LB = nullptr)
{
	const bool f = L.fused;
	SamtextArgs A{};
	A.roff = (const int64_t *)(f ? d : dt + L.roff), A.first = (const int64_t *)(f ? dw + LB->first : dt + L.first), A.poff = (const unsigned long long *)(dt + L.poff);
	A.hdr = (const SamtextHdr *)(dt + L.hdr), A.rg = (const char *)(dt + L.rg);
	A.n_want = (const int32_t *)(f ? d + LA->nw : dt + L.nw), A.want_k = (const int32_t *)(f ? d + LA->wk : dt + L.wk);
	A.reg_mapq = (const int32_t *)(f ? d + LA->mq : dt + L.mq), A.pd = (const bmh_pairdec_t *)(f ? d + LA->pd : dt + L.pd);
	A.reg = (const bmh_alnreg_t *)(f ? d + LA->reg : dt + L.reg), A.wr = (const bmh_wanted_res_t *)(f ? dw + LB->wres : dt + L.wr);
	A.cig = (const uint32_t *)(f ? dw + LB->cig1 : dt + L.cig), A.md = (const char *)(f ? dw + LB->md1 : dt + L.md), A.rpool = dt + L.pool;
	A.total = total, A.n_w = n_w, A.cig_words = cig_words, A.md_bytes = md_bytes, A.rpool_bytes = L.pool_bytes;
	A.ref = (const bmh_refspan_t *)ctx->d_refidx.p, A.name_off = (const uint64_t *)ctx->d_refnames.p;
	A.names = (const char *)ctx->d_refnames.p + ((size_t)ctx->refnames_n + 1) * 8;
	A.n_seqs = ctx->refidx_n, A.n = n, A.pe = pe, A.l_pac = l_pac;
	A.alns = (bmh_st_aln_t *)(dt + L.alns), A.plan = (bmh_st_plan_t *)(dt + L.plan), A.size = (unsigned long long *)(dt + L.size);
	A.toff = (unsigned long long *)(dt + L.toff), A.status = (SamtextStatus *)(dt + L.stat), A.text = nullptr, A.text_cap = 0, A.err = ctx->d_err;
	A.fused = f ? (SamtextFused *)(dt + L.stat + sizeof(SamtextStatus)) : nullptr;
	return A;
}

// the sections of pass C's upload that both forms have, into zeroed memory: SamtextHdr, rg_id, poff and the per-read pool
static void samtext_fill_up(uint8_t *up, const SamtextBlock &L, const bmh_sam_opt_t *o, const bmh_pestat_t *pes, const char *rg_id, size_t l_rg,
                            const SamtextPool &P, int n, const bmh_seq_t *seqs)
{
	SamtextHdr *hdr = (SamtextHdr *)(up + L.hdr);
	hdr->opt_flag = o->flag, hdr->pe = (o->flag & BMH_MEM_F_PE) != 0, hdr->l_rg = (int32_t)l_rg;
	if (hdr->pe) memcpy(hdr->pes, pes, sizeof(hdr->pes));
	if (l_rg) memcpy(up + L.rg, rg_id, l_rg);
	memcpy(up + L.poff, P.poff.data(), ((size_t)n + 1) * 8);
	P.fill(n, seqs, up + L.pool);
}

// what pass C holds on the host until everything has succeeded
struct SamtextOut {
	int64_t *toff = nullptr; // n + 1, malloc'd by the caller
	char *out = nullptr;     // the text, malloc'd by samtext_emit_down
	long long total = 0, lines = 0;
	~SamtextOut() { free(toff), free(out); }
};

// pass C, first half: size and scan, then the one look behind them: stat_bytes of the block's status to the session's pinned h_stat
static int samtext_size_look(bmh_ctx *ctx, const char *who, Stager &st, const SamtextArgs &A, void *h_stat, size_t stat_bytes)
{
	int e;
	if ((e = launch_samtext_size(ctx, A))) return e;
	BMH_HIP(ctx, hipMemcpyAsync(h_stat, A.status, stat_bytes, hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	st.waited(stat_bytes);
	if (const int err = ((const SamtextStatus *)h_stat)->err) {
		ctx->last_error = std::string(who) + ": a record lies outside its read, its vector, the pools or the reference";
		return err;
	}
	return BMH_OK;
}

// ... second half: the buffer sized from the status at h_stat, the emit kernel, text_off and the text down, stage_up bytes staged up
// beside them.  O.toff is the caller's already; O.out, O.total and O.lines are set here.
static int samtext_emit_down(bmh_ctx *ctx, const char *who, Stager &st, SamtextArgs A, const void *h_stat, size_t stage_up, SamtextOut &O)
{
	const SamtextStatus *hs = (const SamtextStatus *)h_stat;
	const size_t nr = (size_t)A.n;
	int e;
	O.total = hs->total, O.lines = A.fused ? ((const SamtextFused *)(hs + 1))->lines : 0;
	if (O.total < 0 || O.total > ((long long)1 << 40) || O.lines < 0) { // cannot happen
		ctx->last_error = std::string(who) + ": the device's sizes are inconsistent";
		return BMH_E_ARG;
	}
	const size_t bytes = (size_t)O.total;
	if (!(O.out = (char *)malloc(bytes + 1))) return BMH_E_NOMEM;
	if ((e = ensure(ctx, ctx->d_sam_out, bytes + 64)) || (e = st.stage(stage_up, (nr + 1) * 8 + bytes + 256))) return e;
	A.text = (char *)ctx->d_sam_out.p, A.text_cap = (unsigned long long)O.total;
	if ((e = launch_samtext_emit(ctx, A)) || (e = st.d2h(O.toff, A.toff, (nr + 1) * 8))) return e;
	return bytes ? st.d2h(O.out, ctx->d_sam_out.p, bytes) : BMH_OK;
}

// Behind st.end(): the offsets checked, then -- all or nothing, the caller's outputs only now -- the hand-over
static int samtext_commit(bmh_ctx *ctx, const char *who, int n, SamtextOut &O, char **text, int64_t *text_off)
{
	if (O.toff[0] != 0 || O.toff[n] != O.total) { // cannot happen
		ctx->last_error = std::string(who) + ": the device's offsets are inconsistent";
		return BMH_E_ARG;
	}
	memcpy(text_off, O.toff, ((size_t)n + 1) * 8);
	*text = O.out, O.out = nullptr;
	return BMH_OK;
}

// the size and emit kernels' times of the session just ended (timing mode)
static int samtext_kernel_ms(bmh_ctx *ctx, float *size_ms, float *emit_ms)
{
	if (!ctx->timing) return BMH_OK;
	BMH_HIP(ctx, hipEventElapsedTime(size_ms, ctx->ev_samtext[0], ctx->ev_samtext[1]));
	BMH_HIP(ctx, hipEventElapsedTime(emit_ms, ctx->ev_samtext[2], ctx->ev_samtext[3]));
	return BMH_OK;
}

int bmh_sam_text_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs,
                        const bmh_alnreg_v *regs, const int64_t *roff, const bmh_pairdec_t *pd, const int32_t *reg_mapq, const int32_t *n_want,
                        const int32_t *want_k, const bmh_wanted_res_t *results, const uint32_t *cigar_pool, const char *md_pool, const char *rg_id,
                        char **text, int64_t *text_off)
{
	static const char *const who = "bmh_sam_text_device";
	if (!ctx) return BMH_E_ARG;
	reset_samtext_stats(ctx);
	std::vector<int64_t> first((size_t)(n > 0 ? n : 0) + 1);
	int64_t lines = 0;
	size_t cig_words = 0, md_bytes = 0;
	int rc = bmh_samtext_check_(o, bns, pes, n, seqs, regs, roff, pd, reg_mapq, n_want, want_k, results, cigar_pool, md_pool, text, text_off, first.data(),
	                            &lines, &cig_words, &md_bytes);
	if (rc || (rc = need_resident(ctx, who, bns, nullptr)) || (rc = need_refnames(ctx, who, bns))) return rc;
	if (n == 0) return empty_text(text, text_off);
	const bool pe = (o->flag & BMH_MEM_F_PE) != 0;
	const size_t nr = (size_t)n, total = (size_t)roff[n], wc = (size_t)first[n], l_rg = rg_id ? strlen(rg_id) : 0;
	if (l_rg > 0x7fffffffu) return BMH_E_ARG;
	SamtextPool P;
	if ((rc = P.plan(n, seqs))) return rc;
	// the device block: everything that goes up, in one piece; then what the kernels make
	const SamtextBlock L = samtext_block(false, nr, total, wc, l_rg, (size_t)P.poff[nr], pe, cig_words, md_bytes);
	HostBuf up(L.up, true);
	SamtextOut O;
	O.toff = (int64_t *)malloc((nr + 1) * 8);
	if (!up.p || !O.toff) {
		ctx->last_error = std::string(who) + ": out of host memory";
		return BMH_E_NOMEM;
	}
	memcpy(up.p + L.roff, roff, (nr + 1) * 8), memcpy(up.p + L.first, first.data(), (nr + 1) * 8);
	memcpy(up.p + L.nw, n_want, nr * 4), memcpy(up.p + L.mq, reg_mapq, total * 4);
	if (pe) memcpy(up.p + L.pd, pd, (nr >> 1) * sizeof(bmh_pairdec_t));
	if (wc) memcpy(up.p + L.wr, results, wc * sizeof(bmh_wanted_res_t));
	if (cig_words) memcpy(up.p + L.cig, cigar_pool, cig_words * 4);
	if (md_bytes) memcpy(up.p + L.md, md_pool, md_bytes);
	slice_copy_flat(n, regs, roff, up.p + L.reg, n_want, want_k, up.p + L.wk);
	samtext_fill_up(up.p, L, o, pes, rg_id, l_rg, P, n, seqs);
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	if (!ctx->h_ststat) BMH_HIP(ctx, hipHostMalloc(&ctx->h_ststat, sizeof(SamtextStatus), hipHostMallocDefault));
	Stager st(ctx);
	st.cnt = {&ctx->stx.h2d_bytes, &ctx->stx.d2h_bytes, &ctx->stx.waits};
	rc = [&]() -> int {
		int e;
		if ((e = ensure(ctx, ctx->d_samtext, L.end)) || (e = st.stage(L.up + 256, 0))) return e;
		uint8_t *d = (uint8_t *)ctx->d_samtext.p;
		BMH_HIP(ctx, hipMemsetAsync(d + L.stat, 0, L.stat_bytes, ctx->stream));
		if ((e = st.h2d(d, up.p, L.up))) return e;
		const SamtextArgs A = samtext_args(ctx, d, L, total, wc, cig_words, md_bytes, n, pe, bns->l_pac);
		if ((e = samtext_size_look(ctx, who, st, A, ctx->h_ststat, L.stat_bytes))) return e;
		return samtext_emit_down(ctx, who, st, A, ctx->h_ststat, L.up + 256, O);
	}();
	if ((rc = st.end(rc)) || (rc = samtext_commit(ctx, who, n, O, text, text_off))) return rc;
	ctx->stx.reads = n, ctx->stx.lines = lines, ctx->stx.text_bytes = O.total;
	return samtext_kernel_ms(ctx, &ctx->stx.size_ms, &ctx->stx.emit_ms);
}

int bmh_ctx_set_samtext_device(bmh_ctx_t *ctx, int on)
{
	if (!ctx) return BMH_E_ARG;
	ctx->samtext_device = on != 0;
	return BMH_OK;
}

int bmh_last_samtext_stats(const bmh_ctx_t *ctx, bmh_samtext_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->stx;
	return BMH_OK;
}

// bmh_sam_batch's pass C (host/sam_post.c; not part of the interface)
__attribute__((visibility("hidden"))) int bmh_samtext_routed_(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n,
                                                              const bmh_seq_t *seqs, const bmh_alnreg_v *regs, const int64_t *roff, const bmh_pairdec_t *pd,
                                                              const int32_t *reg_mapq, const int32_t *n_want, const int32_t *want_k,
                                                              const bmh_wanted_res_t *wr, const uint32_t *cig, const char *md, const char *rg_id,
                                                              char **text, int64_t *text_off)
{
	if (ctx && ctx->samtext_device)
		return bmh_sam_text_device(ctx, o, bns, pes, n, seqs, regs, roff, pd, reg_mapq, n_want, want_k, wr, cig, md, rg_id, text, text_off);
	return bmh_sam_text_batch(o, bns, pes, n, seqs, regs, roff, pd, reg_mapq, n_want, want_k, wr, cig, md, rg_id, text, text_off);
}

// ------------------------------------------------------------------ passes A, B and C of phase 2 as one device session

// what bmh_samtext_check_ refuses of the arguments, the reads and the names (host/sam_post.c; not part of the interface)
int bmh_samtext_check_seqs_(const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs, const bmh_alnreg_v *regs,
                            char **text, int64_t *text_off);
// ... without the vectors: a slice whose regions are on the device already
int bmh_samtext_check_reads_(const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs, char **text,
                             int64_t *text_off);

// ensure() for a block whose first `keep` bytes a session still needs: the new allocation has them before the old one goes.  Every
// pointer into the block is the caller's to make again.  *waited: whether the block moved, which costs the caller one wait.
static int ensure_keep(bmh_ctx *ctx, DevBuf &b, size_t bytes, size_t keep, bool *waited)
{
	*waited = false;
	if (bytes <= b.cap) return BMH_OK;
	DevBuf nb;
	int rc = ensure(ctx, nb, std::max(bytes, 2 * b.cap));
	if (rc) return rc;
	hipError_t e = keep ? hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
	if (e == hipSuccess) e = stream_wait(ctx, ctx->stream);
	if (e != hipSuccess) {
		(void)hipFree(nb.p);
		return set_hip_error(ctx, e, "hipMemcpyAsync(workspace)");
	}
	free_buf(b);
	b = nb;
	*waited = true;
	return BMH_OK;
}

// What the session refuses of its arguments and the context before anything is uploaded, n == 0 included; res: the regions are on the
// device (regs is not looked at).  reads: n entries, made here from seqs.
static int phase2_text_check(bmh_ctx *ctx, const char *who, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes,
                             int n, const bmh_seq_t *seqs, const bmh_alnreg_v *regs, bool res, const char *rg_id, char **text, int64_t *text_off,
                             std::vector<bmh_read_t> &reads)
{
	int rc = res ? bmh_samtext_check_reads_(o, bns, pes, n, seqs, text, text_off) : bmh_samtext_check_seqs_(o, bns, pes, n, seqs, regs, text, text_off);
	if (rc) return rc;
	const size_t nr = (size_t)n;
	reads.resize(nr);
	for (size_t i = 0; i < nr; ++i) { // (what bmh_pp_check_args refuses of the vectors)
		if (!res && ((regs[i].n && !regs[i].a) || regs[i].n > 0x7fffffffu)) return BMH_E_ARG;
		reads[i].l_seq = seqs[i].l_seq, reads[i].seq = (const uint8_t *)seqs[i].seq;
	}
	if ((rc = phase2_check_reads(bns, pac, n, reads.data())) || n == 0) return rc;
	if (!ctx->have_params) return BMH_E_ARG;
	if ((rc = need_resident(ctx, who, bns, pac)) || (rc = need_refnames(ctx, who, bns))) return rc;
	return n > (1 << 28) || (rg_id ? strlen(rg_id) : 0) > 0x7fffffffu ? BMH_E_ARG : BMH_OK;
}

// One session through to the text as the host holds it: the layouts of its three blocks -- pass A's, with pass B's inputs in it, as
// bmh_phase2_device uploads it; pass B's arrays, the overflow area of the redone regions behind them; pass C's in its fused form --
// where the blocks lie on the device, how far the records reach, and every host buffer until the end.
// the bases of a session's reads where an earlier call left them on the device: read i's at bases[soff[i] .. soff[i + 1]), bytes in all
struct ResidentBases {
	const uint8_t *bases;
	const unsigned long long *soff;
	size_t bytes;
};

struct Phase2TextRun {
	bmh_ctx *ctx;
	const char *who;
	const ResidentRegs *res; // not NULL: the regions are on the device, see phase2_text_run
	const ResidentBases *rb; // not NULL: so are the bases, and pass C's per-read pool goes up without them
	Stager st;
	Phase2Plan P;
	SamtextBlock LT;
	size_t up_lo = 0, up_hi = 0; // the part of pass A's upload that is the host's to send
	HostBuf up, tup;             // pass A's and pass C's uploads
	uint8_t *d = nullptr, *dw = nullptr, *dt = nullptr; // d_decide, d_wanted, d_samtext; dw moves where the overflow area outgrows its block
	size_t cig_words = 0, md_bytes = 0; // how far the records reach from the main round's slots
	WantedDown D;
	std::vector<Phase2TextHost> list; // the regions the host redoes, by j
	SamtextOut O;
	// pass C's arguments over the three blocks as they lie and reach now
	SamtextArgs args() const
	{
		SamtextArgs A = samtext_args(ctx, dt, LT, P.Z.total, (size_t)D.n_w, cig_words, md_bytes, P.Z.n, P.pe, P.Z.l_pac, d, &P.LA, dw, &P.LB);
		if (rb) A.bases = rb->bases, A.soff = rb->soff, A.bases_bytes = rb->bytes;
		return A;
	}
	// size and scan again, then the look: SamtextStatus and the SamtextFused behind it
	int look() { return samtext_size_look(ctx, who, st, args(), ctx->h_ptstat, LT.stat_bytes); }
	const SamtextFused *fused() const { return (const SamtextFused *)((const SamtextStatus *)ctx->h_ptstat + 1); }
};

// what the session refuses of the slice itself (*early: see phase2_text_run), then its plan, its layouts and its two uploads, filled
static int phase2_text_plan(Phase2TextRun &S, const bmh_sam_opt_t *o, const bmh_pestat_t *pes, int64_t l_pac, int64_t id0, int n, const bmh_seq_t *seqs,
                            const bmh_read_t *reads, const bmh_alnreg_v *regs, const char *rg_id, bool *early)
{
	bmh_ctx *ctx = S.ctx;
	const ResidentRegs *res = S.res;
	const DecideBlock &LA = S.P.LA;
	const size_t nr = (size_t)n, l_rg = rg_id ? strlen(rg_id) : 0;
	std::vector<int64_t> roff(res ? 0 : nr + 1, 0);
	for (size_t i = 0; !res && i < nr; ++i) roff[i + 1] = roff[i] + (int64_t)regs[i].n; // (the offsets are made here)
	const long long n_regs = res ? res->total : (long long)roff[nr];
	if (n_regs < 0 || n_regs > (1 << 28)) return BMH_E_ARG;
	const size_t total = (size_t)n_regs;
	auto refuse = [&](const std::string &why) {
		ctx->last_error = why;
		ctx->pt.fallbacks = 1, *early = true;
		return BMH_E_RANGE;
	};
	// the slots' addresses as the records hold them (every region may be wanted), then the decide tables
	if (total * BMH_RP_SMALL_CAP > 0xffffffffull || total * kWantMdSlot > 0xffffffffull)
		return refuse(std::string(S.who) + ": the slice's CIGAR or MD slots do not fit 32-bit addresses");
	const char *why;
	int rc = phase2_plan(ctx, o, pes, l_pac, id0, n, reads, regs, res, total, S.P, &why);
	if (rc) return why ? refuse(why) : rc;
	SamtextPool pool;
	if ((rc = pool.plan(n, seqs, S.rb == nullptr))) return rc;
	S.LT = samtext_block(true, nr, total, total, l_rg, (size_t)pool.poff[nr], S.P.pe, 0, 0);
	// (resident regions: the offsets at the block's head and the regions at the upload's tail are not the host's to send)
	S.up_lo = res ? LA.hdr : 0, S.up_hi = res ? LA.reg : LA.up();
	S.up.alloc(S.up_hi), S.tup.alloc(S.LT.up, true), S.O.toff = (int64_t *)malloc((nr + 1) * 8);
	if (!S.up.p || !S.tup.p || !S.O.toff) {
		ctx->last_error = std::string(S.who) + ": out of host memory";
		return BMH_E_NOMEM;
	}
	decide_fill(S.up.p, LA, o, pes, S.P.T, n, regs, res ? nullptr : roff.data());
	wanted_fill(ctx, o->w, n, reads, (uint64_t *)(S.up.p + LA.soff), (WantedHdr *)(S.up.p + LA.whdr), nullptr); // (the bases go up in the per-read pool)
	samtext_fill_up(S.tup.p, S.LT, o, pes, rg_id, l_rg, pool, n, seqs);
	S.cig_words = total * BMH_RP_SMALL_CAP, S.md_bytes = total * kWantMdSlot;
	return BMH_OK;
}

// one upload, passes A and B, the bind kernel, size and scan: three waits; the list of the regions the host redoes, alone, behind a fourth
static int phase2_text_enqueue(Phase2TextRun &S)
{
	bmh_ctx *ctx = S.ctx;
	const DecideBlock &LA = S.P.LA;
	const WantedBlock &LB = S.P.LB;
	const SamtextBlock &LT = S.LT;
	int e;
	// (d_wanted: first[] also where no read has a region)
	if ((e = ensure(ctx, ctx->d_decide, LA.end)) || (e = ensure(ctx, ctx->d_wanted, LB.end)) || (e = ensure(ctx, ctx->d_samtext, LT.end))) return e;
	S.d = (uint8_t *)ctx->d_decide.p, S.dw = (uint8_t *)ctx->d_wanted.p, S.dt = (uint8_t *)ctx->d_samtext.p;
	const SamtextArgs gather = S.args();
	auto upload = [&S](uint8_t *, uint8_t *) -> int {
		bmh_ctx *ctx = S.ctx;
		const size_t total = S.P.Z.total;
		BMH_HIP(ctx, hipMemsetAsync(S.dt + S.LT.stat, 0, S.LT.stat_bytes, ctx->stream));
		if (S.res) { // phase 1's offsets and compact records, from its workspace: nothing of it is read after these two copies
			BMH_HIP(ctx, hipMemcpyAsync(S.d, S.res->roff, ((size_t)S.P.Z.n + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
			if (total) BMH_HIP(ctx, hipMemcpyAsync(S.d + S.P.LA.reg, S.res->reg, total * sizeof(bmh_alnreg_t), hipMemcpyDeviceToDevice, ctx->stream));
		}
		const int e = S.st.h2d(S.d + S.up_lo, S.up.p + S.up_lo, S.up_hi - S.up_lo);
		return e ? e : S.st.h2d(S.dt, S.tup.p, S.LT.up);
	};
	if ((e = phase2_enqueue_ab(ctx, S.who, S.st, S.P, S.up_hi - S.up_lo + LT.up + 512, 0, upload, &gather, S.D))) return e;
	if (S.P.Z.wc) { // what joins pass B's arrays to pass C's input: the slots' addresses into the records, the host's regions into the list
		Phase2TextBindArgs B{};
		B.status = (const WantedStatus *)(S.dw + LB.stat), B.wres = (bmh_wanted_res_t *)(S.dw + LB.wres), B.rec = (const WantRec *)(S.dw + LB.rec);
		B.roff = (const unsigned long long *)S.d, B.reg = (const bmh_alnreg_t *)(S.d + LA.reg), B.total = S.P.Z.total, B.n = S.P.Z.n;
		B.cig_cap = BMH_RP_SMALL_CAP, B.md_cap = kWantMdSlot, B.w_cap = S.P.Z.wc;
		B.list = (Phase2TextHost *)(S.dt + LT.list), B.fused = (SamtextFused *)(S.dt + LT.stat + sizeof(SamtextStatus));
		B.status_out = (SamtextStatus *)(S.dt + LT.stat), B.err = ctx->d_err;
		if ((e = launch_phase2_text_bind(ctx, B, S.D.n_w))) return e;
	} else
		BMH_HIP(ctx, hipMemsetAsync(S.dw + LB.first, 0, ((size_t)S.P.Z.n + 1) * 8, ctx->stream));
	if ((e = S.look())) return e;
	const int32_t n_host = S.fused()->n_host;
	if (n_host == 0) return BMH_OK;
	if (n_host < 0 || (int64_t)n_host > S.D.n_w) { // cannot happen
		ctx->last_error = std::string(S.who) + ": the device's counts are inconsistent";
		return BMH_E_ARG;
	}
	S.list.resize((size_t)n_host);
	BMH_HIP(ctx, hipMemcpyAsync(S.list.data(), S.dt + LT.list, S.list.size() * sizeof(Phase2TextHost), hipMemcpyDeviceToHost, ctx->stream));
	BMH_HIP(ctx, stream_wait(ctx, ctx->stream));
	S.st.waited(S.list.size() * sizeof(Phase2TextHost));
	return BMH_OK;
}

// The overflow area behind pass B's block as it goes up at LB.end: the redone regions' records, their places in want order, their
// CIGAR words and MD bytes.  rec, at, end: where the sections lie in the block; cig_words, md_bytes: how far the records reach with it
struct Phase2TextOverflow {
	std::vector<uint8_t> ov;
	size_t rec, at, end, cig_words, md_bytes;
};
// ... packed from what the host's redo made of list[], the records' offsets counted from the main round's slots, as every record's
static int phase2_text_overflow(bmh_ctx *ctx, const char *who, const WantedBlock &LB, const std::vector<Phase2TextHost> &list, const RedoOut &H, Phase2TextOverflow &V)
{
	const size_t m = list.size();
	size_t cw = 0, mb = 0;
	for (const bmh_wanted_res_t &x : H.hw) cw += (size_t)x.n_cigar, mb += (size_t)x.md_len;
	Block ob;
	ob.at = LB.end;
	V.rec = ob.take(m * sizeof(bmh_wanted_res_t)), V.at = ob.take(m * 8);
	const size_t o_cig = ob.take(cw * 4), o_md = ob.take(mb), cig0 = (o_cig - LB.cig1) / 4, md0 = o_md - LB.md1;
	V.end = ob.at;
	if (cig0 + cw > 0xffffffffull || md0 + mb > 0xffffffffull) {
		ctx->last_error = std::string(who) + ": the redone regions' CIGAR or MD do not fit 32-bit addresses";
		return BMH_E_RANGE;
	}
	V.ov.assign(V.end - LB.end, 0);
	bmh_wanted_res_t *orec = (bmh_wanted_res_t *)(V.ov.data() + (V.rec - LB.end));
	int64_t *oat = (int64_t *)(V.ov.data() + (V.at - LB.end));
	uint32_t *ocig = (uint32_t *)(V.ov.data() + (o_cig - LB.end));
	char *omd = (char *)(V.ov.data() + (o_md - LB.end));
	cw = mb = 0;
	for (size_t t = 0; t < m; ++t) {
		bmh_wanted_res_t x = H.hw[t];
		memcpy(ocig + cw, H.cig + x.cigar_off, 4 * (size_t)x.n_cigar), memcpy(omd + mb, H.md + x.md_off, x.md_len);
		x.cigar_off = (uint32_t)(cig0 + cw), x.md_off = (uint32_t)(md0 + mb), x.flags |= list[t].flags | BMH_WANTED_HOST;
		cw += (size_t)x.n_cigar, mb += (size_t)x.md_len;
		orec[t] = x, oat[t] = list[t].j;
	}
	V.cig_words = cig0 + cw, V.md_bytes = md0 + mb;
	return BMH_OK;
}

// The regions whose alignments outgrew their slots: redone by wanted_redo_host from the sorted region with the coordinates as cut, the
// device gate left around it; their records, CIGAR words and MD bytes go into the overflow area behind pass B's block, the records
// are patched where they lie, and size and scan run again: two more waits, a third where the block had to move
static int phase2_text_redo(Phase2TextRun &S, const bmh_refidx_t *bns, const uint8_t *pac, int w, const bmh_read_t *reads, std::optional<GateGuard> &gate)
{
	bmh_ctx *ctx = S.ctx;
	const WantedBlock &LB = S.P.LB;
	const size_t m = S.list.size();
	int e;
	std::sort(S.list.begin(), S.list.end(), [](const Phase2TextHost &x, const Phase2TextHost &y) { return x.j < y.j; });
	std::vector<RedoRegion> rr(m);
	for (size_t t = 0; t < m; ++t) {
		const Phase2TextHost &x = S.list[t];
		if (x.j < 0 || x.j >= S.D.n_w || x.read < 0 || x.read >= S.P.Z.n || (t && x.j == S.list[t - 1].j)) { // cannot happen
			ctx->last_error = std::string(S.who) + ": the device's list is inconsistent";
			return BMH_E_ARG;
		}
		rr[t] = RedoRegion{x.read, x.reg};
		rr[t].reg.rb = x.rb, rr[t].reg.re = x.re, rr[t].reg.qb = x.qb, rr[t].reg.qe = x.qe;
	}
	RedoOut H;
	gate.reset();
	e = wanted_redo_host(ctx, bns, pac, w, reads, rr, H);
	gate.emplace();
	if (e) return e;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	Phase2TextOverflow V;
	if ((e = phase2_text_overflow(ctx, S.who, LB, S.list, H, V))) return e;
	bool moved;
	if ((e = ensure_keep(ctx, ctx->d_wanted, V.end, LB.end, &moved))) return e;
	if (moved) S.st.waited(0); // (the seventh wait: the block's copy had to arrive before the old one went)
	S.dw = (uint8_t *)ctx->d_wanted.p;
	S.cig_words = V.cig_words, S.md_bytes = V.md_bytes;
	S.st.up_used = 0; // (everything staged so far has arrived; the redo had the staging buffers for itself)
	if ((e = S.st.stage(V.ov.size() + 256, 0))) return e;
	BMH_HIP(ctx, hipMemsetAsync(S.dt + S.LT.stat, 0, S.LT.stat_bytes, ctx->stream));
	if ((e = S.st.h2d(S.dw + LB.end, V.ov.data(), V.ov.size()))) return e;
	if ((e = launch_phase2_text_patch(ctx, (bmh_wanted_res_t *)(S.dw + LB.wres), (const bmh_wanted_res_t *)(S.dw + V.rec), (const int64_t *)(S.dw + V.at),
	                                  (int64_t)m, S.D.n_w, (SamtextStatus *)(S.dt + S.LT.stat), ctx->d_err)))
		return e;
	if ((e = S.look())) return e;
	if (S.fused()->n_host != 0) { // cannot happen
		ctx->last_error = std::string(S.who) + ": the device's counts are inconsistent";
		return BMH_E_ARG;
	}
	return BMH_OK;
}

// The session.  The arguments are checked here; *early: the BMH_E_RANGE is a refusal before any upload (the decide tables, or slot
// addresses past 32 bits), which bmh_sam_batch answers with its other routes.  Nothing of the caller's is written before the end.
// The regions come from the caller's vectors, or -- res, regs being NULL -- from where phase 1 left them on the device with what
// table_plan_kernel found: their offsets and records are then copied on the stream into pass A's block instead of uploaded, and
// everything from launch_decide on is the same.  rb (bmh_pairs_sam_finish): the bases are on the device too; pass C's per-read pool is
// packed without them, its kernels and pass B's gather read them there, and the host's redo reads seqs as ever.
static int phase2_text_run(bmh_ctx *ctx, const char *who, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes,
                           int64_t id0, int n, const bmh_seq_t *seqs, const bmh_alnreg_v *regs, const ResidentRegs *res, const char *rg_id, char **text,
                           int64_t *text_off, bool *early, const ResidentBases *rb = nullptr)
{
	*early = false;
	reset_phase2_text_stats(ctx);
	std::vector<bmh_read_t> reads;
	int rc = phase2_text_check(ctx, who, o, bns, pac, pes, n, seqs, regs, res != nullptr, rg_id, text, text_off, reads);
	if (rc) return rc;
	if (n == 0) return empty_text(text, text_off);
	Phase2TextRun S{ctx, who, res, rb, Stager(ctx)};
	S.st.cnt = {&ctx->pt.h2d_bytes, &ctx->pt.d2h_bytes, &ctx->pt.waits}, S.D.stay = true;
	if ((rc = phase2_text_plan(S, o, pes, bns->l_pac, id0, n, seqs, reads.data(), regs, rg_id, early))) return rc;
	std::optional<GateGuard> gate; // (left around the host's redo, which enters it again through the host form)
	gate.emplace();
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	if (!ctx->h_ptstat) BMH_HIP(ctx, hipHostMalloc(&ctx->h_ptstat, sizeof(SamtextStatus) + sizeof(SamtextFused), hipHostMallocDefault));
	rc = phase2_text_enqueue(S);
	if (!rc && !S.list.empty()) rc = phase2_text_redo(S, bns, pac, o->w, reads.data(), gate);
	if (!rc) rc = samtext_emit_down(ctx, who, S.st, S.args(), ctx->h_ptstat, 0, S.O);
	rc = S.st.end(rc);
	if (rc == BMH_E_CIGAR_CAP) rc = BMH_OK; // a task that outgrew its slots is reported per region, and has been redone
	if (rc) return rc;
	ctx->logk_n = S.P.T.want_log;
	if ((rc = samtext_commit(ctx, who, n, S.O, text, text_off))) return rc;
	bmh_phase2_text_stats_t &s = ctx->pt;
	s.units = S.P.pe ? n >> 1 : n, s.wanted = S.D.n_w, s.fixed = S.D.n_fix, s.redone = (int64_t)S.list.size();
	s.reads = n, s.lines = S.O.lines, s.text_bytes = S.O.total, s.sessions = 1;
	if (ctx->timing) {
		BMH_HIP(ctx, hipEventElapsedTime(&s.decide_ms, ctx->ev_decide[0], ctx->ev_decide[1]));
		if (S.P.Z.wc) {
			if ((rc = wanted_kernel_ms(ctx, &s.wanted_ms))) return rc;
			BMH_HIP(ctx, hipEventElapsedTime(&s.gather_ms, ctx->ev_gather[0], ctx->ev_gather[1]));
		}
	}
	return samtext_kernel_ms(ctx, &s.size_ms, &s.emit_ms);
}

int bmh_phase2_text_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes, int64_t id0, int n,
                           const bmh_seq_t *seqs, const bmh_alnreg_v *regs, const char *rg_id, char **text, int64_t *text_off)
{
	bool early;
	if (!ctx) return BMH_E_ARG;
	return phase2_text_run(ctx, "bmh_phase2_text_device", o, bns, pac, pes, id0, n, seqs, regs, nullptr, rg_id, text, text_off, &early);
}

int bmh_ctx_set_phase2_text_device(bmh_ctx_t *ctx, int on)
{
	if (!ctx) return BMH_E_ARG;
	ctx->phase2_text_device = on != 0;
	return BMH_OK;
}

int bmh_last_phase2_text_stats(const bmh_ctx_t *ctx, bmh_phase2_text_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->pt;
	return BMH_OK;
}

// bmh_sam_batch's three passes as one session (host/sam_post.c; not part of the interface).  *done = 1: *text (malloc'd) and text_off
// are the fused call's.  *done = 0 with BMH_OK: the switch is off, or the call refused the slice before its upload (the statistics then
// say one fall-back), and the caller goes through its other routes.
__attribute__((visibility("hidden"))) int bmh_phase2_text_routed_(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac,
                                                                  const bmh_pestat_t *pes, int64_t id0, int n, const bmh_seq_t *seqs, const bmh_alnreg_v *regs,
                                                                  const char *rg_id, char **text, int64_t *text_off, int *done)
{
	*done = 0;
	if (!ctx || !ctx->phase2_text_device) return BMH_OK;
	bool early;
	const int rc = phase2_text_run(ctx, "bmh_phase2_text_device", o, bns, pac, pes, id0, n, seqs, regs, nullptr, rg_id, text, text_off, &early);
	if (rc == BMH_E_RANGE && early) return BMH_OK;
	*done = rc == BMH_OK;
	return rc;
}

// ------------------------------------------------------------------ single-end reads to SAM text, the regions resident between the phases

static_assert(sizeof(bmh_reads_sam_stats_t) == 64, "bmh_reads_sam_stats_t is part of the interface");

int bmh_reads_sam_device(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int min_seed_len, const bmh_sam_opt_t *o,
                         const bmh_refidx_t *bns, const uint8_t *pac, int64_t id0, int n, const bmh_seq_t *seqs, const char *rg_id, char **text,
                         int64_t *text_off)
{
	static const char *const who = "bmh_reads_sam_device";
	if (!ctx || !so || !co || !o || !bns || !text || !text_off || n < 0 || (n > 0 && !seqs)) return BMH_E_ARG;
	if (o->flag & BMH_MEM_F_PE) {
		ctx->last_error = std::string(who) + ": single-end only (mate rescue lies between the two phases of a paired-end batch: bmh_pairs_sam_device)";
		return BMH_E_ARG;
	}
	// what either phase refuses, phase 1's first, before anything is uploaded
	std::vector<bmh_read_t> reads((size_t)n), again;
	for (int i = 0; i < n; ++i) reads[(size_t)i].l_seq = seqs[i].l_seq, reads[(size_t)i].seq = (const uint8_t *)seqs[i].seq;
	int rc;
	if ((rc = reads_regs_check(ctx, so, co, bns->l_pac, n, reads.data(), min_seed_len, who))) return rc;
	if ((rc = phase2_text_check(ctx, who, o, bns, pac, nullptr, n, seqs, nullptr, true, rg_id, text, text_off, again))) return rc;
	bool early;
	if (n == 0) { // nothing runs
		if ((rc = phase2_text_run(ctx, who, o, bns, pac, nullptr, id0, 0, seqs, nullptr, nullptr, rg_id, text, text_off, &early))) return rc;
		ctx->dstats = bmh_driver_stats_t{};
		if (o->flag & BMH_MEM_F_NO_EXACT) ctx->drop_exact_removed = 0;
		ctx->rs = bmh_reads_sam_stats_t{0, 0, 0, 1, 0, 0, 0, -1.f, 0, 0};
		return BMH_OK;
	}
	ResidentRegs R;
	if ((rc = reads_regs_resident(ctx, so, co, bns->l_pac, n, reads.data(), min_seed_len, o, &R))) return rc;
	rc = phase2_text_run(ctx, who, o, bns, pac, nullptr, id0, n, seqs, nullptr, &R, rg_id, text, text_off, &early);
	ctx->rs.waits_tail = 1 + ctx->pt.waits;
	return rc;
}

int bmh_last_reads_sam_stats(const bmh_ctx_t *ctx, bmh_reads_sam_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->rs;
	return BMH_OK;
}

// ------------------------------------------------------------------ paired-end reads to SAM text: phase 1, the insert-size barrier, mate
// rescue over the resident table, the plan over its output, phase 2 -- the table in d_c2r, then in d_msw, then in pass A's block

static_assert(sizeof(bmh_pairs_sam_stats_t) == 128, "bmh_pairs_sam_stats_t is part of the interface");

// the pair table's refusal needs the table alone: before rescue opens windows of that width
static int pairs_table_refusal(bmh_ctx *ctx, const bmh_sam_opt_t *o, const bmh_pestat_t *pes)
{
	const char *why = nullptr;
	long long kmax, n_term;
	int64_t term_off[4];
	const bmh_ho_plan_t none = BMH_HO_PLAN_INIT;
	if (!decide_tables_from_plan(o, pes, none, 0, &kmax, &n_term, term_off, &why)) return BMH_OK;
	reset_phase2_text_stats(ctx);
	ctx->last_error = why ? why : "bmh_decide_device: the tables are out of range";
	ctx->pt.fallbacks = 1;
	return BMH_E_RANGE;
}

// A paired-end session from behind the barrier: mate rescue over the table `in` and the bases (pool, soff) where they lie -- the
// context's workspaces, or a parked block --, its output table, n_sw and the plan over it in d_msw, then phase 2 from the plan's numbers:
// nothing it ensures or launches touches d_msw.  regions_in, d2h_bytes: phase 1's; park_waits, rb: of a parked session.
static int pairs_rescue_text(bmh_ctx *ctx, const char *who, const bmh_matesw_opt_t *mo, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac,
                             const bmh_pestat_t *pes, int64_t id0, int n, const bmh_seq_t *seqs, const char *rg_id, char **text, int64_t *text_off,
                             const ResidentRegs &in, const uint8_t *pool, const unsigned long long *soff, long long regions_in, long long d2h_bytes,
                             bool pes_given, int park_waits, const ResidentBases *rb)
{
	ResidentRegs R;
	long long n_sw = 0;
	int rc;
	{
		GateGuard gate;
		BMH_HIP(ctx, hipSetDevice(ctx->device));
		int *d_n_sw = nullptr;
		if ((rc = matesw_resident(ctx, bns->l_pac, n >> 1, pool, soff, in, pes, mo, o->mask_level_redun, &R, &d_n_sw, o, &n_sw))) {
			const std::string table_name = "bmh_matesw_table_device"; // the refusals speak as bmh_matesw_device's do
			for (size_t at; (at = ctx->last_error.find(table_name)) != std::string::npos;) ctx->last_error.replace(at, table_name.size(), who);
			return rc;
		}
	}
	bmh_pairs_sam_stats_t &ps = ctx->ps;
	ps = bmh_pairs_sam_stats_t{n, n >> 1, regions_in, in.total, R.total, n_sw, R.kmax, R.pair_kmax, R.opool_cap,
	                           d2h_bytes + ctx->mt.mid_bytes, 0, 1 + park_waits + ctx->mt.waits, pes_given ? 1 : 0, -1.f, R.neg ? 1 : 0, {0, 0, 0, 0, 0, 0}};
	if (ctx->timing) BMH_HIP(ctx, hipEventElapsedTime(&ps.plan_ms, ctx->ev_plan[0], ctx->ev_plan[1]));
	bool early;
	return phase2_text_run(ctx, who, o, bns, pac, pes, id0, n, seqs, nullptr, &R, rg_id, text, text_off, &early, rb);
}

int bmh_pairs_sam_device(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int min_seed_len, const bmh_matesw_opt_t *mo,
                         const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes0, bmh_pestat_t pes_out[4],
                         int64_t id0, int n, const bmh_seq_t *seqs, const char *rg_id, char **text, int64_t *text_off)
{
	static const char *const who = "bmh_pairs_sam_device";
	if (!ctx || !so || !co || !mo || !o || !bns || !text || !text_off || n < 0 || (n > 0 && !seqs)) return BMH_E_ARG;
	if (!(o->flag & BMH_MEM_F_PE)) {
		ctx->last_error = std::string(who) + ": paired-end only (o->flag lacks BMH_MEM_F_PE; single-end reads: bmh_reads_sam_device)";
		return BMH_E_ARG;
	}
	if (n & 1) {
		ctx->last_error = std::string(who) + ": n is odd: reads 2p and 2p+1 are mates";
		return BMH_E_ARG;
	}
	// what either phase refuses, phase 1's first, before anything is uploaded (phase 2's check wants a table: any will do for it)
	bmh_pestat_t pes[4];
	if (pes0) memcpy(pes, pes0, sizeof(pes));
	else {
		memset(pes, 0, sizeof(pes));
		for (bmh_pestat_t &x : pes) x.failed = 1;
	}
	std::vector<bmh_read_t> reads((size_t)n), again;
	for (int i = 0; i < n; ++i) reads[(size_t)i].l_seq = seqs[i].l_seq, reads[(size_t)i].seq = (const uint8_t *)seqs[i].seq;
	int rc;
	if ((rc = reads_regs_check(ctx, so, co, bns->l_pac, n, reads.data(), min_seed_len, who))) return rc;
	if (!pes0 && o->max_ins > BMH_PS_MAX_INS) {
		ctx->last_error = std::string(who) + ": max_ins must be below 2^30 without a table of the caller's: the insert-size word carries the orientation above it";
		return BMH_E_RANGE;
	}
	if ((rc = phase2_text_check(ctx, who, o, bns, pac, pes, n, seqs, nullptr, true, rg_id, text, text_off, again))) return rc;
	bool early;
	if (n == 0) { // nothing runs
		if ((rc = phase2_text_run(ctx, who, o, bns, pac, pes, id0, 0, seqs, nullptr, nullptr, rg_id, text, text_off, &early))) return rc;
		ctx->dstats = bmh_driver_stats_t{};
		if (o->flag & BMH_MEM_F_NO_EXACT) ctx->drop_exact_removed = 0;
		ctx->ps = bmh_pairs_sam_stats_t{0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, pes0 ? 1 : 0, -1.f, 0, {0, 0, 0, 0, 0, 0}};
		if (pes_out) memcpy(pes_out, pes, sizeof(pes));
		return BMH_OK;
	}
	const int64_t l_pac = bns->l_pac;
	// ---- phase 1: the table in d_c2r, the bases in d_pbase, and without a table of the caller's the words
	PairsPhase1 P1;
	if ((rc = pairs_regs_resident(ctx, so, co, l_pac, n, reads.data(), min_seed_len, o, pes0 == nullptr, &P1))) return rc;
	// ---- the insert-size barrier: the table of exactly this call's reads, a host pass over 4 bytes per pair
	if (!pes0 && (rc = bmh_pestat_from_candidates(o, n >> 1, P1.cand.data(), pes, -1))) {
		ctx->last_error = std::string(who) + ": the insert-size words are inconsistent";
		return rc;
	}
	if ((rc = pairs_table_refusal(ctx, o, pes))) return rc;
	if ((rc = pairs_rescue_text(ctx, who, mo, o, bns, pac, pes, id0, n, seqs, rg_id, text, text_off, P1.regs, P1.pool, P1.soff, P1.regions_in, P1.d2h_bytes,
	                            pes0 != nullptr, 0, nullptr)))
		return rc;
	if (pes_out) memcpy(pes_out, pes, sizeof(pes));
	return BMH_OK;
}

int bmh_last_pairs_sam_stats(const bmh_ctx_t *ctx, bmh_pairs_sam_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->ps;
	return BMH_OK;
}

// ------------------------------------------------------------------ the same session cut in two at the barrier (bmh_pairs_sam_begin /
// bmh_pairs_sam_finish): what phase 1 leaves in d_c2r and d_pbase moves into a block that no context's workspace calls touch

} // extern "C"

namespace {

// Parked blocks, per device: taken from and given back to a list that only grows.  hipFree synchronises every stream of its device, so
// nothing in the middle of a chunk calls it: bmh_pairs_parked_trim alone does, for the blocks idle at that moment.
struct ParkBlock {
	void *p = nullptr;
	size_t cap = 0;
};
std::mutex g_park_mu;
std::vector<std::pair<int, ParkBlock>> g_park_idle; // (device, block)

// the smallest idle block of the device that holds `bytes`, else a new one (sized in 1 MiB steps with an eighth of room: batches of a
// chunk are of a size, and a block a little short of the next batch would be of no use to it)
int park_take(bmh_ctx *ctx, size_t bytes, ParkBlock *out)
{
	{
		std::lock_guard<std::mutex> lock(g_park_mu);
		size_t best = g_park_idle.size();
		for (size_t k = 0; k < g_park_idle.size(); ++k)
			if (g_park_idle[k].first == ctx->device && g_park_idle[k].second.cap >= bytes && (best == g_park_idle.size() || g_park_idle[k].second.cap < g_park_idle[best].second.cap))
				best = k;
		if (best != g_park_idle.size()) {
			*out = g_park_idle[best].second;
			g_park_idle.erase(g_park_idle.begin() + (long)best);
			return BMH_OK;
		}
	}
	const size_t cap = (bytes + bytes / 8 + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
	void *p = nullptr;
	BMH_HIP(ctx, hipMalloc(&p, cap));
	*out = ParkBlock{p, cap};
	return BMH_OK;
}

void park_give(int device, ParkBlock &b)
{
	if (!b.p) return;
	std::lock_guard<std::mutex> lock(g_park_mu);
	g_park_idle.emplace_back(device, b);
	b = ParkBlock{};
}

} // namespace

// [roff[n + 1] | the regions | soff[n + 1] | the bases | 16 zero bytes], the last three as d_pbase holds them
struct bmh_pairs_parked {
	int device = 0, n = 0;
	long long total = 0, regions_in = 0, d2h_bytes = 0;
	ParkBlock blk;
	size_t o_reg = 0, o_soff = 0, o_pool = 0, bases = 0, used = 0;
	std::vector<int32_t> l_seq;
};

extern "C" {

static_assert(sizeof(bmh_pairs_parked_info_t) == 24, "bmh_pairs_parked_info_t is part of the interface");

int bmh_pairs_sam_begin(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int min_seed_len, const bmh_sam_opt_t *o,
                        const bmh_refidx_t *bns, int n, const bmh_seq_t *seqs, uint32_t *cand, bmh_pairs_parked_t **parked)
{
	static const char *const who = "bmh_pairs_sam_begin";
	if (!ctx || !so || !co || !o || !bns || !parked || n < 0 || (n > 0 && !seqs)) return BMH_E_ARG;
	if (!(o->flag & BMH_MEM_F_PE)) {
		ctx->last_error = std::string(who) + ": paired-end only (o->flag lacks BMH_MEM_F_PE; single-end reads: bmh_reads_sam_device)";
		return BMH_E_ARG;
	}
	if (n & 1) {
		ctx->last_error = std::string(who) + ": n is odd: reads 2p and 2p+1 are mates";
		return BMH_E_ARG;
	}
	std::vector<bmh_read_t> reads((size_t)n);
	for (int i = 0; i < n; ++i) reads[(size_t)i].l_seq = seqs[i].l_seq, reads[(size_t)i].seq = (const uint8_t *)seqs[i].seq;
	int rc;
	if ((rc = reads_regs_check(ctx, so, co, bns->l_pac, n, reads.data(), min_seed_len, who))) return rc;
	if (cand && o->max_ins > BMH_PS_MAX_INS) {
		ctx->last_error = std::string(who) + ": max_ins must be below 2^30 where the words are collected: the insert-size word carries the orientation above it";
		return BMH_E_RANGE;
	}
	{ // the names, as phase 2 will refuse them: any table and any text pointers will do for this check
		bmh_pestat_t any[4];
		memset(any, 0, sizeof(any));
		char *t = nullptr;
		int64_t t_off = 0;
		if ((rc = bmh_samtext_check_reads_(o, bns, any, n, seqs, &t, &t_off))) return rc;
	}
	std::unique_ptr<bmh_pairs_parked> K(new (std::nothrow) bmh_pairs_parked);
	if (!K) return BMH_E_NOMEM;
	K->device = ctx->device, K->n = n;
	if (n == 0) { // nothing runs, nothing is parked
		*parked = K.release();
		return BMH_OK;
	}
	try {
		K->l_seq.resize((size_t)n);
	} catch (const std::bad_alloc &) {
		return BMH_E_NOMEM;
	}
	for (int i = 0; i < n; ++i) K->l_seq[(size_t)i] = seqs[i].l_seq, K->bases += (size_t)seqs[i].l_seq;
	PairsPhase1 P1;
	if ((rc = pairs_regs_resident(ctx, so, co, bns->l_pac, n, reads.data(), min_seed_len, o, cand != nullptr, &P1))) return rc;
	// ---- the move: the total is the host's only now, so the copies have a wait of their own (finish counts it in waits_mid)
	const size_t nr1 = (size_t)n + 1, total = (size_t)P1.regs.total;
	K->total = P1.regs.total, K->regions_in = P1.regions_in, K->d2h_bytes = P1.d2h_bytes;
	K->o_reg = al256(nr1 * 8), K->o_soff = K->o_reg + al256(total * sizeof(bmh_alnreg_t)), K->o_pool = K->o_soff + al256(nr1 * 8);
	K->used = K->o_pool + K->bases + 16;
	GateGuard gate;
	BMH_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = park_take(ctx, K->used, &K->blk))) return rc;
	uint8_t *d = (uint8_t *)K->blk.p;
	hipError_t e = hipMemcpyAsync(d, P1.regs.roff, nr1 * 8, hipMemcpyDeviceToDevice, ctx->stream);
	if (e == hipSuccess && total) e = hipMemcpyAsync(d + K->o_reg, P1.regs.reg, total * sizeof(bmh_alnreg_t), hipMemcpyDeviceToDevice, ctx->stream);
	// (d_pbase as bases_keep laid it out: the offsets, the reads from al256 behind them, 16 zero bytes)
	if (e == hipSuccess) e = hipMemcpyAsync(d + K->o_soff, P1.soff, K->used - K->o_soff, hipMemcpyDeviceToDevice, ctx->stream);
	const hipError_t w = stream_wait(ctx, ctx->stream); // (also behind a failed enqueue: the block goes back idle)
	if (e != hipSuccess || w != hipSuccess) {
		park_give(K->device, K->blk);
		return set_hip_error(ctx, e != hipSuccess ? e : w, "hipMemcpyAsync(parked block)");
	}
	if (cand) memcpy(cand, P1.cand.data(), (size_t)(n >> 1) * 4);
	*parked = K.release();
	return BMH_OK;
}

int bmh_pairs_sam_finish(bmh_ctx_t *ctx, bmh_pairs_parked_t *parked, const bmh_matesw_opt_t *mo, const bmh_sam_opt_t *o, const bmh_refidx_t *bns,
                         const uint8_t *pac, const bmh_pestat_t pes[4], int64_t id0, int n, const bmh_seq_t *seqs, const char *rg_id, char **text,
                         int64_t *text_off)
{
	static const char *const who = "bmh_pairs_sam_finish";
	if (!ctx) return BMH_E_ARG;
	ctx->park_consumed = false;
	if (!parked || !mo || !o || !bns || !pes || !text || !text_off || n < 0 || (n > 0 && !seqs)) return BMH_E_ARG;
	if (!(o->flag & BMH_MEM_F_PE)) {
		ctx->last_error = std::string(who) + ": paired-end only (o->flag lacks BMH_MEM_F_PE)";
		return BMH_E_ARG;
	}
	if (parked->device != ctx->device) {
		ctx->last_error = std::string(who) + ": the parked block lies on device " + std::to_string(parked->device) + ", this context runs on device " + std::to_string(ctx->device);
		return BMH_E_ARG;
	}
	if (n != parked->n) {
		ctx->last_error = std::string(who) + ": n is " + std::to_string(n) + ", " + std::to_string(parked->n) + " reads were parked";
		return BMH_E_ARG;
	}
	for (int i = 0; i < n; ++i)
		if (seqs[i].l_seq != parked->l_seq[(size_t)i]) {
			ctx->last_error = std::string(who) + ": read " + std::to_string(i) + " has another length than the read that was parked";
			return BMH_E_ARG;
		}
	int rc;
	std::vector<bmh_read_t> again;
	if ((rc = phase2_text_check(ctx, who, o, bns, pac, pes, n, seqs, nullptr, true, rg_id, text, text_off, again))) return rc;
	if (n == 0) { // nothing was parked, nothing runs
		bool early;
		if ((rc = phase2_text_run(ctx, who, o, bns, pac, pes, id0, 0, seqs, nullptr, nullptr, rg_id, text, text_off, &early))) return rc;
		ctx->dstats = bmh_driver_stats_t{};
		ctx->ps = bmh_pairs_sam_stats_t{0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, -1.f, 0, {0, 0, 0, 0, 0, 0}};
		ctx->park_consumed = true;
		delete parked;
		return BMH_OK;
	}
	if ((rc = pairs_table_refusal(ctx, o, pes))) return rc;
	// ---- past the refusals: the handle is this call's, whatever comes of it
	ctx->park_consumed = true;
	std::unique_ptr<bmh_pairs_parked> K(parked);
	const uint8_t *d = (const uint8_t *)K->blk.p;
	ResidentRegs in;
	in.roff = (const unsigned long long *)d, in.reg = (const bmh_alnreg_t *)(d + K->o_reg), in.total = K->total;
	const ResidentBases rb{d + K->o_pool, (const unsigned long long *)(d + K->o_soff), K->bases};
	rc = pairs_rescue_text(ctx, who, mo, o, bns, pac, pes, id0, n, seqs, rg_id, text, text_off, in, rb.bases, rb.soff, K->regions_in, K->d2h_bytes, true, 1, &rb);
	// the block goes back idle once nothing reads it: a successful session has waited for its text; behind an error the stream is drained
	if (rc && hipSetDevice(ctx->device) == hipSuccess) (void)stream_wait(ctx, ctx->stream);
	park_give(K->device, K->blk);
	return rc;
}

int bmh_pairs_finish_consumed(const bmh_ctx_t *ctx) { return ctx && ctx->park_consumed ? 1 : 0; }

void bmh_pairs_parked_free(bmh_pairs_parked_t *parked)
{
	if (!parked) return;
	park_give(parked->device, parked->blk); // (begin left nothing in flight)
	delete parked;
}

int bmh_pairs_parked_info(const bmh_pairs_parked_t *parked, bmh_pairs_parked_info_t *info)
{
	if (!parked || !info) return BMH_E_ARG;
	*info = bmh_pairs_parked_info_t{parked->device, parked->n, (int64_t)parked->total, (int64_t)parked->used};
	return BMH_OK;
}

int bmh_pairs_parked_trim(int device)
{
	std::vector<ParkBlock> gone;
	{
		std::lock_guard<std::mutex> lock(g_park_mu);
		for (size_t k = g_park_idle.size(); k-- > 0;)
			if (g_park_idle[k].first == device) gone.push_back(g_park_idle[k].second), g_park_idle.erase(g_park_idle.begin() + (long)k);
	}
	if (gone.empty()) return BMH_OK;
	int rc = hipSetDevice(device) == hipSuccess ? BMH_OK : BMH_E_HIP;
	for (ParkBlock &b : gone)
		if (rc != BMH_OK || hipFree(b.p) != hipSuccess) rc = BMH_E_HIP;
	return rc;
}

int bmh_driver_stats(const bmh_ctx_t *ctx, bmh_driver_stats_t *st)
{
	if (!ctx || !st) return BMH_E_ARG;
	*st = ctx->dstats;
	return BMH_OK;
}

} // extern "C"
