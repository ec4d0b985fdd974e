// api_ctx.hip -- context lifetime and what every entry point stands on: error text, stage timers, the upload / download arenas, debug hooks,
// memory helpers.  (The extern "C" boundary declared in include/pfmi.h -- the host side of libpfmi.so -- is the api_*.hip files.)
#include "api_internal.h"

#include <map>
#include <mutex>
#include <string>
#include <stdarg.h>
#include <stdio.h>

static thread_local char g_err[1024] = "";

void pf_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Stage timers.  Mode 1 (pfmi_profile(ctx, 1)) synchronises the host after every stage: each stage then starts on an idle GPU
// and its figure includes the host's launch latency (~1 ms for the scan's launch sequence).  Mode 2 leaves the event pairs in the
// stream and reads them when pfmi_kernel_time asks: the pipeline runs as it does unprofiled, the first event of a stage gets its
// time stamp when the previous stage's last kernel retires, so a stage's figure is its kernels' time.
static hipEvent_t pf_kev_get(pfmi_ctx *c) {
    if (!c->kev_pool.empty()) { hipEvent_t e = c->kev_pool.back(); c->kev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
static void pf_kernel_resolve(pfmi_ctx *c, bool keep) {
    for (auto &p : c->kpending) {
        float ms = 0.f;
        if (keep && p.e0 && p.e1 && hipEventSynchronize(p.e1) == hipSuccess && hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
            KernelStat &s = c->kstats[p.name];
            s.ms += ms;
            s.launches += 1;
        }
        if (p.e0) c->kev_pool.push_back(p.e0);
        if (p.e1) c->kev_pool.push_back(p.e1);
    }
    c->kpending.clear();
}
void pf_kernel_begin(pfmi_ctx *c) {
    if (c->profile == 1) (void)hipEventRecord(c->kev0, c->stream);
    else if (c->profile == 2) {
        if (c->kpending.size() >= 4096) pf_kernel_resolve(c, true);
        if (c->kcur) c->kev_pool.push_back(c->kcur);                  // a begin that was never ended (no kernel took the launch): reuse its event
        c->kcur = pf_kev_get(c);
        if (c->kcur) (void)hipEventRecord(c->kcur, c->stream);
    }
}
void pf_kernel_end(pfmi_ctx *c, const char *name) {
    if (c->profile == 2) {
        hipEvent_t e1 = pf_kev_get(c);
        if (e1) (void)hipEventRecord(e1, c->stream);
        c->kpending.push_back({name, c->kcur, e1});                   // (name: a string literal of the caller)
        c->kcur = nullptr;
        return;
    }
    if (c->profile != 1) return;
    (void)hipEventRecord(c->kev1, c->stream);
    (void)hipEventSynchronize(c->kev1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->kev0, c->kev1);
    KernelStat &s = c->kstats[name];
    s.ms += ms;
    s.launches += 1;
}

// ---- host <-> device copies ---------------------------------------------------------------------------------------
// Uploads up to PF_ARENA_MAX bytes are staged in the ctx's pinned arena and copied asynchronously: the caller's buffer is free on
// return and the stream is NOT synchronised, so a chain of entry points (fit -> scan -> pool -> PSIS -> resample) is enqueued
// without a single host round trip.  Larger blocks (traces, parity-mode normals) take the plain synchronous path.
#define PF_ARENA_BYTES (16u << 20)
#define PF_ARENA_MAX (4u << 20)
void pf_arena_reset(pfmi_ctx *c) { c->arena.off = 0; }
int32_t pf_upload(pfmi_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return PFMI_OK;
    if (bytes > PF_ARENA_MAX) {
        PF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
        PF_HIP(hipStreamSynchronize(c->stream));
        pf_arena_reset(c);
        return PFMI_OK;
    }
    PinArena &a = c->arena;
    if (!a.base) {
        void *pp = nullptr;
        PF_HIP(hipHostMalloc(&pp, PF_ARENA_BYTES, hipHostMallocDefault));
        a.base = reinterpret_cast<char *>(pp); a.cap = PF_ARENA_BYTES; a.off = 0;
    }
    if (a.off + bytes > a.cap) {                 // full: everything staged so far must have been consumed before the rewind
        PF_HIP(hipStreamSynchronize(c->stream));
        a.off = 0;
    }
    memcpy(a.base + a.off, src, bytes);
    PF_HIP(hipMemcpyAsync(dst, a.base + a.off, bytes, hipMemcpyHostToDevice, c->stream));
    a.off += (bytes + 255) & ~(size_t)255;
    return PFMI_OK;
}
#define PF_DL_BYTES (4u << 20)
#define PF_DL_MAX (1u << 20)
int32_t pf_download(pfmi_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return PFMI_OK;
    PinArena &a = c->dl;
    if (bytes <= PF_DL_MAX) {
        if (!a.base) {
            void *pp = nullptr;
            PF_HIP(hipHostMalloc(&pp, PF_DL_BYTES, hipHostMallocMapped));          // (the gather kernel of pf_dl_flush writes into it)
            a.base = reinterpret_cast<char *>(pp); a.cap = PF_DL_BYTES; a.off = 0;
        }
        if (a.off + bytes <= a.cap) {
            // (round 5) the copy itself is NOT issued here: every small result of an entry point used to be its own blit kernel in the stream
            // (eight of them, 5 us each, behind the last kernel of a step); pf_dl_flush -- called by the wait -- moves all of them with ONE
            // kernel that writes straight into the page-locked arena.  The sources are result buffers nothing rewrites before the wait.
            static const bool immediate = [] { const char *e = getenv("PFMI_DL_IMMEDIATE"); return e && e[0] == '1'; }();      // A/B: one blit copy per result, at once
            if (immediate) PF_HIP(hipMemcpyAsync(a.base + a.off, src, bytes, hipMemcpyDeviceToHost, c->stream));
            c->dl_pending.push_back(DlPending{dst, a.base + a.off, bytes, c->defer, immediate ? nullptr : static_cast<const char *>(src), immediate});
            a.off += (bytes + 255) & ~(size_t)255;
            return PFMI_OK;
        }
    }
    // a large result: its own copy (pageable destination: blocks until the copy is done).  The staged small results go out FIRST, as their one
    // gather kernel, so that the wait behind this copy finds them delivered instead of paying a launch + a second round trip
    PF_TRY(pf_dl_flush(c));
    PF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return PFMI_OK;
}
static void pf_deferred_drop(pfmi_ctx *c) { c->dl_pending.clear(); c->post_sync.clear(); c->dl.off = 0; }
// ---- one kernel for all staged downloads of a wait: block (x, y) copies slice x of segment y into the page-locked arena (zero copy)
#define PF_DL_NSEG 24
struct DlSegs { const char *src[PF_DL_NSEG]; char *dst[PF_DL_NSEG]; uint32_t bytes[PF_DL_NSEG]; };
__global__ __launch_bounds__(256) void pf_dl_gather_kernel(DlSegs S) {
    const int y = blockIdx.y;
    const char *src = S.src[y];
    char *dst = S.dst[y];
    const uint32_t n = S.bytes[y];
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | n) & 7u) == 0) {
        const uint32_t n8 = n >> 3;
        for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256)
            reinterpret_cast<uint64_t *>(dst)[i] = reinterpret_cast<const uint64_t *>(src)[i];
    } else {
        for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dst[i] = src[i];
    }
}
int32_t pf_dl_flush(pfmi_ctx *c) {
    DlSegs S;
    int n = 0;
    uint32_t big = 0;
    auto launch = [&]() -> int32_t {
        if (n == 0) return PFMI_OK;
        const unsigned gx = big > (64u << 10) ? 32 : big > (4u << 10) ? 4 : 1;
        hipLaunchKernelGGL(pf_dl_gather_kernel, dim3(gx, (unsigned)n), dim3(256), 0, c->stream, S);
        PF_HIP(hipGetLastError());
        n = 0; big = 0;
        return PFMI_OK;
    };
    for (DlPending &q : c->dl_pending) {
        if (q.issued || q.src == nullptr) continue;
        S.src[n] = q.src; S.dst[n] = const_cast<char *>(q.slot); S.bytes[n] = (uint32_t)q.bytes;
        if ((uint32_t)q.bytes > big) big = (uint32_t)q.bytes;
        q.issued = true;
        if (++n == PF_DL_NSEG) PF_TRY(launch());
    }
    return launch();
}
int32_t pf_stream_sync(pfmi_ctx *c) {
    {
        const int32_t rf = pf_dl_flush(c);
        if (rf != PFMI_OK) { pf_deferred_drop(c); return rf; }
    }
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { pf_deferred_drop(c); PF_HIP(e); }        // nothing is delivered after a failed wait
    for (const DlPending &q : c->dl_pending) memcpy(q.dst, q.slot, q.bytes);
    c->dl_pending.clear();
    c->dl.off = 0;
    pf_arena_reset(c);
    // what deferred entry points would have done behind their own wait (pfmi_defer_downloads): the first failure is this wait's result
    int32_t rc = PFMI_OK;
    std::vector<std::function<int32_t()>> hooks;
    hooks.swap(c->post_sync);
    for (auto &h : hooks) { const int32_t r = h(); if (rc == PFMI_OK) rc = r; }
    return rc;
}
// Staged downloads are delivered by the pf_stream_sync of the entry point that queued them.  An entry point that FAILED between queuing and
// waiting leaves entries whose destinations (stack variables, a caller's array) may be gone: every public entry point forgets them first.
// (entries queued under pfmi_defer_downloads stay: their destinations are the caller's until the next wait)
void pf_download_forget(pfmi_ctx *c) {
    size_t w = 0;
    for (size_t i = 0; i < c->dl_pending.size(); ++i) if (c->dl_pending[i].keep) c->dl_pending[w++] = c->dl_pending[i];
    c->dl_pending.resize(w);
    if (w == 0) c->dl.off = 0;
}
// pinned host staging of the callback path (grown on demand, freed in pfmi_destroy)
int32_t ensure_pinned(pfmi_ctx *c, size_t x_bytes, size_t lp_bytes) {
    for (int b = 0; b < 2; ++b) {
        if (x_bytes > c->pin_x_cap) {
            if (c->pin_x[b]) (void)hipHostFree(c->pin_x[b]);
            c->pin_x[b] = nullptr;
            PF_HIP(hipHostMalloc(&c->pin_x[b], x_bytes, hipHostMallocDefault));
        }
        if (lp_bytes > c->pin_lp_cap) {
            if (c->pin_lp[b]) (void)hipHostFree(c->pin_lp[b]);
            c->pin_lp[b] = nullptr;
            PF_HIP(hipHostMalloc(&c->pin_lp[b], lp_bytes, hipHostMallocDefault));
        }
        if (!c->cb_ev[b]) PF_HIP(hipEventCreateWithFlags(&c->cb_ev[b], hipEventDisableTiming));
    }
    if (x_bytes > c->pin_x_cap) c->pin_x_cap = x_bytes;
    if (lp_bytes > c->pin_lp_cap) c->pin_lp_cap = lp_bytes;
    return PFMI_OK;
}

// ---- test / tuning hooks (pfmi_common.h: pf_debug_get) ---------------------------------------------------------------------
namespace {
std::mutex g_dbg_mu;
// key -> value.  A value is an immutable heap string that is NEVER freed or modified once published (a later pfmi_debug_set of the same key
// installs a new string and leaks the old one: a few bytes per call of a test hook), so the pointer pf_debug_get hands out stays valid after
// the mutex is released, whatever other threads set meanwhile.  Unsetting a key erases its entry (the string stays allocated): the
// environment governs that hook again.  (It used to leave a nullptr tombstone, which hid the environment from every later reader of the
// process: after one set / unset of PFMI_ELBO_KERNEL, tests that selected a kernel through the environment ran the default one.)
std::map<std::string, const char *> g_dbg;
}
const char *pf_debug_get(const char *name) {
    {
        std::lock_guard<std::mutex> lk(g_dbg_mu);
        auto it = g_dbg.find(name);
        if (it != g_dbg.end()) return it->second;
    }
    static const bool env_hooks = [] { const char *e = getenv("PFMI_DEBUG_HOOKS"); return e && e[0] == '1'; }();
    return env_hooks ? getenv(name) : nullptr;
}

// a streaming call that was never waited for (pfmi_stream_wait), or that an error exit of the pump left in the "needs drain" state: let what
// is in flight on the side streams finish -- the optimiser still writes the staging trace, a closure's scans their block buffers -- and forget
// the call.  Called by whatever is about to reuse or free that memory.  Drains THIS ctx's streams, never the device.
void stream_abandon(pfmi_ctx *c) {
    for (hipStream_t s : {c->s_opt, c->s_fit, c->s_scan1}) if (s) (void)hipStreamSynchronize(s);
    for (hipStream_t s : c->s_cb) if (s) (void)hipStreamSynchronize(s);
    c->sr.active = false;
    c->stream_pending = false;
    c->stream_drain = false;
}

// a closure optimisation that was never waited for: its rounds still write the staging trace and the closure's buffers on the ctx stream.
// Drains THIS ctx's stream (never the device) and forgets the call; `active` is only cleared here, so no failure path can skip the drain.
void lbc_abandon(pfmi_ctx *c) {
    if (!c->lbc.active) return;
    (void)hipStreamSynchronize(c->stream);
    c->lbc.active = false;
    c->opt_pending = false;
}

extern "C" {

const char *pfmi_last_error(void) { return g_err; }

int32_t pfmi_debug_set(const char *key, const char *value) {
    PF_CHECK(key != nullptr && strncmp(key, "PFMI_", 5) == 0, PFMI_ERR_ARG, "debug_set: keys are the PFMI_* hook names");
    const char *copy = (value && value[0]) ? strdup(value) : nullptr;
    PF_CHECK(copy != nullptr || !(value && value[0]), PFMI_ERR_ARG, "debug_set: out of memory");
    std::lock_guard<std::mutex> lk(g_dbg_mu);
    if (copy) g_dbg[key] = copy;                         // the previous string (if any) is deliberately leaked: readers may still hold it
    else g_dbg.erase(key);
    return PFMI_OK;
}
int32_t pfmi_version(void) { return 100; }

int32_t pfmi_device_count(int32_t *count) {
    PF_CHECK(count != nullptr, PFMI_ERR_ARG, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; pf_set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return PFMI_ERR_HIP; }
    *count = n;
    return PFMI_OK;
}

int32_t pfmi_create(int32_t device, pfmi_ctx **out) {
    PF_CHECK(out != nullptr, PFMI_ERR_ARG, "null out");
    *out = nullptr;
    int n = 0;
    PF_HIP(hipGetDeviceCount(&n));
    PF_CHECK(n > 0, PFMI_ERR_HIP, "no HIP device visible: libpfmi has no CPU fallback");
    PF_CHECK(device >= 0 && device < n, PFMI_ERR_ARG, "device %d out of range (%d devices)", device, n);
    hipDeviceProp_t prop;
    PF_HIP(hipGetDeviceProperties(&prop, device));
    PF_CHECK(strncmp(prop.gcnArchName, "gfx950", 6) == 0, PFMI_ERR_UNSUPPORTED,
             "libpfmi is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
    PF_HIP(hipSetDevice(device));
    pfmi_ctx *c = new pfmi_ctx();
    c->device = device;
    c->ncu = prop.multiProcessorCount;
    PF_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    PF_HIP(hipEventCreate(&c->ev0));
    PF_HIP(hipEventCreate(&c->ev1));
    PF_HIP(hipEventCreate(&c->kev0));
    PF_HIP(hipEventCreate(&c->kev1));
    *out = c;
    return PFMI_OK;
}

int32_t pfmi_destroy(pfmi_ctx *c) {
    if (!c) return PFMI_OK;
    pf_comm_ctx_dying(c);                   // communicators that borrow this context close themselves first (any finaliser order is safe)
    (void)hipSetDevice(c->device);
    stream_abandon(c);
    lbc_abandon(c);
    (void)hipStreamSynchronize(c->stream);
    for (int b = 0; b < 2; ++b) {
        if (c->pin_x[b]) (void)hipHostFree(c->pin_x[b]);
        if (c->pin_lp[b]) (void)hipHostFree(c->pin_lp[b]);
        if (c->cb_ev[b]) (void)hipEventDestroy(c->cb_ev[b]);
    }
    if (c->arena.base) (void)hipHostFree(c->arena.base);
    if (c->dl.base) (void)hipHostFree(c->dl.base);
    (void)hipEventDestroy(c->ev0); (void)hipEventDestroy(c->ev1);
    (void)hipEventDestroy(c->kev0); (void)hipEventDestroy(c->kev1);
    pf_kernel_resolve(c, false);
    for (hipEvent_t e : c->kev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : {c->sg_fit, c->sg_opt, c->sg_scan[0], c->sg_scan[1], c->sg_start}) if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {c->s_opt, c->s_fit, c->s_scan1}) if (s) (void)hipStreamDestroy(s);
    for (hipStream_t s : c->s_cb) if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : c->sg_cb) if (e) (void)hipEventDestroy(e);
    if (c->h_prog) (void)hipHostFree(c->h_prog);
    if (c->lc_status) (void)hipHostFree(c->lc_status);
    if (c->nt_status) (void)hipHostFree(c->nt_status);
    if (c->h_list) (void)hipHostFree(c->h_list);
    (void)hipStreamDestroy(c->stream);
    delete c;                               // every DevBuf of the context, the target's included, frees its memory: no stream carries work
    return PFMI_OK;
}

int32_t pfmi_sync(pfmi_ctx *c) {
    PF_CTX(c);
    return pf_stream_sync(c);
}

int32_t pfmi_timer_start(pfmi_ctx *c) {
    PF_CTX(c);
    PF_HIP(hipEventRecord(c->ev0, c->stream));
    return PFMI_OK;
}
int32_t pfmi_timer_stop(pfmi_ctx *c, double *ms) {
    PF_CTX(c);
    PF_HIP(hipEventRecord(c->ev1, c->stream));
    PF_HIP(hipEventSynchronize(c->ev1));
    float f = 0.f;
    PF_HIP(hipEventElapsedTime(&f, c->ev0, c->ev1));
    if (ms) *ms = f;
    return PFMI_OK;
}
int32_t pfmi_profile(pfmi_ctx *c, int32_t enable) {
    PF_CTX(c);
    PF_CHECK(enable >= 0 && enable <= 2, PFMI_ERR_ARG, "profile: mode %d outside 0..2", enable);
    pf_kernel_resolve(c, false);
    c->profile = enable;
    c->kstats.clear();
    return PFMI_OK;
}
int32_t pfmi_kernel_time(pfmi_ctx *c, const char *name, double *ms, int64_t *launches) {
    PF_CTX(c);
    PF_CHECK(name != nullptr, PFMI_ERR_ARG, "null name");
    pf_kernel_resolve(c, true);                                       // mode 2: waits for the recorded stages
    if (strcmp(name, "qf_handover_lost") == 0) {                      // not a stage: pieces of the scan that ever gave up waiting on this ctx
        if (ms) *ms = 0.0;
        if (launches) *launches = c->qf_lost_total;
        return PFMI_OK;
    }
    if (strncmp(name, "qf:", 3) == 0) {                               // not a stage either: scan launches of one plan (launch_qf_ng), host-side count
        auto pl = c->qf_plans.find(name);
        if (ms) *ms = 0.0;
        if (launches) *launches = (pl == c->qf_plans.end()) ? 0 : pl->second;
        return PFMI_OK;
    }
    if (strncmp(name, "xw:", 3) == 0 || strncmp(name, "mf:", 3) == 0 || strncmp(name, "lane:", 5) == 0) {   // launches of one draw-kernel plan, host-side count
        auto pl = c->draw_plans.find(name);
        if (ms) *ms = 0.0;
        if (launches) *launches = (pl == c->draw_plans.end()) ? 0 : pl->second;
        return PFMI_OK;
    }
    bool sampler_plan = false;                                        // launches of one plan of a step or warm kernel or of the operator surface, host-side count ("hmc", "nuts", ... are the stages)
    for (const char *pre : {"hmc:", "hmc_fused:", "nuts:", "nuts_fused:", "hmc_adapt:", "nuts_adapt:", "hmc_metric:", "nuts_metric:", "hmc_fused_metric:", "nuts_fused_metric:", "chees:", "woodbury:", "woodbury_diag:"}) sampler_plan = sampler_plan || strncmp(name, pre, strlen(pre)) == 0;
    if (sampler_plan) {
        auto pl = c->hmc_plans.find(name);
        if (ms) *ms = 0.0;
        if (launches) *launches = (pl == c->hmc_plans.end()) ? 0 : pl->second;
        return PFMI_OK;
    }
    if (strncmp(name, "chain_diag:", 11) == 0) {                      // counting launches of one plan of pfmi_chain_diagnostics, host-side count
        auto pl = c->cd_plans.find(name);
        if (ms) *ms = 0.0;
        if (launches) *launches = (pl == c->cd_plans.end()) ? 0 : pl->second;
        return PFMI_OK;
    }
    if (strncmp(name, "fit:", 4) == 0 || strncmp(name, "hist:", 5) == 0) {   // launches of one fit-kernel or history-walk plan, host-side count ("fit" and "history" stay the stages)
        auto pl = c->fit_plans.find(name);
        if (ms) *ms = 0.0;
        if (launches) *launches = (pl == c->fit_plans.end()) ? 0 : pl->second;
        return PFMI_OK;
    }
    auto it = c->kstats.find(name);
    if (ms) *ms = (it == c->kstats.end()) ? 0.0 : it->second.ms;
    if (launches) *launches = (it == c->kstats.end()) ? 0 : it->second.launches;
    return PFMI_OK;
}

int32_t pfmi_defer_downloads(pfmi_ctx *c, int32_t mode) {
    PF_CHECK(c != nullptr, PFMI_ERR_ARG, "null pfmi_ctx");
    if (mode < 0) { pf_deferred_drop(c); c->defer = false; return PFMI_OK; }       // cancel: nothing queued is ever delivered
    c->defer = mode != 0;
    return PFMI_OK;
}

// ---- host utility: the seed-hierarchy generator of the Python / C mirrors ------------------------------------------
// out[i] = low 64 bits of Philox4x32-10(counter = (t0 + i, stream), key = seed) -- bit-identical to pf_rand_u64 on the device
// and to pfmi/hostrng.py (which falls back to NumPy when the library predates this entry).  Pure host code, no ctx.
int32_t pfmi_host_rand_u64(uint64_t seed, uint64_t t0, int64_t n, uint32_t stream, uint64_t *out) {
    PF_CHECK(n >= 0 && (out != nullptr || n == 0), PFMI_ERR_ARG, "host_rand_u64: bad arguments");
    const uint32_t key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t t = t0 + (uint64_t)i;
        uint32_t c0 = (uint32_t)t, c1 = (uint32_t)(t >> 32), c2 = stream, c3 = 0u, k0 = key0, k1 = key1;
        for (int r = 0; r < 10; ++r) {
            const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
            const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
            c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        out[i] = (uint64_t)c0 | ((uint64_t)c1 << 32);
    }
    return PFMI_OK;
}
// the same for m generators in one call (out is [m][n] row-major): a host that seeds every run of a batch pays one call, not m
int32_t pfmi_host_rand_u64_multi(int32_t m, const uint64_t *seeds, const uint64_t *t0, int64_t n, uint32_t stream, uint64_t *out) {
    PF_CHECK(m >= 0 && n >= 0 && (m == 0 || (seeds && t0)) && (out != nullptr || (int64_t)m * n == 0), PFMI_ERR_ARG, "host_rand_u64_multi: bad arguments");
    for (int32_t j = 0; j < m; ++j) PF_TRY(pfmi_host_rand_u64(seeds[j], t0[j], n, stream, out + (size_t)j * (size_t)n));
    return PFMI_OK;
}

// ---- device utilities ----------------------------------------------------------------------------------
int32_t pfmi_malloc_dev(pfmi_ctx *c, int64_t bytes, void **dev_ptr) {
    PF_CTX(c);
    PF_CHECK(dev_ptr != nullptr && bytes > 0, PFMI_ERR_ARG, "malloc_dev: bad arguments");
    PF_HIP(hipMalloc(dev_ptr, (size_t)bytes));
    return PFMI_OK;
}
int32_t pfmi_free_dev(pfmi_ctx *c, void *dev_ptr) {
    PF_CTX(c);
    if (dev_ptr) PF_HIP(hipFree(dev_ptr));
    return PFMI_OK;
}
int32_t pfmi_host_alloc(int64_t bytes, void **host_ptr) {
    PF_CHECK(bytes > 0 && host_ptr, PFMI_ERR_ARG, "host_alloc: bad arguments");
    *host_ptr = nullptr;
    PF_HIP(hipHostMalloc(host_ptr, (size_t)bytes, hipHostMallocPortable | hipHostMallocMapped));   // (mapped: the owner-only assembly of a multi-GPU result writes into it from every GPU)
    return PFMI_OK;
}
int32_t pfmi_host_free(void *host_ptr) {
    if (host_ptr) PF_HIP(hipHostFree(host_ptr));
    return PFMI_OK;
}
int32_t pfmi_memcpy_h2d(pfmi_ctx *c, void *dst, const void *src, int64_t bytes) {
    PF_CTX(c);
    return pf_upload(c, dst, src, (size_t)bytes);
}
int32_t pfmi_memcpy_d2h(pfmi_ctx *c, void *dst, const void *src, int64_t bytes) {
    PF_CTX(c);
    return d2h(c, dst, src, (size_t)bytes);
}

}  // extern "C"
