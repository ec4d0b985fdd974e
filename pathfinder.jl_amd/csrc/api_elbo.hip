// api_elbo.hip -- everything that draws from or evaluates the fits: the ELBO scan with its host- and device-closure routes, pfmi_draws,
// pfmi_logpdf, the mixture of fits and the Woodbury operator surface.
#include "api_internal.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <memory>
#include <thread>
#include <vector>

// ---- ELBO ---------------------------------------------------------------------------------------------
// The user's host closure on a staged block of `n` columns.  pfmi_set_callback_threads(ctx, t) with t > 1 -- the reference's `ntasks`
// (src/elbo.jl:3-6, src/resample.jl:85-92 through src/utils.jl:33-49; the caller asserts thread safety, src/multipath.jl:104-108) --
// cuts the block into t contiguous column ranges and calls `fn` on each from its own thread (the calling thread takes the first
// range): same columns, same per-column results, whatever t is.  Threads live for one block: a block is milliseconds of closure
// time, their creation tens of microseconds.
static void host_callback_block(pfmi_ctx *c, const double *X, int d, int64_t n, double *out) {
    const TargetDev &T = c->target;
    int t = c->cb_threads;
    if (t > n) t = (int)n;
    if (t <= 1) { T.fn(X, d, n, out, T.user); return; }
    const int64_t per = (n + t - 1) / t;
    std::vector<std::thread> th;
    th.reserve((size_t)t - 1);
    for (int i = 1; i < t; ++i) {
        const int64_t j0 = (int64_t)i * per, j1 = std::min<int64_t>(n, j0 + per);
        if (j0 >= j1) break;
        try {
            th.emplace_back([=, &T] { T.fn(X + (size_t)j0 * (size_t)d, d, j1 - j0, out + j0, T.user); });
        } catch (...) {                                        // no thread to be had (resource limits): this range runs on the calling thread
            T.fn(X + (size_t)j0 * (size_t)d, d, j1 - j0, out + j0, T.user);
        }
    }
    T.fn(X, d, std::min<int64_t>(n, per), out, T.user);
    for (std::thread &x : th) x.join();
}

// evaluate the host-callback target on `n` columns stored at device pointer d_x; results to d_lp (pinned staging, 64 MB blocks)
int32_t callback_logp(pfmi_ctx *c, const double *d_x, int64_t n, double *d_lp) {
    const int d = c->d;
    int64_t chunk = (int64_t)((64ll << 20) / (sizeof(double) * (size_t)d));
    if (chunk < 1) chunk = 1;
    if (chunk > n) chunk = n;
    PF_TRY(ensure_pinned(c, sizeof(double) * (size_t)chunk * d, sizeof(double) * (size_t)chunk));
    for (int64_t s0 = 0; s0 < n; s0 += chunk) {
        const int64_t ns = (n - s0 < chunk) ? n - s0 : chunk;
        PF_TRY(d2h(c, c->pin_x[0], d_x + (size_t)s0 * d, sizeof(double) * (size_t)ns * d));
        host_callback_block(c, reinterpret_cast<const double *>(c->pin_x[0]), d, ns, reinterpret_cast<double *>(c->pin_lp[0]));
        PF_TRY(pf_upload(c, d_lp + s0, c->pin_lp[0], sizeof(double) * (size_t)ns));
    }
    return PFMI_OK;
}

// chunk of fits whose draws are materialised in HBM at a time for a DEVICE_CALLBACK target (PFMI_DEVCB_CHUNK_MB, default 2048 MB)
int64_t devcb_chunk_fits(const pfmi_ctx *c, int64_t per_fit_doubles, int64_t nf, int64_t N) {
    // the draws of a block of fits live in one scratch buffer: 2 GB by default (config 3: 256 fits of 8 MB).  When a fit's draws are
    // large (config 5: 160 MB) such a block holds a dozen fits and the writer has to cut every fit into workgroups of a few draw groups,
    // each of which streams the whole factor block (857 GB/s written at one GPU's share of config 5); the block then grows until a
    // launch has 16 draw groups per workgroup on two workgroups per CU -- bounded by a quarter of the free device memory
    double mb = 2048.0;
    const char *e = pf_debug_get("PFMI_DEVCB_CHUNK_MB");
    if (e && atof(e) > 0) mb = atof(e);
    else {
        const int64_t ngroups = (N + 15) / 16, ncu = c->ncu > 0 ? c->ncu : 256;
        const int64_t split = ngroups / 16 > 0 ? ngroups / 16 : 1;              // workgroups a fit can be cut into
        const double want_mb = (double)((2 * ncu + split - 1) / split) * sizeof(double) * (double)per_fit_doubles / 1048576.0;
        size_t free_b = 0, total_b = 0;
        if (want_mb > mb && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const double cap_mb = (double)free_b / 4.0 / 1048576.0;
            mb = want_mb < cap_mb ? want_mb : (cap_mb > mb ? cap_mb : mb);
        }
    }
    int64_t chunk = (int64_t)(mb * 1048576.0 / (sizeof(double) * (double)per_fit_doubles));
    if (chunk < 1) chunk = 1;
    if (chunk > nf) chunk = nf > 0 ? nf : 1;
    return chunk;
}

// DEVICE_CALLBACK: the user's kernel on `n` columns at d_x -> d_lp, on the ctx stream.  Failed fits leave their draws unwritten (the
// closure then sees stale memory); their log densities are NaN, like an exception in the reference: `npts` slots of `N` values each
// are patched by status afterwards.
int32_t devcb_logp(pfmi_ctx *c, const double *d_x, int64_t n, double *d_lp, const int32_t *d_points, int64_t npts, int64_t N) {
    pf_kernel_begin(c);
    c->target.dev_fn(d_x, c->d, n, d_lp, (void *)c->stream, c->target.user);
    pf_kernel_end(c, "device_callback");
    PF_HIP(hipGetLastError());
    return pf_launch_nan_failed(c, npts, N, d_points, d_lp);
}

int32_t elbo_reserve(pfmi_ctx *c, size_t P, int32_t K, int64_t N) {
    PF_TRY(c->logp.ensure(sizeof(double) * P * N));
    PF_TRY(c->logq.ensure(sizeof(double) * P * N));
    PF_TRY(c->elbo.ensure(sizeof(double) * P));
    PF_TRY(c->se.ensure(sizeof(double) * P));
    return c->best_iter.ensure(sizeof(int64_t) * K);
}

int32_t devcb_scan_block(pfmi_ctx *c, hipStream_t ss, const int32_t *list, const uint64_t *seeds, int64_t n, int64_t N, const double *d_u,
                         int64_t ustride, double *bx, double *blp) {
    PF_TRY(pf_launch_elbo_draws(c, list, seeds, n, 0, N, d_u, ustride, bx, (int64_t)c->d * N, c->logp.as<double>(), c->logq.as<double>(), N,
                                false, true));
    pf_kernel_begin(c);
    c->target.dev_fn(bx, c->d, n * N, blp, (void *)ss, c->target.user);
    pf_kernel_end(c, "device_callback");
    PF_HIP(hipGetLastError());
    return pf_launch_scatter_rows(c, n, N, list, blp, c->logp.as<double>());
}

extern "C" {

int32_t pfmi_set_callback_threads(pfmi_ctx *c, int32_t nthreads) {
    PF_CTX(c);
    PF_CHECK(nthreads >= 1 && nthreads <= 1024, PFMI_ERR_ARG, "set_callback_threads: 1 <= nthreads <= 1024");
    c->cb_threads = nthreads;
    return PFMI_OK;
}

int32_t pfmi_elbo_batch_enqueue(pfmi_ctx *c, int64_t N, const uint64_t *seeds, const double *u_host) {
    PF_CTX_MUT(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "elbo_batch: call pfmi_fit_batch first");
    PF_CHECK(c->target.kind >= 0, PFMI_ERR_STATE, "elbo_batch: call pfmi_set_target first");
    PF_CHECK(c->target.d == c->d, PFMI_ERR_ARG, "target dimension %d != trace dimension %d", c->target.d, c->d);
    PF_CHECK(N >= 1 && seeds, PFMI_ERR_ARG, "elbo_batch: bad arguments");
    const int64_t P = c->P;
    const int d = c->d;
    c->N_e = N;
    PF_TRY(elbo_reserve(c, (size_t)P, c->K, N));
    // ONE upload (round 4; three copies in the stream cost three 12-us hand-overs between the fit and the scan): the per-point seeds, then
    // the list of fits = every point that is not the first of its path (fit_distributions[2:end]) -- their seeds, then their indices
    int64_t nf = 0;
    for (int k = 0; k < c->K; ++k) nf += c->path_npts(k) - 1;
    const size_t off_ls = sizeof(uint64_t) * (size_t)P, off_li = off_ls + sizeof(uint64_t) * (size_t)(nf > 0 ? nf : 1);
    const size_t up_bytes = off_li + sizeof(int32_t) * (size_t)(nf > 0 ? nf : 1);
    std::vector<char> stage(up_bytes);
    memcpy(stage.data(), seeds, sizeof(uint64_t) * (size_t)P);
    {
        uint64_t *ls = reinterpret_cast<uint64_t *>(stage.data() + off_ls);
        int32_t *li = reinterpret_cast<int32_t *>(stage.data() + off_li);
        int64_t t = 0;
        for (int k = 0; k < c->K; ++k)
            for (int64_t p = c->off[k] + 1; p < c->off[k] + c->path_npts(k); ++p, ++t) { li[t] = (int32_t)p; ls[t] = seeds[p]; }
    }
    PF_TRY(c->seeds.ensure(up_bytes + 16));
    c->d_stream_tab = nullptr;                                  // (the streams of a streaming call lived in this buffer)
    PF_TRY(pf_upload(c, c->seeds.p, stage.data(), up_bytes));
    uint64_t *d_lseeds = reinterpret_cast<uint64_t *>(c->seeds.as<char>() + off_ls);
    int32_t *d_list = reinterpret_cast<int32_t *>(c->seeds.as<char>() + off_li);
    const double *d_u = nullptr;
    if (u_host) {
        PF_TRY(c->ubuf.ensure(sizeof(double) * (size_t)P * d * N));
        PF_TRY(pf_upload(c, c->ubuf.p, u_host, sizeof(double) * (size_t)P * d * N));
        d_u = c->ubuf.as<double>();
    }
    const int64_t ustride = (int64_t)d * N;
    if (c->target.kind == PFMI_TARGET_DEVICE_CALLBACK) {
        // device closure (the reference's general logp kept on the GPU): the draws of a block of fits are materialised in HBM
        // (8 d bytes written per draw), the user's kernel reads them on the same stream (8 d bytes read per draw) and its log
        // densities are scattered into the point-indexed table.  Nothing crosses PCIe, nothing synchronises.
        const int64_t per = (int64_t)d * N;
        int64_t chunk = devcb_chunk_fits(c, per, nf, N);
        // Round 6: the blocks alternate between PF_DCB_NB = 2 streams (two buffers), so that the closure of block i runs beside the writer of block
        // i + 1: the writer is bound by no single resource (SIMD issue ~70 %, LDS pipe ~50 %, HBM writes at half the link) and the closure
        // wants what it leaves idle, HBM reads -- each kernel fills the other's launch tails and memory pipe.  7.90 -> 6.87 ms for 1 403 fits x 1000
        // draws at d = 1000 (2.85 -> 3.27 TB/s moved); a third stream adds nothing.  Same kernels on the same data: the same bits.
        // PFMI_DEVCB_OVERLAP = 0 | 2 (debug hook): one stream (kernel timing) / two.
        int nb = nf > 1 ? PF_DCB_NB : 1;
        if (const char *ov = pf_debug_get("PFMI_DEVCB_OVERLAP")) { const int v = atoi(ov); nb = (v <= 0 || nf <= 1) ? 1 : (v < PF_DCB_NB ? (v < 2 ? 2 : v) : PF_DCB_NB); }
        if (nb > 1) {
            size_t free_b = 0, total_b = 0;
            double have = 0.0;
            for (int b = 0; b < PF_DCB_NB; ++b) have += (double)c->dcb_x[b].cap;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) have += (double)free_b;
            // full-size buffers only when memory is plentiful and there are blocks to alternate; else the same footprint cut into nb blocks
            if ((double)nb * (double)sizeof(double) * (double)chunk * (double)(per + N) > 0.5 * have || chunk * nb > nf) chunk = (chunk + nb - 1) / nb;
            if (chunk < 1) chunk = 1;
        }
        for (int b = 0; b < nb; ++b) {
            PF_TRY(c->dcb_x[b].ensure(sizeof(double) * (size_t)chunk * per));
            PF_TRY(c->dcb_lp[b].ensure(sizeof(double) * (size_t)chunk * N));
        }
        for (int b = 1; b < nb; ++b)
            if (!c->s_cb[b - 1]) PF_HIP(hipStreamCreateWithFlags(&c->s_cb[b - 1], hipStreamNonBlocking));
        for (int b = 0; b < nb; ++b)
            if (!c->sg_cb[b]) PF_HIP(hipEventCreateWithFlags(&c->sg_cb[b], hipEventDisableTiming));
        if (nb > 1) {                                                // the side streams start behind the uploads and the fits
            PF_HIP(hipEventRecord(c->sg_cb[0], c->stream));
            for (int b = 1; b < nb; ++b) PF_HIP(hipStreamWaitEvent(c->s_cb[b - 1], c->sg_cb[0], 0));
        }
        c->cb_bytes_dev = 0.0;
        int64_t blk = 0;
        for (int64_t s0 = 0; s0 < nf; s0 += chunk, ++blk) {
            const int64_t ns = (nf - s0 < chunk) ? nf - s0 : chunk;
            const int b = (int)(blk % nb);
            hipStream_t ss = b ? c->s_cb[b - 1] : c->stream;
            StreamSwap sw(c, ss);
            PF_TRY(devcb_scan_block(c, ss, d_list + s0, d_lseeds + s0, ns, N, d_u, ustride, c->dcb_x[b].as<double>(), c->dcb_lp[b].as<double>()));
            c->cb_bytes_dev += (double)sizeof(double) * (double)ns * (double)per;
        }
        for (int b = 1; b < nb && b < blk; ++b) {                    // the reduction waits for the side streams' blocks
            PF_HIP(hipEventRecord(c->sg_cb[b], c->s_cb[b - 1]));
            PF_HIP(hipStreamWaitEvent(c->stream, c->sg_cb[b], 0));
        }
    } else if (c->target.kind != PFMI_TARGET_HOST_CALLBACK) {
        PF_TRY(pf_launch_elbo_draws(c, d_list, d_lseeds, nf, 0, N, d_u, ustride, nullptr, 0, c->logp.as<double>(),
                                    c->logq.as<double>(), N, true, true));
    } else {
        // host closure (the reference's general logp, src/elbo.jl:15): the draws of a block of fits are materialised on the device,
        // handed to the callback through PINNED staging and the log densities scattered back by one kernel.  Double buffered:
        // while the host evaluates block i, the device already generates and downloads block i + 1.
        const int64_t per = (int64_t)d * N;
        int64_t chunk = (int64_t)((64ll << 20) / (sizeof(double) * (size_t)per));
        if (chunk < 1) chunk = 1;
        if (chunk > nf) chunk = nf > 0 ? nf : 1;
        const size_t xb = sizeof(double) * (size_t)chunk * per, lb = sizeof(double) * (size_t)chunk * N;
        PF_TRY(ensure_pinned(c, xb, lb));
        for (int b = 0; b < 2; ++b) { PF_TRY(c->cb_x[b].ensure(xb)); PF_TRY(c->cb_lp[b].ensure(lb)); }
        c->cb_seconds = 0.0; c->cb_bytes_d2h = 0.0;
        const int64_t nblocks = (nf + chunk - 1) / chunk;
        auto enqueue = [&](int64_t i) -> int32_t {                  // generate block i and start its download
            const int b = (int)(i & 1);
            const int64_t s0 = i * chunk, ns = (nf - s0 < chunk) ? nf - s0 : chunk;
            PF_TRY(pf_launch_elbo_draws(c, d_list + s0, d_lseeds + s0, ns, 0, N, d_u, ustride, c->cb_x[b].as<double>(), per,
                                        c->logp.as<double>(), c->logq.as<double>(), N, false, true));
            PF_HIP(hipMemcpyAsync(c->pin_x[b], c->cb_x[b].p, sizeof(double) * (size_t)ns * per, hipMemcpyDeviceToHost, c->stream));
            PF_HIP(hipEventRecord(c->cb_ev[b], c->stream));
            return PFMI_OK;
        };
        if (nblocks > 0) PF_TRY(enqueue(0));
        for (int64_t i = 0; i < nblocks; ++i) {
            const int b = (int)(i & 1);
            const int64_t s0 = i * chunk, ns = (nf - s0 < chunk) ? nf - s0 : chunk;
            if (i + 1 < nblocks) PF_TRY(enqueue(i + 1));
            PF_HIP(hipEventSynchronize(c->cb_ev[b]));
            const auto t0 = std::chrono::steady_clock::now();
            host_callback_block(c, reinterpret_cast<const double *>(c->pin_x[b]), d, ns * N, reinterpret_cast<double *>(c->pin_lp[b]));
            c->cb_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            c->cb_bytes_d2h += (double)sizeof(double) * (double)ns * (double)per;
            PF_HIP(hipMemcpyAsync(c->cb_lp[b].p, c->pin_lp[b], sizeof(double) * (size_t)ns * N, hipMemcpyHostToDevice, c->stream));
            PF_TRY(pf_launch_scatter_rows(c, ns, N, d_list + s0, c->cb_lp[b].as<double>(), c->logp.as<double>()));
        }
    }
    PF_TRY(pf_launch_elbo_reduce(c));
    c->elbo_done = true;
    c->elbo_pending = true;
    return PFMI_OK;
}

int32_t pfmi_elbo_batch_wait(pfmi_ctx *c, double *elbo, double *se, int64_t *best_iter) {
    PF_CTX(c);
    PF_CHECK(c->elbo_done, PFMI_ERR_STATE, "elbo_batch_wait: call pfmi_elbo_batch_enqueue first");
    c->elbo_pending = false;
    if (elbo) PF_TRY(pf_download(c, elbo, c->elbo.p, sizeof(double) * c->P));
    if (se) PF_TRY(pf_download(c, se, c->se.p, sizeof(double) * c->P));
    if (best_iter) PF_TRY(pf_download(c, best_iter, c->best_iter.p, sizeof(int64_t) * c->K));
    // pieces of the scan that gave up waiting for their fit's constants (they poison their draws; elbo_qf_kernel.hip): the counter is
    // the last word of the hand-over buffer
    auto lost2 = std::make_shared<std::array<uint32_t, 2>>();
    (*lost2)[0] = (*lost2)[1] = 0;
    for (int q = 0; q < 2; ++q)
        if (c->qf_share_s[q].cap >= sizeof(uint32_t))
            PF_TRY(pf_download(c, &(*lost2)[(size_t)q], c->qf_share_s[q].as<char>() + c->qf_share_s[q].cap - sizeof(uint32_t), sizeof(uint32_t)));
    auto after = [c, lost2]() -> int32_t {
        uint32_t lost = (*lost2)[0] + (*lost2)[1];
        for (int q = 0; q < 2; ++q)
            if ((*lost2)[(size_t)q] != 0) (void)hipMemsetAsync(c->qf_share_s[q].as<char>() + c->qf_share_s[q].cap - sizeof(uint32_t), 0, sizeof(uint32_t), c->stream);
        {
            const char *fake = pf_debug_get("PFMI_QF_FAKE_LOST");       // test hook: the first wait of a ctx reports one lost piece (exercises the retry path)
            if (fake && fake[0] == '1' && !c->qf_no_share) lost = 1;
        }
        if (lost != 0) {
            // plain contention (another process on the GPU, CU masking, a profiler serialising dispatch) must not turn into wrong
            // results or a hard failure.  The poisoned scan (and whatever was enqueued behind it) is void; this ctx takes the two-launch cut --
            // no in-kernel wait -- from now on, and the caller is told to enqueue the step again.
            c->qf_no_share = true;
            c->qf_lost_total += lost;
            c->elbo_done = false; c->pooled = false;
            pf_set_error("ELBO scan: %u workgroup(s) gave up waiting for their fit's constants (GPU shared or dispatch serialised?); results discarded, "
                         "later scans on this context use the two-launch cut: enqueue the step again", lost);
            return PFMI_ERR_RETRY;
        }
        return PFMI_OK;
    };
    if (c->defer) { c->post_sync.push_back(after); return PFMI_OK; }
    PF_TRY(pf_stream_sync(c));
    return after();
}

int32_t pfmi_elbo_batch(pfmi_ctx *c, int64_t N, const uint64_t *seeds, const double *u_host, double *elbo,
                        double *se, int64_t *best_iter) {
    PF_TRY(pfmi_elbo_batch_enqueue(c, N, seeds, u_host));
    return pfmi_elbo_batch_wait(c, elbo, se, best_iter);
}

int32_t pfmi_callback_stats(pfmi_ctx *c, double *callback_seconds, double *bytes_to_host) {
    PF_CTX(c);
    if (callback_seconds) *callback_seconds = c->cb_seconds;
    if (bytes_to_host) *bytes_to_host = c->cb_bytes_d2h;
    return PFMI_OK;
}

int32_t pfmi_callback_stats_dev(pfmi_ctx *c, double *bytes_in_hbm) {
    PF_CTX(c);
    if (bytes_in_hbm) *bytes_in_hbm = c->cb_bytes_dev;
    return PFMI_OK;
}

int32_t pfmi_get_elbo_logs(pfmi_ctx *c, int64_t p, double *logp, double *logq) {
    PF_CTX(c);
    PF_CHECK(c->elbo_done, PFMI_ERR_STATE, "get_elbo_logs: call pfmi_elbo_batch first");
    PF_CHECK(p >= 0 && p < c->P, PFMI_ERR_ARG, "point out of range");
    if (logp) PF_TRY(d2h(c, logp, c->logp.as<double>() + (size_t)p * c->N_e, sizeof(double) * c->N_e));
    if (logq) PF_TRY(d2h(c, logq, c->logq.as<double>() + (size_t)p * c->N_e, sizeof(double) * c->N_e));
    return PFMI_OK;
}

int32_t pfmi_draws(pfmi_ctx *c, int64_t p, uint64_t seed, int64_t n0, int64_t N, const double *u_host, double *X,
                   double *logp, double *logq) {
    PF_CTX_MUT(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "draws: call pfmi_fit_batch first");
    PF_CHECK(p >= 0 && p < c->P && N >= 1 && n0 >= 0, PFMI_ERR_ARG, "draws: bad arguments");
    const int d = c->d;
    const bool have_t = c->target.kind >= 0 && c->target.d == d;
    PF_TRY(c->xbuf.ensure(sizeof(double) * (size_t)d * N));
    PF_TRY(c->scratch.ensure(sizeof(double) * 2 * N + 64));
    double *d_lp = c->scratch.as<double>(), *d_lq = d_lp + N;
    int32_t *d_pt = reinterpret_cast<int32_t *>(d_lq + N);
    uint64_t *d_sd = reinterpret_cast<uint64_t *>(d_lq + N) + 1;
    const int32_t pt = (int32_t)p;
    PF_TRY(pf_upload(c, d_pt, &pt, sizeof(int32_t)));
    PF_TRY(pf_upload(c, d_sd, &seed, sizeof(uint64_t)));
    const double *d_u = nullptr;
    if (u_host) {
        PF_TRY(c->ubuf.ensure(sizeof(double) * (size_t)d * N));
        PF_TRY(pf_upload(c, c->ubuf.p, u_host, sizeof(double) * (size_t)d * N));
        d_u = c->ubuf.as<double>();
    }
    const bool cb = have_t && c->target.kind == PFMI_TARGET_HOST_CALLBACK;
    const bool dcb = have_t && c->target.kind == PFMI_TARGET_DEVICE_CALLBACK;
    PF_TRY(pf_launch_elbo_draws(c, d_pt, d_sd, 1, n0, N, d_u, 0, c->xbuf.as<double>(), 0, d_lp, d_lq, N,
                                have_t && !cb && !dcb, false));
    if (cb) PF_TRY(callback_logp(c, c->xbuf.as<double>(), N, d_lp));
    if (dcb) PF_TRY(devcb_logp(c, c->xbuf.as<double>(), N, d_lp, d_pt, 1, N));
    if (X) PF_TRY(d2h(c, X, c->xbuf.p, sizeof(double) * (size_t)d * N));
    if (logp) PF_TRY(d2h(c, logp, d_lp, sizeof(double) * N));
    if (logq) PF_TRY(d2h(c, logq, d_lq, sizeof(double) * N));
    return PFMI_OK;
}

int32_t pfmi_logpdf(pfmi_ctx *c, int64_t p, int64_t N, const double *X, double *out) {
    PF_CTX(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "logpdf: call pfmi_fit_batch first");
    PF_CHECK(p >= 0 && p < c->P && N >= 1 && X && out, PFMI_ERR_ARG, "logpdf: bad arguments");
    PF_TRY(c->xbuf.ensure(sizeof(double) * (size_t)c->d * N));
    PF_TRY(c->scratch.ensure(sizeof(double) * N));
    PF_TRY(pf_upload(c, c->xbuf.p, X, sizeof(double) * (size_t)c->d * N));
    PF_TRY(pf_launch_logpdf(c, p, N, c->xbuf.as<double>(), c->scratch.as<double>()));
    PF_TRY(d2h(c, out, c->scratch.p, sizeof(double) * N));
    return PFMI_OK;
}

// ---- uniform mixture of fits (mixture_kernels.hip) ----------------------------------------------------------
// points validated and uploaded to c->mix (int32), behind them room for comp [K][N] (when the caller keeps none) and lse [N]
static int32_t mixture_stage(pfmi_ctx *c, int32_t K, const int64_t *points, int64_t N, bool own_comp, bool own_lse,
                             int32_t **d_pts, double **d_comp, double **d_lse) {
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "mixture_logpdf: call pfmi_fit_batch first");
    PF_CHECK(K >= 1 && N >= 1 && points, PFMI_ERR_ARG, "mixture_logpdf: bad arguments (K=%d, N=%lld)", (int)K, (long long)N);
    std::vector<int32_t> pts(K);
    for (int32_t k = 0; k < K; ++k) {
        PF_CHECK(points[k] >= 0 && points[k] < c->P, PFMI_ERR_ARG, "mixture_logpdf: point %lld out of range [0, %lld)",
                 (long long)points[k], (long long)c->P);
        pts[k] = (int32_t)points[k];
    }
    const size_t pbytes = ((sizeof(int32_t) * (size_t)K + 7) / 8) * 8;
    const size_t cbytes = own_comp ? sizeof(double) * (size_t)K * N : 0, lbytes = own_lse ? sizeof(double) * (size_t)N : 0;
    PF_TRY(c->mix.ensure(pbytes + cbytes + lbytes));
    char *base = c->mix.as<char>();
    PF_TRY(pf_upload(c, base, pts.data(), sizeof(int32_t) * (size_t)K));
    *d_pts = reinterpret_cast<int32_t *>(base);
    *d_comp = own_comp ? reinterpret_cast<double *>(base + pbytes) : nullptr;
    *d_lse = own_lse ? reinterpret_cast<double *>(base + pbytes + cbytes) : nullptr;
    return PFMI_OK;
}

int32_t pfmi_mixture_logpdf(pfmi_ctx *c, int32_t K, const int64_t *points, int64_t N, const double *X, double *lse, double *comp) {
    PF_CTX_MUT(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "mixture_logpdf: call pfmi_fit_batch first");
    PF_CHECK(X && lse, PFMI_ERR_ARG, "mixture_logpdf: null X or lse");
    int32_t *d_pts;
    double *d_comp, *d_lse;
    PF_TRY(mixture_stage(c, K, points, N, true, true, &d_pts, &d_comp, &d_lse));
    PF_TRY(c->xbuf.ensure(sizeof(double) * (size_t)c->d * N));
    PF_TRY(pf_upload(c, c->xbuf.p, X, sizeof(double) * (size_t)c->d * N));       // once for all K components
    PF_TRY(pf_launch_mixture_logpdf(c, K, d_pts, N, c->xbuf.as<double>(), d_lse, d_comp));
    if (comp) PF_TRY(pf_download(c, comp, d_comp, sizeof(double) * (size_t)K * N));
    PF_TRY(d2h(c, lse, d_lse, sizeof(double) * N));
    return PFMI_OK;
}

int32_t pfmi_mixture_logpdf_dev(pfmi_ctx *c, int32_t K, const int64_t *points, int64_t N, const void *X_dev, void *lse_dev,
                                void *comp_dev) {
    PF_CTX_MUT(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "mixture_logpdf: call pfmi_fit_batch first");
    PF_CHECK(X_dev && lse_dev, PFMI_ERR_ARG, "mixture_logpdf: null X or lse");
    int32_t *d_pts;
    double *d_comp, *d_lse;
    PF_TRY(mixture_stage(c, K, points, N, comp_dev == nullptr, false, &d_pts, &d_comp, &d_lse));
    if (comp_dev) d_comp = reinterpret_cast<double *>(comp_dev);
    return pf_launch_mixture_logpdf(c, K, d_pts, N, reinterpret_cast<const double *>(X_dev), reinterpret_cast<double *>(lse_dev),
                                    d_comp);
}

// ---- remaining Woodbury operator surface ------------------------------------------------------------------
int32_t pfmi_woodbury_apply(pfmi_ctx *c, int64_t p, int32_t op, int64_t N, const double *X, double *out) {
    PF_CTX(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "woodbury_apply: call pfmi_fit_batch first");
    PF_CHECK(p >= 0 && p < c->P && N >= 1 && X && out, PFMI_ERR_ARG, "woodbury_apply: bad arguments");
    PF_CHECK(op >= PFMI_OP_UNWHITEN && op <= PFMI_OP_INVQUAD, PFMI_ERR_ARG, "woodbury_apply: unknown op %d", op);
    const size_t bytes = sizeof(double) * (size_t)c->d * N;
    PF_TRY(c->xbuf.ensure(bytes));
    PF_TRY(c->gbuf.ensure(bytes));
    PF_TRY(c->scratch.ensure(bytes));
    PF_TRY(pf_upload(c, c->xbuf.p, X, bytes));
    double *in = c->xbuf.as<double>(), *o1 = c->gbuf.as<double>(), *o2 = c->scratch.as<double>();
    const double *res = o1;
    switch (op) {
        case PFMI_OP_UNWHITEN: PF_TRY(pf_launch_woodbury_prim(c, 0, p, N, in, o1)); break;
        case PFMI_OP_WHITEN: PF_TRY(pf_launch_woodbury_prim(c, 1, p, N, in, o1)); break;
        case PFMI_OP_RMUL: PF_TRY(pf_launch_woodbury_prim(c, 2, p, N, in, o1)); break;
        case PFMI_OP_INVUNWHITEN: PF_TRY(pf_launch_woodbury_prim(c, 3, p, N, in, o1)); break;
        case PFMI_OP_MUL:                                            // lmul!(F.L, lmul!(F.R, x))
            PF_TRY(pf_launch_woodbury_prim(c, 2, p, N, in, o1));
            PF_TRY(pf_launch_woodbury_prim(c, 0, p, N, o1, o2));
            res = o2; break;
        case PFMI_OP_SOLVE:                                          // ldiv!(F.R, ldiv!(F.L, x))
            PF_TRY(pf_launch_woodbury_prim(c, 1, p, N, in, o1));
            PF_TRY(pf_launch_woodbury_prim(c, 3, p, N, o1, o2));
            res = o2; break;
        case PFMI_OP_QUAD:
            PF_TRY(pf_launch_woodbury_prim(c, 2, p, N, in, o1));
            PF_TRY(pf_launch_colsumsq(c, N, o1, o2));
            return d2h(c, out, o2, sizeof(double) * N);
        case PFMI_OP_INVQUAD:
            PF_TRY(pf_launch_woodbury_prim(c, 1, p, N, in, o1));
            PF_TRY(pf_launch_colsumsq(c, N, o1, o2));
            return d2h(c, out, o2, sizeof(double) * N);
    }
    return d2h(c, out, res, bytes);
}

int32_t pfmi_woodbury_diag(pfmi_ctx *c, int64_t p, double *diag) {
    PF_CTX(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "woodbury_diag: call pfmi_fit_batch first");
    PF_CHECK(p >= 0 && p < c->P && diag, PFMI_ERR_ARG, "woodbury_diag: bad arguments");
    PF_TRY(c->gbuf.ensure(sizeof(double) * c->d));
    PF_TRY(pf_launch_woodbury_diag(c, p, c->gbuf.as<double>()));
    return d2h(c, diag, c->gbuf.p, sizeof(double) * c->d);
}

}  // extern "C"
