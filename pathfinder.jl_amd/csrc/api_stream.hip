// api_stream.hip -- the streaming pipeline: pfmi_stream_enqueue / _seeds / _pump / _wait / _cancel.
#include "api_internal.h"
#include "fit_args.h"
#include <limits.h>

#include <chrono>
#include <stdio.h>
#include <vector>

// ---- streaming pipeline: optimise, fit and scan as ONE dataflow the calling thread schedules -----------------------------------------
// (reference: src/multipath.jl:190-208 runs optimisation, fit and ELBO of a run back to back inside one task; here the K optimisations
// run as one persistent kernel and the fits / scans of the trace points they have ALREADY produced run on the other CUs meanwhile)
//
//   stream s_opt   pf_lbfgs_kernel: one workgroup per path; publishes its point count every PF_STREAM_PUB points into page-locked HOST memory
//   host           pfmi_stream_pump (called by pfmi_stream_wait until the pipeline is drained): reads the counts; once every path that is still
//                  running has recorded l1 points, the segment [l0, l1) of trace positions is complete and its work is launched:
//   stream s_fit   history walk of the segment (state carried from the previous segment) -> fits of the segment's points -> event
//   ctx stream / s_scan1 (alternating)   upload of the segment's work list -> wait for the fits -> ELBO scan of the segment's fits
//   ctx stream     at the end: waits for all of them -> mean / SE / argmax; then whatever the caller enqueues (pool, PSIS, resample)
//
// No kernel waits for another kernel: a consumer is only launched when its inputs are complete (the host saw the count; a kernel launch
// acquires what was released before it), so nothing depends on dispatch order, residency or the number of CUs.  The trace points stay in
// the optimiser's fixed-stride staging buffers (point l of path k = slot k * (maxiters + 1) + l): nothing is packed, no offset depends on
// another path's length.  Same kernels, same arithmetic as fit_batch + elbo_batch_enqueue on the packed trace: bit-identical results
// (tests/test_gpu_stream.py).  Four streams in all -- the default number of hardware queues, so none of them shares a queue.
#define PF_STREAM_PUB 16                   // points between two publications of the optimiser's progress (a power of two; hook PFMI_STREAM_PUB)
static int32_t qf_share_reserve(pfmi_ctx *c, int slot, size_t bytes) {
    DevBuf &b = c->qf_share_s[slot];
    if (b.cap >= bytes) return PFMI_OK;
    PF_TRY(b.ensure(bytes));
    PF_HIP(hipMemsetAsync(b.p, 0, b.cap, c->stream));
    c->qf_epoch_s[slot] = 0;
    return PFMI_OK;
}

// the runs' predrawn seed streams [K][cap]: host copy of the per-point seeds (the scan's work lists are cut from it) + ONE upload of the
// per-point seeds (slot k * cap + l holds stream value l - 1 of run k) and the raw streams (pfmi_pool_build_best: a failed run's draw seed)
static int32_t stream_set_seeds(pfmi_ctx *c, const uint64_t *seeds) {
    const size_t K = (size_t)c->K, cap = (size_t)c->vcap, Pz = K * cap;
    std::vector<uint64_t> stage(2 * Pz);
    for (size_t k = 0; k < K; ++k) {
        stage[k * cap] = 0;
        if (cap > 1) memcpy(stage.data() + k * cap + 1, seeds + k * cap, sizeof(uint64_t) * (cap - 1));
    }
    memcpy(stage.data() + Pz, seeds, sizeof(uint64_t) * Pz);
    PF_TRY(pf_upload(c, c->seeds.p, stage.data(), sizeof(uint64_t) * 2 * Pz));     // on the ctx stream: in front of everything that reads them
    stage.resize(Pz);
    c->sr.seeds_pt.swap(stage);
    c->sr.have_seeds = true;
    return PFMI_OK;
}

static int32_t stream_enqueue_impl(pfmi_ctx *c, int32_t K, const double *x0, int32_t J, int32_t maxiters, double g_tol, double eps, int64_t N,
                                   const uint64_t *seeds) {
    const TargetDev &T = c->target;
    // the producer: the built-in optimiser (one persistent kernel), or -- a DEVICE_CALLBACK target with a gradient closure -- the rounds of the
    // closure optimiser, issued by the pump on s_opt; the closure's scans then write the draws and call the value closure segment by segment
    const bool closure = T.kind == PFMI_TARGET_DEVICE_CALLBACK && T.grad_fn != nullptr;
    PF_CHECK(T.kind == PFMI_TARGET_GAUSS || T.kind == PFMI_TARGET_FUNNEL || closure, PFMI_ERR_UNSUPPORTED,
             "stream_enqueue: needs a built-in target or a DEVICE_CALLBACK target with a gradient closure (the optimiser runs on the device)");
    PF_CHECK(K > 0 && x0 && maxiters >= 0 && N >= 1, PFMI_ERR_ARG, "stream_enqueue: bad arguments");
    PF_CHECK(J >= 1 && J <= 16, PFMI_ERR_UNSUPPORTED, "stream_enqueue: history_length %d outside 1..16", J);
    // a previous streaming call that was never waited for (a host exception between enqueue and wait) or that an error exit left to be
    // drained: drain and forget it, like pfmi_set_traces / pfmi_optimize_batch_enqueue do -- a persistent context must stay usable.
    // A packed closure optimisation still in flight writes the same staging trace: drained too.
    if (c->sr.active || c->stream_drain) stream_abandon(c);
    lbc_abandon(c);
    hmc_forget(c);
    if (c->s_opt) PF_TRY(pf_stream_sync(c));      // the page-locked progress words and work lists are reused: the previous call's copies must have landed
    const int ncu = c->ncu > 0 ? c->ncu : 256;
    const int d = T.d;
    // (the built-in optimiser keeps a path's vectors in registers; the closure's round kernel walks memory: any d the memory check admits)
    PF_CHECK(closure || d <= 16384, PFMI_ERR_UNSUPPORTED, "stream_enqueue: the device optimiser takes d <= 16384");
    const int64_t cap = (int64_t)maxiters + 1, P = (int64_t)K * cap;
    PF_CHECK(P < (1ll << 31), PFMI_ERR_UNSUPPORTED, "stream_enqueue: too many trace slots");
    const int kpad = pf_kpad_for(J);
    const int64_t nf = (int64_t)K * (cap - 1);
    int64_t dcb_chunk = 1;
    {   // the fixed-stride layout sizes every per-point buffer for the LONGEST possible path: refuse what the device cannot hold
        size_t free_b = 0, total_b = 0;
        double need = 8.0 * (double)P * ((double)d * (kpad + 5) + 2.0 * (double)N + 4.0 * kpad * kpad);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            double have = (double)free_b;
            for (const DevBuf *b : {&c->vh, &c->alpha_all, &c->sqrt_alpha, &c->mu, &c->logp, &c->logq, &c->st_theta, &c->st_grad}) have += (double)b->cap;
            if (closure) {
                // the closure optimiser's own footprint (lbc_enqueue's line without the staging trace, counted above) and the scans' two
                // block buffers of draws + log densities (one per scan stream), sized as pfmi_elbo_batch_enqueue sizes them
                for (const DevBuf *b : {&c->lc_X, &c->lc_out, &c->lc_x, &c->lc_g, &c->lc_p, &c->lb_hs, &c->lb_hy, &c->dcb_x[0], &c->dcb_x[1],
                                        &c->dcb_lp[0], &c->dcb_lp[1]}) have += (double)b->cap;
                need += 8.0 * K * ((6.0 + 2.0 * J) * d + 1.0) + (double)K * pf_lbc_path_state_bytes(J);
                const int64_t per = (int64_t)d * N;
                dcb_chunk = devcb_chunk_fits(c, per, nf, N);
                if (2.0 * sizeof(double) * (double)dcb_chunk * (double)(per + N) > 0.5 * have) dcb_chunk = (dcb_chunk + 1) / 2;
                if (dcb_chunk < 1) dcb_chunk = 1;
                need += 2.0 * sizeof(double) * (double)dcb_chunk * (double)(per + N);
            }
            PF_CHECK(need < 0.8 * have, PFMI_ERR_UNSUPPORTED, "stream_enqueue: the fixed-stride layout needs %.1f GB for %d paths x %lld slots "
                     "(%.1f GB available): use the packed route", need / 1e9, K, (long long)cap, have / 1e9);
        } else if (closure) {
            dcb_chunk = devcb_chunk_fits(c, (int64_t)d * N, nf, N);
        }
    }
    // ---- every allocation BEFORE the first launch (a hipFree behind a grown buffer would synchronise the device in mid-flight)
    const size_t Pz = (size_t)P, dz = (size_t)d;
    // the room of ONE upload: the per-point seeds (slot k * cap + l holds stream value l - 1 of run k), then the raw streams; behind them the
    // scan's work lists (filled segment by segment from h_list)
    const size_t off_tab = sizeof(uint64_t) * Pz, off_ls = off_tab + sizeof(uint64_t) * Pz;
    const size_t off_li = off_ls + sizeof(uint64_t) * (size_t)(nf > 0 ? nf : 1);
    const size_t all_bytes = off_li + sizeof(int32_t) * (size_t)(nf > 0 ? nf : 1);
    PF_TRY(staging_reserve(c, K, (size_t)cap, d));
    PF_TRY(c->hs_ial.ensure(sizeof(double) * (size_t)K * dz));
    PF_TRY(c->hs_nacc.ensure(sizeof(int32_t) * K));
    PF_TRY(elbo_reserve(c, Pz, K, N));
    PF_TRY(c->seeds.ensure(all_bytes + 16));
    PF_TRY(c->d_off.ensure(sizeof(int64_t) * (K + 1)));
    PF_TRY(c->d_path_of.ensure(sizeof(int32_t) * Pz));
    for (int q = 0; q < 2; ++q) PF_TRY(qf_share_reserve(c, q, (size_t)ncu * 1700 * sizeof(double) + ((size_t)ncu + 1) * sizeof(unsigned) + (64 << 10)));
    if (closure) {
        PF_TRY(pf_lbc_alloc(c, K, J, d));
        for (int q = 0; q < 2; ++q) {                                   // block buffers of the scans: one per scan stream (ctx stream, s_scan1)
            PF_TRY(c->dcb_x[q].ensure(sizeof(double) * (size_t)dcb_chunk * dz * (size_t)N));
            PF_TRY(c->dcb_lp[q].ensure(sizeof(double) * (size_t)dcb_chunk * (size_t)N));
        }
    }
    if (!c->s_opt) {
        int lo = 0, hi = 0;
        PF_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));              // (hi is the numerically smaller = more urgent one)
        PF_HIP(hipStreamCreateWithPriority(&c->s_opt, hipStreamNonBlocking, hi));     // the producer and the fits go in front of queued scan workgroups
        PF_HIP(hipStreamCreateWithPriority(&c->s_fit, hipStreamNonBlocking, hi));
        PF_HIP(hipStreamCreateWithFlags(&c->s_scan1, hipStreamNonBlocking));
        for (hipEvent_t *e : {&c->sg_fit, &c->sg_opt, &c->sg_scan[0], &c->sg_scan[1], &c->sg_start}) PF_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    if (c->h_prog_cap < 2 * K) {
        if (c->h_prog) (void)hipHostFree(c->h_prog);
        c->h_prog = nullptr; c->h_prog_cap = 0;
        PF_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_prog), sizeof(int32_t) * 2 * (size_t)K, hipHostMallocCoherent | hipHostMallocMapped));
        c->h_prog_cap = 2 * K;
    }
    const size_t list_bytes = (size_t)(nf > 0 ? nf : 1) * (sizeof(uint64_t) + sizeof(int32_t));
    if (c->h_list_cap < list_bytes) {
        if (c->h_list) (void)hipHostFree(c->h_list);
        c->h_list = nullptr; c->h_list_cap = 0;
        PF_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_list), list_bytes, hipHostMallocDefault));
        c->h_list_cap = list_bytes;
    }
    PF_TRY(fit_reserve(c, Pz, K, dz, J, kpad));       // (last of them: it ends with the hist_src clear, this call's first operation on the ctx stream)
    // ---- host-side layout: slot offsets
    const bool same_layout = c->virt && c->K == K && c->vcap == cap && c->d == d && (int64_t)c->path_of.size() == P;
    c->off.assign((size_t)K + 1, 0);
    for (int k = 0; k <= K; ++k) c->off[(size_t)k] = (int64_t)k * cap;
    if (!same_layout) {
        c->path_of.resize(Pz);
        for (int k = 0; k < K; ++k)
            for (int64_t l = 0; l < cap; ++l) c->path_of[(size_t)(k * cap + l)] = k;
    }
    c->K = K; c->d = d; c->P = P; c->J = J; c->kpad = kpad; c->N_e = N; c->virt = true; c->vcap = cap;
    c->npts_h.assign((size_t)K, 0);
    results_reset(c); c->opt_pending = false;
    c->d_stream_tab = reinterpret_cast<const uint64_t *>(c->seeds.as<char>() + off_tab);
    PF_TRY(pf_upload(c, c->lb_x0.p, x0, sizeof(double) * (size_t)K * dz));
    PF_TRY(pf_upload(c, c->d_off.p, c->off.data(), sizeof(int64_t) * (K + 1)));
    if (!same_layout) PF_TRY(pf_upload(c, c->d_path_of.p, c->path_of.data(), sizeof(int32_t) * Pz));
    // slots no path reaches: PFMI_FIT_ABSENT, j_eff 0, NaN ELBO (0xFF.. is a NaN) -- nothing is ever launched for them
    PF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->status.p), PFMI_FIT_ABSENT, Pz, c->stream));
    PF_HIP(hipMemsetAsync(c->hist_len.p, 0, sizeof(int32_t) * Pz, c->stream));
    PF_HIP(hipMemsetAsync(c->elbo.p, 0xFF, sizeof(double) * Pz, c->stream));
    PF_HIP(hipMemsetAsync(c->se.p, 0xFF, sizeof(double) * Pz, c->stream));
    PF_HIP(hipMemsetAsync(c->st_npts.p, 0, sizeof(int32_t) * K, c->stream));
    for (int i = 0; i < 2 * K; ++i) __atomic_store_n(c->h_prog + i, 0, __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    pfmi_ctx::StreamRun &R = c->sr;
    {
        std::vector<uint64_t> keep;
        keep.swap(R.seeds_pt);
        R = pfmi_ctx::StreamRun();
        R.seeds_pt.swap(keep);
    }
    R.K = K; R.J = J; R.cap = (int)cap; R.N = N; R.eps = eps; R.closure = closure; R.dcb_chunk = dcb_chunk;
    R.d_lseeds = reinterpret_cast<uint64_t *>(c->seeds.as<char>() + off_ls);
    R.d_list = reinterpret_cast<int32_t *>(c->seeds.as<char>() + off_li);
    // a segment should fill at least half the CUs with one workgroup per fit
    R.pub = PF_STREAM_PUB;
    // when are the segments cut?  Few paths (one publication step = at most one round of CUs): at FIXED, geometrically growing positions, as soon
    // as a segment's inputs are complete.  Many paths: whenever a scan stream is free, with everything that has arrived meanwhile
    // (profiles/r05_experiments.md section 4: 8 / 16 paths 3.94 / 6.84 against 4.01 / 6.93 ms, and far less sensitive to what else
    // shares the hardware queues; 32 / 64 paths 12.66 / 24.29 against 12.46 / 24.03 ms)
    R.policy = (K * PF_STREAM_PUB <= ncu) ? 1 : 0;
    { const char *po = pf_debug_get("PFMI_STREAM_POLICY"); if (po) R.policy = atoi(po); }
    { const char *fe = pf_debug_get("PFMI_STREAM_FIT_EAGER"); R.fit_eager = fe ? atoi(fe) : 1; }
    { const char *pb = pf_debug_get("PFMI_STREAM_PUB"); if (pb && (atoi(pb) == 4 || atoi(pb) == 8 || atoi(pb) == 32)) R.pub = atoi(pb); }
    R.minlen = ((ncu / 2 + K - 1) / K + R.pub - 1) / R.pub * R.pub;
    if (R.minlen < R.pub) R.minlen = R.pub;
    { const char *ml = pf_debug_get("PFMI_STREAM_MINLEN"); if (ml && atoi(ml) > 0) R.minlen = (atoi(ml) + R.pub - 1) / R.pub * R.pub; }
    if (seeds) PF_TRY(stream_set_seeds(c, seeds));
    c->stream_pending = true;
    PF_HIP(hipEventRecord(c->sg_start, c->stream));
    for (hipStream_t s : {c->s_opt, c->s_fit, c->s_scan1}) PF_HIP(hipStreamWaitEvent(s, c->sg_start, 0));
    c->lbc.rounds = 0; c->lbc.columns = 0;
    {   // ---- the producer
        StreamSwap sw(c, c->s_opt);
        pf_kernel_begin(c);
        if (closure) {
            // its init kernel now; the rounds (closure + step kernel, on s_opt) are issued by the pump.  Every round that records a row
            // publishes the count, so R.pub only sets where the segments may be cut.
            lbc_begin(c, K, J, maxiters, g_tol, c->h_prog);
            PF_TRY(pf_launch_lbc_init(c, c->s_opt));
        } else {
            PF_TRY(pf_launch_lbfgs(c, K, J, maxiters, g_tol, c->lb_x0.as<double>(), R.pub - 1, c->h_prog));
        }
        pf_kernel_end(c, "optimize");
        PF_HIP(hipEventRecord(c->sg_opt, c->s_opt));
    }
    R.active = true;
    R.t_progress = R.t_start = std::chrono::steady_clock::now();
    return PFMI_OK;
}

// One scheduling pass: launches the next segment when its inputs are complete (and a scan stream is free), finishes the call when the last
// one is out.  *finished = 1: everything is enqueued (pfmi_stream_wait then returns at once).  Never blocks.
static int32_t stream_pump_pass(pfmi_ctx *c, int32_t *finished) {
    pfmi_ctx::StreamRun &R = c->sr;
    if (finished) *finished = R.active ? 0 : 1;
    if (!R.active) return PFMI_OK;
    const int K = R.K;
    // a closure producer: the rounds it may have in flight are issued first (the gradient closure is called here, on s_opt).  Once the
    // optimisation has finished -- no path running, or the hard cap -- every published count is final.
    if (R.closure && !c->lbc.finished) PF_TRY(lbc_issue_rounds(c, c->s_opt));
    const bool opt_over = R.closure && c->lbc.finished;
    bool all_done = true;
    int avail = INT_MAX, lmax = 0;
    for (int k = 0; k < K; ++k) {
        const int dn = opt_over ? 1 : __atomic_load_n(c->h_prog + K + k, __ATOMIC_ACQUIRE);     // flag first: a raised flag means the count is final
        const int n = __atomic_load_n(c->h_prog + k, __ATOMIC_ACQUIRE);
        c->npts_h[(size_t)k] = dn ? n : -n;                                           // (negative: still running, at least that many points)
        if (!dn) { all_done = false; if (n < avail) avail = n; }
        if (n > lmax) lmax = n;
    }
    if (!R.have_seeds) return PFMI_OK;                                              // pfmi_stream_seeds has not been called yet
    const auto now = std::chrono::steady_clock::now();
    if (!all_done) {
        // Watchdog.  The producer is a plain kernel: it runs, or its stream carries an error.  An ERROR ends the call at once; no
        // progress alone ends it only after PFMI_STREAM_TIMEOUT_S seconds (default 60: a host that pumps rarely or a GPU shared with another
        // process must not trip it), and never with a device-wide synchronise -- that would block for ever behind a hung kernel and stall
        // every other context of the device.  The context's own side streams are drained by the next entry point that reuses its memory.
        // An error exit leaves the call in the "needs drain" state (stream_drain): the next entry point that reuses its memory drains the
        // side streams.
        const hipError_t q = hipStreamQuery(c->s_opt);
        if (q != hipSuccess && q != hipErrorNotReady) {
            R.active = false; c->stream_pending = false; c->stream_drain = true;
            PF_CHECK(false, PFMI_ERR_HIP, "stream_pump: the optimiser's stream reports %s", hipGetErrorString(q));
        }
        const int64_t rnd = R.closure ? c->lbc.seen : -1;                            // a closure round that has completed is progress too
        if (avail != R.last_min || rnd != R.last_round) { R.last_min = avail; R.last_round = rnd; R.t_progress = now; }
        else {
            double limit = 60.0;
            if (const char *tl = pf_debug_get("PFMI_STREAM_TIMEOUT_S")) { const double v = atof(tl); if (v > 0) limit = v; }
            if (std::chrono::duration<double>(now - R.t_progress).count() > limit) {
                R.active = false; c->stream_pending = false; c->stream_drain = true;
                PF_CHECK(false, PFMI_ERR_HIP, "stream_pump: the optimiser made no progress for %.0f s (stream state: %s)", limit, hipGetErrorString(q));
            }
        }
    }
    int l1 = all_done ? lmax : avail / R.pub * R.pub;
    if (l1 > R.cap) l1 = R.cap;
    const int l0 = R.l_next;
    // at most one scan launch queued per scan stream: the next segment then takes everything that has arrived meanwhile
    int q_free = -1;
    for (int q = 0; q < 2 && q_free < 0; ++q) {
        const int qq = (R.nseg + q) & 1;
        if (!R.scan_used[qq] || hipEventQuery(c->sg_scan[qq]) == hipSuccess) q_free = qq;
    }
    if (R.policy == 1) {
        // fixed boundaries (geometric): a segment goes out as soon as its positions are complete, whatever the scan streams are doing
        static const int step[] = {1, 1, 2, 2, 2, 4, 4, 8, 8, 16};               // in publication steps: 16, 32, 64, 96, 128, 192, 256, 384, ... at 16 points
        int bnd = 0, i = 0;
        while (bnd <= l0) { bnd += R.pub * step[i < 10 ? i : 9]; ++i; }
        if (!all_done) {
            if (l1 < bnd) return PFMI_OK;
            l1 = bnd;
        }
        q_free = R.nseg & 1;
    } else {
        if (!all_done && (l1 - l0 < R.minlen || q_free < 0)) return PFMI_OK;
        if (R.policy == 2 && !all_done) {
            // not behind a much larger launch that has just started: a small segment's fits would wait a round for CUs and its scan would
            // block its stream for the work that arrives meanwhile
            const int other = q_free ^ 1;
            if (R.scan_used[other] && hipEventQuery(c->sg_scan[other]) != hipSuccess && (int64_t)K * (l1 - l0) * 2 < R.scan_ns[other]) return PFMI_OK;
        }
        if (q_free < 0) q_free = R.nseg & 1;
    }
    if (l1 > l0) {
        // ---- the walk and the fits: of EVERYTHING that has arrived, not only of this segment.  Once the chip is full of scan workgroups
        //      (0.5 ms each, not preemptible) a fit launch waits for the next round boundary whatever its size; one launch that covers all
        //      the positions available then spares the later segments that wait (measured: 8 paths 3.99 -> 3.97 ms, 64 paths 24.23 -> 24.10 ms end to end;
        //      PFMI_STREAM_FIT_EAGER = 0 restores per-segment fits)
        if (R.l_fit < l1) {
            int lf = all_done ? lmax : avail / R.pub * R.pub;
            if (lf > R.cap) lf = R.cap;
            if (lf < l1) lf = l1;
            if (R.fit_eager == 0) lf = l1;
            StreamSwap sw(c, c->s_fit);
            const HistSeg sg{c->st_npts.as<int32_t>(), R.l_fit, lf, c->hs_ial.as<double>(), c->hs_nacc.as<int32_t>(), c->hinit};
            PF_TRY(pf_launch_history(c, R.eps, &sg));
            PF_TRY(pf_launch_fit(c, R.l_fit, lf - R.l_fit));
            PF_HIP(hipEventRecord(c->sg_fit, c->s_fit));
            R.l_fit = lf;
        }
        // ---- its scan: the fits that exist, position-major
        uint64_t *hs = reinterpret_cast<uint64_t *>(c->h_list);
        int32_t *hl = reinterpret_cast<int32_t *>(c->h_list + sizeof(uint64_t) * (size_t)((int64_t)K * (R.cap - 1) > 0 ? (int64_t)K * (R.cap - 1) : 1));
        int64_t t = R.s0;
        for (int l = l0 > 1 ? l0 : 1; l < l1; ++l)
            for (int k = 0; k < K; ++k) {
                const int n = c->npts_h[(size_t)k];
                if (n >= 0 && l >= n) continue;                                       // the path ended before this position
                const int64_t pp = (int64_t)k * R.cap + l;
                hl[t] = (int32_t)pp; hs[t] = R.seeds_pt[(size_t)pp]; ++t;
            }
        const int64_t ns = t - R.s0;
        if (ns > 0) {
            const int qq = q_free;
            hipStream_t ss = qq == 0 ? c->stream : c->s_scan1;
            StreamSwap sw(c, ss, qq, !all_done);
            PF_HIP(hipMemcpyAsync(R.d_lseeds + R.s0, hs + R.s0, sizeof(uint64_t) * (size_t)ns, hipMemcpyHostToDevice, ss));
            PF_HIP(hipMemcpyAsync(R.d_list + R.s0, hl + R.s0, sizeof(int32_t) * (size_t)ns, hipMemcpyHostToDevice, ss));
            PF_HIP(hipStreamWaitEvent(ss, c->sg_fit, 0));
            if (R.closure) {
                // the device-closure scan of pfmi_elbo_batch_enqueue on this segment's work list, in blocks of this stream's buffer.  Same kernels
                // on the same (fit, seed) pairs: the packed route's bits.
                for (int64_t b0 = 0; b0 < ns; b0 += R.dcb_chunk) {
                    const int64_t nb = ns - b0 < R.dcb_chunk ? ns - b0 : R.dcb_chunk;
                    PF_TRY(devcb_scan_block(c, ss, R.d_list + R.s0 + b0, R.d_lseeds + R.s0 + b0, nb, R.N, nullptr, 0, c->dcb_x[qq].as<double>(),
                                            c->dcb_lp[qq].as<double>()));
                }
            } else {
                PF_TRY(pf_launch_elbo_draws(c, R.d_list + R.s0, R.d_lseeds + R.s0, ns, 0, R.N, nullptr, 0, nullptr, 0, c->logp.as<double>(),
                                            c->logq.as<double>(), R.N, true, true));
            }
            PF_HIP(hipEventRecord(c->sg_scan[qq], ss));
            R.scan_used[qq] = true;
            R.scan_ns[qq] = ns;
            ++R.nseg;
        }
        R.trace.insert(R.trace.end(), {std::chrono::duration<double>(now - R.t_start).count() * 1e6, (double)l0, (double)l1, (double)ns, (double)q_free});
        R.s0 = t;
        R.l_next = l1;
    }
    if (!all_done) return PFMI_OK;
    // ---- drained: join the side streams, reduce
    for (int k = 0; k < K; ++k) {
        PF_CHECK(c->npts_h[(size_t)k] >= 1 && c->npts_h[(size_t)k] <= R.cap, PFMI_ERR_NUMERIC, "stream: path %d produced %d points", k, c->npts_h[(size_t)k]);
    }
    PF_HIP(hipEventRecord(c->sg_fit, c->s_fit));
    if (R.closure) {
        c->lbc.finished = true;                                     // every path has ended: no further round is issued
        PF_HIP(hipEventRecord(c->sg_opt, c->s_opt));                // behind the last round issued
    }
    PF_HIP(hipStreamWaitEvent(c->stream, c->sg_opt, 0));
    PF_HIP(hipStreamWaitEvent(c->stream, c->sg_fit, 0));
    if (R.scan_used[1]) PF_HIP(hipStreamWaitEvent(c->stream, c->sg_scan[1], 0));
    R.active = false;
    c->stream_pending = false;
    c->fitted = true;
    if (const char *tr = pf_debug_get("PFMI_STREAM_TRACE")) {         // test / tuning hook: what was launched when
        if (tr[0] == '1') {
            fprintf(stderr, "stream: %d segments, drained at %.0f us:", R.nseg, std::chrono::duration<double>(std::chrono::steady_clock::now() - R.t_start).count() * 1e6);
            for (size_t i = 0; i + 4 < R.trace.size() + 1; i += 5)
                fprintf(stderr, "  [%.0f us: %d..%d, %d fits, q%d]", R.trace[i], (int)R.trace[i + 1], (int)R.trace[i + 2], (int)R.trace[i + 3], (int)R.trace[i + 4]);
            fprintf(stderr, "\n");
        }
    }
    PF_TRY(pf_launch_elbo_reduce(c));
    c->elbo_done = true; c->elbo_pending = true; c->have_trace_lp = true;
    if (finished) *finished = 1;
    return PFMI_OK;
}

extern "C" {

int32_t pfmi_stream_enqueue(pfmi_ctx *c, int32_t K, const double *x0, int32_t J, int32_t maxiters, double g_tol, double eps, int64_t N,
                            const uint64_t *seeds) {
    PF_CTX_MUT(c);
    const int32_t rc = stream_enqueue_impl(c, K, x0, J, maxiters, g_tol, eps, N, seeds);
    if (rc != PFMI_OK && rc != PFMI_ERR_ARG && rc != PFMI_ERR_UNSUPPORTED) {
        // failed half-way (an allocation, an upload, the producer's launch): nothing of the call survives -- the side streams are drained and the
        // context forgets the half-built layout, so that later calls see "no traces" instead of a layout whose producer never ran
        stream_abandon(c);
        c->virt = false; c->P = 0; c->K = 0; c->fitted = false; c->elbo_done = false; c->pooled = false; c->opt_pending = false;
    }
    return rc;
}

// Give up an outstanding streaming call (a host that failed between pfmi_stream_enqueue and pfmi_stream_wait): what is in flight is drained, the
// half-made results are forgotten, the context is usable again.  No call outstanding: no-op.
int32_t pfmi_stream_cancel(pfmi_ctx *c) {
    PF_CTX(c);
    if (!c->sr.active && !c->stream_pending && !c->stream_drain) return PFMI_OK;
    stream_abandon(c);
    (void)hipStreamSynchronize(c->stream);
    c->fitted = false; c->elbo_done = false; c->elbo_pending = false; c->pooled = false;
    return PFMI_OK;
}

int32_t pfmi_stream_seeds(pfmi_ctx *c, const uint64_t *seeds) {
    PF_CTX(c);
    PF_CHECK(c->sr.active && !c->sr.have_seeds, PFMI_ERR_STATE, "stream_seeds: no pfmi_stream_enqueue(..., seeds = NULL) outstanding");
    PF_CHECK(seeds != nullptr, PFMI_ERR_ARG, "stream_seeds: null seeds");
    return stream_set_seeds(c, seeds);
}

int32_t pfmi_stream_pump(pfmi_ctx *c, int32_t *finished) {
    PF_CTX_MUT(c);
    const auto tp0 = std::chrono::steady_clock::now();
    const int seg0 = c->sr.l_next;
    const bool was_active = c->sr.active;
    const int32_t rc = stream_pump_pass(c, finished);
    if (was_active && (c->sr.l_next != seg0 || !c->sr.active)) {     // this pass launched a segment (or the reduction): the scheduler's real cost
        c->sr.host_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count();
        c->sr.host_n += 1;
        if (!c->sr.active && c->profile) {                            // "stream_host_schedule": host milliseconds per call spent launching segments
            KernelStat &ks = c->kstats["stream_host_schedule"];
            ks.ms += c->sr.host_s * 1e3; ks.launches += c->sr.host_n;
        }
    }
    if (rc != PFMI_OK && c->sr.active) stream_abandon(c);          // a failed pass ends the call: what is in flight is drained, the context is usable again
    return rc;
}

int32_t pfmi_stream_wait(pfmi_ctx *c, int64_t *npoints) {
    PF_CTX(c);
    PF_CHECK(c->virt && (c->sr.active || c->elbo_done), PFMI_ERR_STATE, "stream_wait: no pfmi_stream_enqueue outstanding");
    PF_CHECK(npoints != nullptr, PFMI_ERR_ARG, "stream_wait: null npoints");
    PF_CHECK(!c->sr.active || c->sr.have_seeds, PFMI_ERR_STATE, "stream_wait: pfmi_stream_enqueue was given no seeds: call pfmi_stream_seeds first");
    int32_t fin = 0;
    while (true) {
        PF_TRY(pfmi_stream_pump(c, &fin));
        if (fin) break;
        for (int i = 0; i < 64; ++i) __builtin_ia32_pause();
    }
    for (int k = 0; k < c->K; ++k) npoints[k] = c->npts_h[(size_t)k];
    return PFMI_OK;
}

}  // extern "C"
