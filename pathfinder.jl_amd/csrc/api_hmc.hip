// api_hmc.hip -- static HMC on a fitted metric for gradient closures: the entry points of include/pfmi.h over hmc_kernel.hip, and the
// diagnostics of its chains (or of any uploaded ones), pfmi_chain_diagnostics over chain_diag_kernels.hip.  Also the ONE enqueue path of
// both samplers (chain_check_target, chain_check_chains, chain_begin: checks, the buffer list, uploads, bookkeeping) and their shared epilogues; api_nuts.hip and api_adapt.hip
// call them.
#include "api_internal.h"

#include <math.h>
#include <vector>

static_assert(PFMI_HMC_CONTINUE == PFMI_NUTS_CONTINUE && PFMI_HMC_RECORD_PATH == PFMI_NUTS_RECORD_PATH, "the samplers share their flags");

// an HMC call that was never waited for still writes the chains and the records on the ctx stream: drain THIS ctx's stream (never the
// device) and forget the chains.  Called by whatever replaces the target, the traces or the fit the chains were made for.
void hmc_forget(pfmi_ctx *c) {
    if (c->hmc.active) (void)hipStreamSynchronize(c->stream);
    c->hmc.active = false;
    c->hmc.have = false;
    c->hmc.adapting = false;
    c->hmc.W = 0;
    c->hmc.eps_kept = false;
    c->hmc.scaled = false;
    c->hmc.metric_run = false;
    c->hmc.rec_u = false;
    c->hmc.nwin = 0;
    c->scale_staged.clear();                              // (an enqueue has taken the staged scale before it forgets the chains: metric_plan)
}

// The one refusal epilogue of the enqueues, the pump and the wait: an error exit drains this ctx's stream and leaves no chains, no traces
// and no run behind.  (Every reader of HmcState tests `have` -- cleared here -- before any other field.)
int32_t chain_refused(pfmi_ctx *c, int32_t rc) {
    if (rc != PFMI_OK) {
        (void)hipStreamSynchronize(c->stream);
        c->hmc.finished = true;
        hmc_forget(c);
    }
    return rc;
}

// the one wait epilogue: a chain whose start point had a non-finite log density or gradient cannot leave it
int32_t chain_dead_check(pfmi_ctx *c, const char *name, const std::vector<int32_t> &dead) {
    for (int k = 0; k < c->hmc.K; ++k)
        if (dead[(size_t)k]) {
            c->hmc.have = false;
            PF_CHECK(false, PFMI_ERR_NUMERIC, "%s: the start point of chain %d has a non-finite log density or gradient", name, k);
        }
    return PFMI_OK;
}

// rounds [round0, round0 + nrounds) of the recorded path: X, v and the closure's output (queued; the caller waits)
int32_t chain_path_download(pfmi_ctx *c, int64_t round0, int64_t nrounds, double *X, double *closure_out, double *v) {
    const size_t vec = (size_t)c->hmc.K * c->d, ovec = (size_t)c->hmc.K * (c->d + 1);
    if (X) PF_TRY(pf_download(c, X, c->hm_pX.as<double>() + (size_t)round0 * vec, sizeof(double) * vec * (size_t)nrounds));
    if (v) PF_TRY(pf_download(c, v, c->hm_pv.as<double>() + (size_t)round0 * vec, sizeof(double) * vec * (size_t)nrounds));
    if (closure_out) PF_TRY(pf_download(c, closure_out, c->hm_pout.as<double>() + (size_t)round0 * ovec, sizeof(double) * ovec * (size_t)nrounds));
    return PFMI_OK;
}

int32_t chain_check_target(pfmi_ctx *c, const ChainKind &S, const ChainCall &A) {
    const TargetDev &Tg = c->target;
    const bool cont = (A.flags & PFMI_HMC_CONTINUE) != 0;
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "%s_enqueue: call pfmi_fit_batch first", S.name);
    PF_CHECK(Tg.kind == PFMI_TARGET_DEVICE_CALLBACK && Tg.grad_fn != nullptr, PFMI_ERR_UNSUPPORTED,
             "%s_enqueue: needs a DEVICE_CALLBACK target with a gradient closure (pfmi_set_target_gradient)", S.name);
    PF_CHECK(Tg.d == c->d, PFMI_ERR_STATE, "%s_enqueue: the target's dimension %d is not the fit's %d", S.name, Tg.d, c->d);
    PF_CHECK(A.K >= 1 && A.points && A.seeds && A.step_size && (cont || A.x0), PFMI_ERR_ARG, "%s_enqueue: K < 1 or a null argument", S.name);
    return PFMI_OK;
}

int32_t chain_check_chains(pfmi_ctx *c, const ChainKind &S, const ChainCall &A) {
    const HmcState &H = c->hmc;
    const int32_t K = A.K, flags = A.flags;
    const int64_t *points = A.points;
    const double *step_size = A.step_size;
    const bool cont = (flags & PFMI_HMC_CONTINUE) != 0;
    PF_CHECK((flags & ~(PFMI_HMC_CONTINUE | PFMI_HMC_RECORD_PATH)) == 0, PFMI_ERR_ARG, "%s_enqueue: unknown flags %d", S.name, flags);
    for (int k = 0; k < K; ++k) {
        PF_CHECK(points[k] >= 0 && points[k] < c->P, PFMI_ERR_ARG, "%s_enqueue: point %lld of chain %d outside [0, %lld)", S.name, (long long)points[k],
                 k, (long long)c->P);
        PF_CHECK(isfinite(step_size[k]) && step_size[k] > 0.0, PFMI_ERR_ARG, "%s_enqueue: step size of chain %d is not positive and finite", S.name, k);
    }
    PF_CHECK(!cont || (H.have && H.K == K), PFMI_ERR_STATE, "%s_enqueue: PFMI_%s_CONTINUE without %d resident chains", S.name, S.NAME, K);
    PF_CHECK(!cont || H.kind == S.kind, PFMI_ERR_STATE, "%s_enqueue: PFMI_%s_CONTINUE on the chains of pfmi_%s_enqueue", S.name, S.NAME,
             H.kind == 0 ? "hmc" : H.kind == 1 ? "nuts" : "chees");
    PF_CHECK(c->scale_staged.empty() || c->scale_staged_K == K, PFMI_ERR_ARG, "%s_enqueue: the scale of pfmi_chain_scale_set is for %d chains, not %d",
             S.name, c->scale_staged_K, K);
    return PFMI_OK;
}

int32_t chain_begin(pfmi_ctx *c, const ChainKind &S, const ChainCall &A, int64_t per_transition, const char *need_detail,
                    std::vector<ChainBuf> bufs, int32_t (*drain)(pfmi_ctx *), int64_t *rounds_out) {
    HmcState &H = c->hmc;
    const int32_t K = A.K;
    const int64_t *points = A.points, T = A.T, W = A.W;
    const double *step_size = A.step_size;
    const bool cont = (A.flags & PFMI_HMC_CONTINUE) != 0, rec = (A.flags & PFMI_HMC_RECORD_PATH) != 0;
    const int d = c->d;
    const int64_t rounds = (cont ? 0 : 1) + (W + T) * per_transition;
    {   // the fits the chains ask for are successes
        std::vector<int32_t> st((size_t)c->P);
        PF_TRY(d2h(c, st.data(), c->status.p, sizeof(int32_t) * (size_t)c->P));
        for (int k = 0; k < K; ++k)
            PF_CHECK(st[(size_t)points[k]] == PFMI_FIT_OK, PFMI_ERR_NUMERIC, "%s_enqueue: the fit of point %lld (chain %d) has status %d", S.name,
                     (long long)points[k], k, st[(size_t)points[k]]);
    }
    // The buffers of the call, each size stated ONCE: the samplers' common ones here, `bufs` holds the caller's own.  The estimate and the
    // `ensure`s both walk this list.  (est = false: the small per-chain arrays the estimate has always left out.)
    const size_t vec = sizeof(double) * (size_t)K * d, rows = (size_t)K * (size_t)T, out_bytes = sizeof(double) * (size_t)K * (d + 1);
    for (DevBuf *b : {&c->hm_X, &c->hm_x0}) bufs.push_back({b, vec, CHAIN_BUF});
    bufs.push_back({&c->hm_out, out_bytes, CHAIN_BUF});
    bufs.push_back({&c->hm_pts, sizeof(int32_t) * (size_t)K, CHAIN_BUF, false});
    bufs.push_back({&c->hm_seeds, sizeof(uint64_t) * (size_t)K, CHAIN_BUF, false});
    bufs.push_back({&c->hm_eps, sizeof(double) * (size_t)K, CHAIN_BUF, false});
    bufs.push_back({&c->hm_draws, sizeof(double) * rows * d, CALL_BUF});
    for (DevBuf *b : {&c->hm_lp, &c->hm_acc, &c->hm_de}) bufs.push_back({b, sizeof(double) * rows, CALL_BUF});
    bufs.push_back({&c->hm_div, sizeof(int32_t) * rows, CALL_BUF});
    if (W) bufs.push_back({&c->hm_adapt, adapt_bytes(K, W), CALL_BUF});
    MetricPlan MP;
    PF_TRY(metric_plan(c, A, bufs, MP));
    for (DevBuf *b : {&c->hm_pX, &c->hm_pv}) bufs.push_back({b, vec, PATH_BUF});
    bufs.push_back({&c->hm_pout, out_bytes, PATH_BUF});
    // what this call grows: a CONTINUE keeps the chains' buffers, only RECORD_PATH has path rows (one per round, of the cap for NUTS)
    std::vector<ChainBuf> grown;
    for (ChainBuf b : bufs) {
        if ((b.scope == CHAIN_BUF && cont) || (b.scope == PATH_BUF && !rec)) continue;
        if (b.scope == PATH_BUF) b.bytes *= (size_t)rounds;
        grown.push_back(b);
    }
    {   // against what is free (a buffer that is large enough already -- the records of an equal call before -- costs nothing:
        // hipMemGetInfo's free figure excludes it)
        size_t fr = 0, tot = 0;
        PF_HIP(hipMemGetInfo(&fr, &tot));
        double need = 0.0;
        for (const ChainBuf &b : grown) if (b.est && b.bytes > b.buf->cap) need += (double)b.bytes;
        PF_CHECK(need < 0.8 * (double)fr, PFMI_ERR_UNSUPPORTED, "%s_enqueue: %.3g GB more needed for K = %d, d = %d, %lld transitions%s; %.3g GB free",
                 S.name, need / 1e9, K, d, (long long)T, need_detail, (double)fr / 1e9);
    }
    if (!cont) hmc_forget(c);
    else {
        if (drain) PF_TRY(drain(c));                      // NUTS: the rounds of the call before that were not issued yet
        if (drain || H.active) PF_HIP(hipStreamSynchronize(c->stream));     // its records are rewritten (and may be reallocated)
        H.active = false;
    }
    for (const ChainBuf &b : grown) PF_TRY(b.buf->ensure(b.bytes));
    std::vector<int32_t> p32((size_t)K);
    for (int k = 0; k < K; ++k) p32[(size_t)k] = (int32_t)points[k];
    PF_TRY(pf_upload(c, c->hm_pts.p, p32.data(), sizeof(int32_t) * (size_t)K));
    PF_TRY(pf_upload(c, c->hm_seeds.p, A.seeds, sizeof(uint64_t) * (size_t)K));
    if (cont) PF_TRY(adapt_keep_step_sizes(c));
    PF_TRY(pf_upload(c, c->hm_eps.p, step_size, sizeof(double) * (size_t)K));
    if (!cont) PF_TRY(pf_upload(c, c->hm_x0.p, A.x0, vec));
    if (W) PF_TRY(adapt_reset(c, K, W, step_size, A.delta, A.metric && MP.nwin == 0 ? PF_ADAPT_NO_METRIC_WINDOW : 0));
    H.K = K; H.record = rec; H.kind = S.kind;
    PF_TRY(metric_begin(c, A, MP));
    H.t0 = cont ? H.t0 + H.T : W; H.T = T;
    H.adapting = W > 0;
    if (W) H.W = W;
    H.rounds = 0; H.columns = 0; H.path_rounds = rec ? rounds : 0;
    H.have = true; H.active = true;                       // from here on, failure paths drain (chain_refused)
    *rounds_out = rounds;
    return PFMI_OK;
}

// ---- the one pump of the samplers whose round count is decided on the device (NUTS, ChEES); scheduled as the closure L-BFGS's rounds are
// (lbc_issue_rounds, api_inputs.hip)
#define PF_CHAIN_WINDOW 4               // rounds in flight at most

// Issues the rounds a run may have in flight: the gradient closure on all K trial points, then the sampler's launches that consume its answer.
// At most PF_CHAIN_WINDOW rounds ahead of the last one whose progress word the host has read, never more than the hard cap.  Sets H.finished.
// A pump without a closure stage (closure_stage null: fused NUTS on a built-in target, api_nuts_fused.hip) issues its launches alone.
int32_t chain_issue_rounds(pfmi_ctx *c, const ChainPump &P) {
    HmcState &H = c->hmc;
    const TargetDev &Tg = c->target;
    const int64_t w = __atomic_load_n(c->nt_status, __ATOMIC_ACQUIRE);
    const int64_t round = w >> 32, active = w & 0xffffffffll;
    if (round > H.seen) H.seen = round;
    if (round == H.seen) H.word_low = active;
    if (round == H.seen && active == 0) H.finished = true;
    while (!H.finished && H.issued < H.max_rounds && H.issued - H.seen < PF_CHAIN_WINDOW) {
        if (P.closure_stage) {
            pf_kernel_begin(c);
            Tg.grad_fn(c->hm_X.as<double>(), c->d, H.K, c->hm_out.as<double>(), (void *)c->stream, Tg.grad_user);
            pf_kernel_end(c, P.closure_stage(H));
            H.columns += H.K;
        }
        const int64_t prow = H.issued++;
        PF_TRY(P.round(c, H.issued, prow));
    }
    if (!H.finished && H.issued >= H.max_rounds && H.seen >= H.issued) H.finished = true;      // the hard cap: a stuck flag cannot loop forever
    return PFMI_OK;
}

int32_t chain_pump_pass(pfmi_ctx *c, const ChainPump &P, int32_t *finished) {
    HmcState &H = c->hmc;
    PF_TRY(chain_issue_rounds(c, P));
    if (!H.finished) {
        const hipError_t e = hipStreamQuery(c->stream);
        PF_CHECK(e == hipSuccess || e == hipErrorNotReady, PFMI_ERR_HIP, "%s_pump: %s", P.name, hipGetErrorString(e));
    }
    *finished = H.finished ? 1 : 0;
    return PFMI_OK;
}

int32_t chain_drain(pfmi_ctx *c, const ChainPump &P) {   // pump to the end (every pass is bounded by the window, the run by the cap)
    int32_t fin = c->hmc.finished ? 1 : 0;
    while (!fin) {
        PF_TRY(chain_pump_pass(c, P, &fin));
        if (!fin) for (int i = 0; i < 64; ++i) __builtin_ia32_pause();
    }
    return PFMI_OK;
}

static const ChainKind HMC_KIND = {"hmc", "HMC", "nuts", 0};

int32_t hmc_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                    int32_t nleapfrog, int64_t T, int32_t flags, int64_t W, double delta, int metric) {
    HmcState &H = c->hmc;
    const TargetDev &Tg = c->target;
    const int d = c->d;
    const size_t vec = sizeof(double) * (size_t)K * d;
    const ChainCall A = {K, points, x0, seeds, step_size, T, flags, W, delta, metric};
    PF_TRY(chain_check_target(c, HMC_KIND, A));
    PF_CHECK(nleapfrog >= 1 && T >= 1, PFMI_ERR_ARG, "hmc_enqueue: nleapfrog %d and ntransitions %lld must be >= 1", nleapfrog, (long long)T);
    PF_TRY(chain_check_chains(c, HMC_KIND, A));
    std::vector<ChainBuf> own;
    for (DevBuf *b : {&c->hm_x, &c->hm_wg, &c->hm_wt, &c->hm_v}) own.push_back({b, vec, CHAIN_BUF});
    own.push_back({&c->hm_st, pf_hmc_chain_bytes() * (size_t)K, CHAIN_BUF, false});
    int64_t rounds = 0;
    PF_TRY(chain_begin(c, HMC_KIND, A, nleapfrog, "", own, nullptr, &rounds));
    const bool cont = (flags & PFMI_HMC_CONTINUE) != 0;
    const bool scaled = H.scaled;                        // chains that carry a scale: the metric kernel, plain run or adaptive
    const char *stage = scaled ? "hmc_metric" : W ? "hmc_adapt" : "hmc";
    const char *cstage = scaled ? "hmc_metric_closure" : W ? "hmc_adapt_closure" : "hmc_closure";
    const auto step = scaled ? pf_launch_hmc_metric_step : pf_launch_hmc_step;
    H.nleap = nleapfrog; H.finished = true;
    if (!cont) PF_TRY(pf_launch_hmc_init(c, c->stream));
    else {
        pf_kernel_begin(c);
        PF_TRY(step(c, -1, c->stream));
        pf_kernel_end(c, stage);
    }
    for (int64_t r = 0; r < rounds; ++r) {
        // the closure on all K trial points (written by the launch before), then the step kernel that consumes its answer
        pf_kernel_begin(c);
        Tg.grad_fn(c->hm_X.as<double>(), d, K, c->hm_out.as<double>(), (void *)c->stream, Tg.grad_user);
        pf_kernel_end(c, cstage);
        H.columns += K;
        pf_kernel_begin(c);
        PF_TRY(step(c, r, c->stream));
        pf_kernel_end(c, stage);
        ++H.rounds;
    }
    return PFMI_OK;
}

extern "C" {

int32_t pfmi_hmc_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                         int32_t nleapfrog, int64_t ntransitions, int32_t flags) {
    PF_CTX_MUT(c);
    return chain_refused(c, hmc_enqueue(c, K, points, x0, seeds, step_size, nleapfrog, ntransitions, flags, 0, 0.0));
}

int32_t pfmi_hmc_wait(pfmi_ctx *c) {
    PF_CTX(c);
    PF_CHECK(c->hmc.have, PFMI_ERR_STATE, "hmc_wait: no pfmi_hmc_enqueue outstanding");
    PF_CHECK(c->hmc.kind == 0, PFMI_ERR_STATE, "hmc_wait: the run on this ctx is pfmi_%s_enqueue's (pfmi_%s_wait)", c->hmc.kind == 1 ? "nuts" : "chees",
             c->hmc.kind == 1 ? "nuts" : "chees");
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    std::vector<int32_t> dead;
    PF_TRY(pf_hmc_dead_flags(c, dead));
    return chain_dead_check(c, "hmc", dead);
}

int32_t pfmi_hmc_get(pfmi_ctx *c, double *draws, double *logp, double *accept_prob, double *energy_error, int32_t *divergent) {
    PF_CTX(c);
    PF_CHECK(c->hmc.have, PFMI_ERR_STATE, "hmc_get: no HMC run on this ctx");
    PF_CHECK(c->hmc.finished, PFMI_ERR_STATE, "hmc_get: the NUTS run has rounds to go (pfmi_nuts_wait)");
    const size_t rows = (size_t)c->hmc.K * (size_t)c->hmc.T;
    if (logp) PF_TRY(pf_download(c, logp, c->hm_lp.p, sizeof(double) * rows));
    if (accept_prob) PF_TRY(pf_download(c, accept_prob, c->hm_acc.p, sizeof(double) * rows));
    if (energy_error) PF_TRY(pf_download(c, energy_error, c->hm_de.p, sizeof(double) * rows));
    if (divergent) PF_TRY(pf_download(c, divergent, c->hm_div.p, sizeof(int32_t) * rows));
    if (draws) PF_TRY(pf_download(c, draws, c->hm_draws.p, sizeof(double) * rows * (size_t)c->d));
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    return PFMI_OK;
}

int32_t pfmi_hmc_draws_dev(pfmi_ctx *c, void **dev_ptr, int64_t *count) {
    PF_CTX(c);
    PF_CHECK(c->hmc.have, PFMI_ERR_STATE, "hmc_draws_dev: no HMC run on this ctx");
    PF_CHECK(dev_ptr != nullptr, PFMI_ERR_ARG, "hmc_draws_dev: null dev_ptr");
    *dev_ptr = c->hm_draws.p;
    if (count) *count = (int64_t)c->hmc.K * c->hmc.T;
    return PFMI_OK;
}

int32_t pfmi_hmc_get_path(pfmi_ctx *c, int64_t round0, int64_t nrounds, double *X, double *closure_out, double *v) {
    PF_CTX(c);
    const HmcState &H = c->hmc;
    PF_CHECK(H.have && H.record && H.kind != 1, PFMI_ERR_STATE, "hmc_get_path: the last pfmi_hmc_enqueue did not run with PFMI_HMC_RECORD_PATH");
    PF_CHECK(H.finished, PFMI_ERR_STATE, "hmc_get_path: the ChEES run has rounds to go (pfmi_chees_wait)");
    PF_CHECK(round0 >= 0 && nrounds >= 0 && round0 + nrounds <= H.path_rounds, PFMI_ERR_ARG, "hmc_get_path: rounds [%lld, %lld) outside [0, %lld)",
             (long long)round0, (long long)(round0 + nrounds), (long long)H.path_rounds);
    PF_TRY(chain_path_download(c, round0, nrounds, X, closure_out, v));
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    return PFMI_OK;
}

int32_t pfmi_hmc_stats(pfmi_ctx *c, int64_t *rounds, int64_t *closure_columns) {
    PF_CHECK(c != nullptr, PFMI_ERR_ARG, "null pfmi_ctx");
    if (rounds) *rounds = c->hmc.rounds;
    if (closure_columns) *closure_columns = c->hmc.columns;
    return PFMI_OK;
}

int32_t pfmi_chain_diagnostics(pfmi_ctx *c, int32_t source, const double *draws, int32_t d, int64_t T, int32_t K, int32_t flags,
                               double *mean, double *sd, double *mcse_mean, double *ess_mean, double *ess_bulk, double *ess_tail,
                               double *rhat) {
    PF_CTX(c);
    const bool resident = source == PFMI_CHAIN_SRC_HMC, with_lp = (flags & PFMI_CHAIN_WITH_LP) != 0;
    PF_CHECK(resident || source == PFMI_CHAIN_SRC_HOST, PFMI_ERR_ARG, "chain_diagnostics: unknown source %d", source);
    PF_CHECK((flags & ~PFMI_CHAIN_WITH_LP) == 0, PFMI_ERR_ARG, "chain_diagnostics: unknown flags %d", flags);
    PF_CHECK(resident || !with_lp, PFMI_ERR_ARG, "chain_diagnostics: PFMI_CHAIN_WITH_LP needs PFMI_CHAIN_SRC_HMC");
    if (resident) {
        PF_CHECK(draws == nullptr, PFMI_ERR_ARG, "chain_diagnostics: PFMI_CHAIN_SRC_HMC takes no host draws");
        PF_CHECK(c->hmc.have, PFMI_ERR_STATE, "chain_diagnostics: no HMC run on this ctx");
        PF_CHECK(c->hmc.finished, PFMI_ERR_STATE, "chain_diagnostics: the NUTS run has rounds to go (pfmi_nuts_wait)");
        PF_CHECK((d == 0 && T == 0 && K == 0) || (d == c->d && T == c->hmc.T && K == c->hmc.K), PFMI_ERR_ARG,
                 "chain_diagnostics: d = %d, T = %lld, K = %d are not the resident run's %d, %lld, %d (or all 0)", d, (long long)T, K, c->d,
                 (long long)c->hmc.T, c->hmc.K);
        d = c->d; T = c->hmc.T; K = c->hmc.K;
    } else {
        PF_CHECK(draws != nullptr, PFMI_ERR_ARG, "chain_diagnostics: null draws");
    }
    PF_CHECK(T >= 8 && K >= 1 && d >= 1, PFMI_ERR_ARG, "chain_diagnostics: needs T >= 8, K >= 1, d >= 1 (T = %lld, K = %d, d = %d)", (long long)T,
             K, d);
    PF_CHECK((double)K * (double)T < 2147483648.0, PFMI_ERR_UNSUPPORTED, "chain_diagnostics: K T = %.3g draws per coordinate is beyond 2^31",
             (double)K * (double)T);
    const size_t ws_bytes = pf_chain_diag_bytes(d, T, K, with_lp), in_bytes = resident ? 0 : sizeof(double) * (size_t)K * (size_t)T * (size_t)d;
    {   // what the `ensure`s below will grow, against what is free (as pfmi_hmc_enqueue does)
        size_t fr = 0, tot = 0;
        PF_HIP(hipMemGetInfo(&fr, &tot));
        double need = 0.0;
        if (ws_bytes > c->cd_ws.cap) need += (double)ws_bytes;
        if (in_bytes > c->cd_in.cap) need += (double)in_bytes;
        PF_CHECK(need < 0.8 * (double)fr, PFMI_ERR_UNSUPPORTED,
                 "chain_diagnostics: %.0f bytes more needed for d = %d, T = %lld, K = %d (workspace %zu, records %zu); %.0f bytes free", need, d,
                 (long long)T, K, ws_bytes, in_bytes, (double)fr);
    }
    PF_TRY(c->cd_ws.ensure(ws_bytes));
    const double *rec = c->hm_draws.as<double>(), *lp = with_lp ? c->hm_lp.as<double>() : nullptr;
    if (!resident) {
        PF_TRY(c->cd_in.ensure(in_bytes));
        PF_TRY(pf_upload(c, c->cd_in.p, draws, in_bytes));
        rec = c->cd_in.as<double>();
    }
    const double *out = nullptr;
    PF_TRY(pf_launch_chain_diag(c, rec, lp, d, T, K, &out));
    const size_t V = (size_t)d + (with_lp ? 1 : 0);
    double *dst[7] = {mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, rhat};
    for (int q = 0; q < 7; ++q)
        if (dst[q]) PF_TRY(pf_download(c, dst[q], out + (size_t)q * V, sizeof(double) * V));
    PF_TRY(pf_stream_sync(c));
    if (resident) c->hmc.active = false;                  // the stream is drained: the run's rounds are done
    return PFMI_OK;
}

}  // extern "C"
