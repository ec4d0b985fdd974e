// api_hmc.hip -- static HMC on a fitted metric for gradient closures: the entry points of include/pfmi.h over hmc_kernel.hip, and the
// diagnostics of its chains (or of any uploaded ones), pfmi_chain_diagnostics over chain_diag_kernels.hip.
#include "api_internal.h"

#include <math.h>
#include <vector>

// an HMC call that was never waited for still writes the chains and the records on the ctx stream: drain THIS ctx's stream (never the
// device) and forget the chains.  Called by whatever replaces the target, the traces or the fit the chains were made for.
void hmc_forget(pfmi_ctx *c) {
    if (c->hmc.active) (void)hipStreamSynchronize(c->stream);
    c->hmc.active = false;
    c->hmc.have = false;
    c->hmc.adapting = false;
    c->hmc.W = 0;
    c->hmc.eps_kept = false;
}

int32_t hmc_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                    int32_t nleapfrog, int64_t T, int32_t flags, int64_t W, double delta) {
    HmcState &H = c->hmc;
    const TargetDev &Tg = c->target;
    const bool cont = (flags & PFMI_HMC_CONTINUE) != 0, rec = (flags & PFMI_HMC_RECORD_PATH) != 0;
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "hmc_enqueue: call pfmi_fit_batch first");
    PF_CHECK(Tg.kind == PFMI_TARGET_DEVICE_CALLBACK && Tg.grad_fn != nullptr, PFMI_ERR_UNSUPPORTED,
             "hmc_enqueue: needs a DEVICE_CALLBACK target with a gradient closure (pfmi_set_target_gradient)");
    PF_CHECK(Tg.d == c->d, PFMI_ERR_STATE, "hmc_enqueue: the target's dimension %d is not the fit's %d", Tg.d, c->d);
    PF_CHECK(K >= 1 && points && seeds && step_size && (cont || x0), PFMI_ERR_ARG, "hmc_enqueue: K < 1 or a null argument");
    PF_CHECK(nleapfrog >= 1 && T >= 1, PFMI_ERR_ARG, "hmc_enqueue: nleapfrog %d and ntransitions %lld must be >= 1", nleapfrog, (long long)T);
    PF_CHECK((flags & ~(PFMI_HMC_CONTINUE | PFMI_HMC_RECORD_PATH)) == 0, PFMI_ERR_ARG, "hmc_enqueue: unknown flags %d", flags);
    for (int k = 0; k < K; ++k) {
        PF_CHECK(points[k] >= 0 && points[k] < c->P, PFMI_ERR_ARG, "hmc_enqueue: point %lld of chain %d outside [0, %lld)", (long long)points[k], k,
                 (long long)c->P);
        PF_CHECK(isfinite(step_size[k]) && step_size[k] > 0.0, PFMI_ERR_ARG, "hmc_enqueue: step size of chain %d is not positive and finite", k);
    }
    PF_CHECK(!cont || (H.have && H.K == K), PFMI_ERR_STATE, "hmc_enqueue: PFMI_HMC_CONTINUE without %d resident chains", K);
    PF_CHECK(!cont || H.kind == 0, PFMI_ERR_STATE, "hmc_enqueue: PFMI_HMC_CONTINUE on the chains of pfmi_nuts_enqueue");
    const int d = c->d;
    const int64_t rounds = (cont ? 0 : 1) + (W + T) * (int64_t)nleapfrog;
    const char *stage = W ? "hmc_adapt" : "hmc", *cstage = W ? "hmc_adapt_closure" : "hmc_closure";
    {   // the fits the chains ask for are successes
        std::vector<int32_t> st((size_t)c->P);
        PF_TRY(d2h(c, st.data(), c->status.p, sizeof(int32_t) * (size_t)c->P));
        for (int k = 0; k < K; ++k)
            PF_CHECK(st[(size_t)points[k]] == PFMI_FIT_OK, PFMI_ERR_NUMERIC, "hmc_enqueue: the fit of point %lld (chain %d) has status %d",
                     (long long)points[k], k, st[(size_t)points[k]]);
    }
    const size_t vec = sizeof(double) * (size_t)K * d, rows = (size_t)K * (size_t)T;
    const size_t out_bytes = sizeof(double) * (size_t)K * (d + 1);
    {   // what the call's `ensure`s below will grow (a buffer that is large enough already -- the chains of a CONTINUE, the records of an
        // equal call before -- costs nothing: hipMemGetInfo's free figure excludes it)
        size_t fr = 0, tot = 0;
        PF_HIP(hipMemGetInfo(&fr, &tot));
        double need = 0.0;
        auto grow = [&](const DevBuf &b, size_t bytes) { if (bytes > b.cap) need += (double)bytes; };
        if (!cont) {
            for (const DevBuf *b : {&c->hm_X, &c->hm_x0, &c->hm_x, &c->hm_wg, &c->hm_wt, &c->hm_v}) grow(*b, vec);
            grow(c->hm_out, out_bytes);
        }
        grow(c->hm_draws, sizeof(double) * rows * d);
        for (const DevBuf *b : {&c->hm_lp, &c->hm_acc, &c->hm_de}) grow(*b, sizeof(double) * rows);
        grow(c->hm_div, sizeof(int32_t) * rows);
        if (W) grow(c->hm_adapt, adapt_bytes(K, W));
        if (rec) {
            grow(c->hm_pX, vec * (size_t)rounds);
            grow(c->hm_pv, vec * (size_t)rounds);
            grow(c->hm_pout, out_bytes * (size_t)rounds);
        }
        PF_CHECK(need < 0.8 * (double)fr, PFMI_ERR_UNSUPPORTED, "hmc_enqueue: %.3g GB more needed for K = %d, d = %d, %lld transitions; %.3g GB free",
                 need / 1e9, K, d, (long long)T, (double)fr / 1e9);
    }
    if (!cont) {
        hmc_forget(c);
        for (DevBuf *b : {&c->hm_X, &c->hm_x0, &c->hm_x, &c->hm_wg, &c->hm_wt, &c->hm_v}) PF_TRY(b->ensure(vec));
        PF_TRY(c->hm_out.ensure(out_bytes));
        PF_TRY(c->hm_st.ensure(pf_hmc_chain_bytes() * (size_t)K));
        PF_TRY(c->hm_pts.ensure(sizeof(int32_t) * (size_t)K));
        PF_TRY(c->hm_seeds.ensure(sizeof(uint64_t) * (size_t)K));
        PF_TRY(c->hm_eps.ensure(sizeof(double) * (size_t)K));
    } else if (H.active) {
        PF_HIP(hipStreamSynchronize(c->stream));          // the records of the call before are rewritten (and may be reallocated)
        H.active = false;
    }
    PF_TRY(c->hm_draws.ensure(sizeof(double) * rows * d));
    for (DevBuf *b : {&c->hm_lp, &c->hm_acc, &c->hm_de}) PF_TRY(b->ensure(sizeof(double) * rows));
    PF_TRY(c->hm_div.ensure(sizeof(int32_t) * rows));
    if (rec) {
        PF_TRY(c->hm_pX.ensure(vec * (size_t)rounds));
        PF_TRY(c->hm_pv.ensure(vec * (size_t)rounds));
        PF_TRY(c->hm_pout.ensure(out_bytes * (size_t)rounds));
    }
    std::vector<int32_t> p32((size_t)K);
    for (int k = 0; k < K; ++k) p32[(size_t)k] = (int32_t)points[k];
    PF_TRY(pf_upload(c, c->hm_pts.p, p32.data(), sizeof(int32_t) * (size_t)K));
    PF_TRY(pf_upload(c, c->hm_seeds.p, seeds, sizeof(uint64_t) * (size_t)K));
    if (cont) PF_TRY(adapt_keep_step_sizes(c));
    PF_TRY(pf_upload(c, c->hm_eps.p, step_size, sizeof(double) * (size_t)K));
    if (!cont) PF_TRY(pf_upload(c, c->hm_x0.p, x0, vec));
    if (W) PF_TRY(adapt_reserve(c, K, W, step_size, delta));
    H.K = K; H.nleap = nleapfrog; H.record = rec; H.kind = 0; H.finished = true;
    H.t0 = cont ? H.t0 + H.T : W; H.T = T;
    H.adapting = W > 0;
    if (W) H.W = W;
    H.rounds = 0; H.columns = 0; H.path_rounds = rec ? rounds : 0;
    H.have = true; H.active = true;                       // from here on, failure paths drain (pfmi_hmc_enqueue)
    if (!cont) PF_TRY(pf_launch_hmc_init(c, c->stream));
    else {
        pf_kernel_begin(c);
        PF_TRY(pf_launch_hmc_step(c, -1, c->stream));
        pf_kernel_end(c, stage);
    }
    for (int64_t r = 0; r < rounds; ++r) {
        // the closure on all K trial points (written by the launch before), then the step kernel that consumes its answer
        pf_kernel_begin(c);
        Tg.grad_fn(c->hm_X.as<double>(), d, K, c->hm_out.as<double>(), (void *)c->stream, Tg.grad_user);
        pf_kernel_end(c, cstage);
        H.columns += K;
        pf_kernel_begin(c);
        PF_TRY(pf_launch_hmc_step(c, r, c->stream));
        pf_kernel_end(c, stage);
        ++H.rounds;
    }
    return PFMI_OK;
}

extern "C" {

int32_t pfmi_hmc_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                         int32_t nleapfrog, int64_t ntransitions, int32_t flags) {
    PF_CTX_MUT(c);
    const int32_t rc = hmc_enqueue(c, K, points, x0, seeds, step_size, nleapfrog, ntransitions, flags, 0, 0.0);
    if (rc != PFMI_OK) {                                  // an error exit drains this ctx's stream and leaves no chains behind
        (void)hipStreamSynchronize(c->stream);
        c->hmc.active = false; c->hmc.have = false;
    }
    return rc;
}

int32_t pfmi_hmc_wait(pfmi_ctx *c) {
    PF_CTX(c);
    PF_CHECK(c->hmc.have, PFMI_ERR_STATE, "hmc_wait: no pfmi_hmc_enqueue outstanding");
    PF_CHECK(c->hmc.kind == 0, PFMI_ERR_STATE, "hmc_wait: the run on this ctx is pfmi_nuts_enqueue's (pfmi_nuts_wait)");
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    std::vector<int32_t> dead;
    PF_TRY(pf_hmc_dead_flags(c, dead));
    for (int k = 0; k < c->hmc.K; ++k)
        if (dead[(size_t)k]) {
            c->hmc.have = false;
            PF_CHECK(false, PFMI_ERR_NUMERIC, "hmc: the start point of chain %d has a non-finite log density or gradient", k);
        }
    return PFMI_OK;
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
    PF_CHECK(H.have && H.record && H.kind == 0, PFMI_ERR_STATE, "hmc_get_path: the last pfmi_hmc_enqueue did not run with PFMI_HMC_RECORD_PATH");
    PF_CHECK(round0 >= 0 && nrounds >= 0 && round0 + nrounds <= H.path_rounds, PFMI_ERR_ARG, "hmc_get_path: rounds [%lld, %lld) outside [0, %lld)",
             (long long)round0, (long long)(round0 + nrounds), (long long)H.path_rounds);
    const size_t vec = (size_t)H.K * c->d, ovec = (size_t)H.K * (c->d + 1);
    if (X) PF_TRY(pf_download(c, X, c->hm_pX.as<double>() + (size_t)round0 * vec, sizeof(double) * vec * (size_t)nrounds));
    if (v) PF_TRY(pf_download(c, v, c->hm_pv.as<double>() + (size_t)round0 * vec, sizeof(double) * vec * (size_t)nrounds));
    if (closure_out) PF_TRY(pf_download(c, closure_out, c->hm_pout.as<double>() + (size_t)round0 * ovec, sizeof(double) * ovec * (size_t)nrounds));
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
