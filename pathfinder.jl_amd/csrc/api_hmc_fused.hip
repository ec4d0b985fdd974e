// api_hmc_fused.hip -- static HMC on the BUILT-IN targets: pfmi_hmc_fused_enqueue of include/pfmi.h over hmc_fused_kernel.hip.  The run is a
// static-HMC run (HmcState::kind 0) in the buffers and layouts of pfmi_hmc_enqueue / pfmi_hmc_adapt_enqueue: the checks, the buffer list,
// the uploads and the bookkeeping are api_hmc.hip's (chain_check_chains, chain_begin, chain_refused), waiting and reading stay
// pfmi_hmc_wait, pfmi_hmc_get, pfmi_hmc_draws_dev, pfmi_hmc_get_path, pfmi_adapt_get and pfmi_chain_diagnostics.  What differs is the
// schedule: no closure rounds but launches of up to HM_FUSED_ROUNDS rounds each.  pfmi_hmc_fused_metric_enqueue is the same body with a
// staged or resident scale allowed and, for nwarmup >= 1, the metric windows of adapt.h: chains that carry a scale are launched through
// hmc_fused_metric_kernel.hip, and pfmi_adapt_metric_get serves the windows.
#include "api_internal.h"
#include "hmc_rows.h"

#include <vector>

static const ChainKind HMC_FUSED_KIND = {"hmc_fused", "HMC", "nuts", 0};
static const ChainKind HMC_FUSED_METRIC_KIND = {"hmc_fused_metric", "HMC", "nuts", 0};

// the most rounds of one launch: HM_FUSED_ROUNDS, or the test hook's value
static int64_t fused_round_cap() {
    if (const char *v = pf_debug_get("PFMI_HMC_FUSED_ROUNDS")) {
        const long long n = atoll(v);
        if (n >= 1 && n <= 2147483647ll) return n;
    }
    return HM_FUSED_ROUNDS;
}

// The one body of pfmi_hmc_fused_enqueue and pfmi_hmc_fused_metric_enqueue.  scale_ok: the entry point takes a staged scale and chains that
// carry one (the fused-metric kernel steps them); metric: CHAIN_METRIC_* of an adaptive run (W >= 1), the metric windows of chain_begin.
// `closure_route`: the entry point that serves a callback target, for the refusal's message.
static int32_t hmc_fused_enqueue(pfmi_ctx *c, const ChainKind &S, const char *closure_route, int32_t K, const int64_t *points, const double *x0,
                                 const uint64_t *seeds, const double *step_size, int32_t nleapfrog, int64_t W, int64_t T, double delta, int32_t flags,
                                 bool scale_ok, int metric) {
    HmcState &H = c->hmc;
    const TargetDev &Tg = c->target;
    const bool cont = (flags & PFMI_HMC_CONTINUE) != 0;
    const ChainCall A = {K, points, x0, seeds, step_size, T, flags, W, delta, metric};
    // (the order of pfmi_hmc_enqueue's checks: fit, target, dimension, null arguments; the sampler's parameter; flags, points, step sizes, CONTINUE)
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "%s_enqueue: call pfmi_fit_batch first", S.name);
    PF_CHECK(Tg.kind == PFMI_TARGET_GAUSS || Tg.kind == PFMI_TARGET_FUNNEL, PFMI_ERR_UNSUPPORTED,
             "%s_enqueue: needs a built-in target (PFMI_TARGET_GAUSS, PFMI_TARGET_FUNNEL); a DEVICE_CALLBACK target with a gradient closure "
             "runs through %s", S.name, closure_route);
    PF_CHECK(Tg.d == c->d, PFMI_ERR_STATE, "%s_enqueue: the target's dimension %d is not the fit's %d", S.name, Tg.d, c->d);
    PF_CHECK(K >= 1 && points && seeds && step_size && (cont || x0), PFMI_ERR_ARG, "%s_enqueue: K < 1 or a null argument", S.name);
    PF_CHECK(nleapfrog >= 1 && T >= 1, PFMI_ERR_ARG, "%s_enqueue: nleapfrog %d and ntransitions %lld must be >= 1", S.name, nleapfrog, (long long)T);
    PF_TRY(chain_check_chains(c, S, A));
    // (pfmi_hmc_fused_enqueue launches the fused kernel alone: a staged scale, or resident chains that carry one, are the other entry point's)
    PF_CHECK(scale_ok || (c->scale_staged.empty() && !(cont && H.scaled)), PFMI_ERR_UNSUPPORTED,
             "%s_enqueue: chains with a per-coordinate scale (pfmi_chain_scale_set) are not supported; pfmi_hmc_fused_metric_enqueue runs them", S.name);
    PF_CHECK(((double)W + (double)T) * (double)nleapfrog < 9.0e15, PFMI_ERR_UNSUPPORTED, "%s_enqueue: %.3g rounds in one call", S.name,
             ((double)W + (double)T) * (double)nleapfrog);
    const size_t vec = sizeof(double) * (size_t)K * c->d;
    std::vector<ChainBuf> own;
    for (DevBuf *b : {&c->hm_x, &c->hm_wg, &c->hm_wt, &c->hm_v}) own.push_back({b, vec, CHAIN_BUF});
    own.push_back({&c->hm_st, pf_hmc_chain_bytes() * (size_t)K, CHAIN_BUF, false});
    int64_t rounds = 0;
    PF_TRY(chain_begin(c, S, A, nleapfrog, "", own, nullptr, &rounds));
    H.nleap = nleapfrog; H.finished = true;
    if (!cont) PF_TRY(pf_launch_hmc_init(c, c->stream));
    // Trips: every evaluation is one, and a CONTINUE starts with the trip that only opens the next trajectory (round -1).  Cut into
    // launches of at most `cap` trips; a launch re-enters from the HmChain state and the vectors the one before left.  Chains that carry
    // a scale (chain_begin: a staged one, the resident one of a CONTINUE, ones in front of metric windows) take the fused-metric kernel.
    const int64_t cap = fused_round_cap();
    const auto launch = H.scaled ? pf_launch_hmc_fused_metric : pf_launch_hmc_fused;
    const char *stage = H.scaled ? "hmc_fused_metric" : "hmc_fused";
    for (int64_t r = cont ? -1 : 0; r < rounds;) {
        const int64_t n = rounds - r < cap ? rounds - r : cap;
        pf_kernel_begin(c);
        PF_TRY(launch(c, r, (int)n, c->stream));
        pf_kernel_end(c, stage);
        H.rounds += n - (r < 0 ? 1 : 0);
        r += n;
    }
    return PFMI_OK;
}

extern "C" {

int32_t pfmi_hmc_fused_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                               int32_t nleapfrog, int64_t nwarmup, int64_t ntransitions, double target_accept, int32_t flags) {
    PF_CTX_MUT(c);
    int32_t rc = PFMI_OK;
    if (nwarmup != 0) rc = adapt_args("hmc_fused_enqueue", nwarmup, target_accept, flags);      // (nwarmup < 0: its PFMI_ERR_ARG)
    if (rc == PFMI_OK)
        rc = hmc_fused_enqueue(c, HMC_FUSED_KIND, "pfmi_hmc_enqueue", K, points, x0, seeds, step_size, nleapfrog, nwarmup, ntransitions,
                               nwarmup ? target_accept : 0.0, flags, false, CHAIN_METRIC_NONE);
    return chain_refused(c, rc);
}

int32_t pfmi_hmc_fused_metric_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                                      int32_t nleapfrog, int64_t nwarmup, int64_t ntransitions, double target_accept, int32_t flags) {
    PF_CTX_MUT(c);
    int32_t rc = PFMI_OK;
    int metric = CHAIN_METRIC_NONE;
    if (nwarmup != 0) {                 // an adaptive run is a fresh run: its one flag selects the record of the whitened rows
        rc = adapt_args("hmc_fused_metric_enqueue", nwarmup, target_accept, flags, PFMI_ADAPT_RECORD_WHITENED);
        metric = (flags & PFMI_ADAPT_RECORD_WHITENED) ? CHAIN_METRIC_RECORD : CHAIN_METRIC_WINDOWS;
        flags = 0;
    }
    if (rc == PFMI_OK)
        rc = hmc_fused_enqueue(c, HMC_FUSED_METRIC_KIND, "pfmi_hmc_adapt_metric_enqueue (a plain run on a scale: pfmi_hmc_enqueue)", K, points, x0, seeds,
                               step_size, nleapfrog, nwarmup, ntransitions, nwarmup ? target_accept : 0.0, flags, true, metric);
    return chain_refused(c, rc);
}

}  // extern "C"
