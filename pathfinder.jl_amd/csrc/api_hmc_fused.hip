// api_hmc_fused.hip -- static HMC on the BUILT-IN targets: pfmi_hmc_fused_enqueue of include/pfmi.h over hmc_fused_kernel.hip.  The run is a
// static-HMC run (HmcState::kind 0) in the buffers and layouts of pfmi_hmc_enqueue / pfmi_hmc_adapt_enqueue: the checks, the buffer list,
// the uploads and the bookkeeping are api_hmc.hip's (chain_check_chains, chain_begin, chain_refused), waiting and reading stay
// pfmi_hmc_wait, pfmi_hmc_get, pfmi_hmc_draws_dev, pfmi_hmc_get_path, pfmi_adapt_get and pfmi_chain_diagnostics.  What differs is the
// schedule: no closure rounds but launches of up to HM_FUSED_ROUNDS rounds each.
#include "api_internal.h"
#include "hmc_rows.h"

#include <vector>

static const ChainKind HMC_FUSED_KIND = {"hmc_fused", "HMC", "nuts", 0};

// the most rounds of one launch: HM_FUSED_ROUNDS, or the test hook's value
static int64_t fused_round_cap() {
    if (const char *v = pf_debug_get("PFMI_HMC_FUSED_ROUNDS")) {
        const long long n = atoll(v);
        if (n >= 1 && n <= 2147483647ll) return n;
    }
    return HM_FUSED_ROUNDS;
}

static int32_t hmc_fused_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                                 int32_t nleapfrog, int64_t W, int64_t T, double delta, int32_t flags) {
    HmcState &H = c->hmc;
    const TargetDev &Tg = c->target;
    const bool cont = (flags & PFMI_HMC_CONTINUE) != 0;
    const ChainCall A = {K, points, x0, seeds, step_size, T, flags, W, delta};
    // (the order of pfmi_hmc_enqueue's checks: fit, target, dimension, null arguments; the sampler's parameter; flags, points, step sizes, CONTINUE)
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "hmc_fused_enqueue: call pfmi_fit_batch first");
    PF_CHECK(Tg.kind == PFMI_TARGET_GAUSS || Tg.kind == PFMI_TARGET_FUNNEL, PFMI_ERR_UNSUPPORTED,
             "hmc_fused_enqueue: needs a built-in target (PFMI_TARGET_GAUSS, PFMI_TARGET_FUNNEL); a DEVICE_CALLBACK target with a gradient closure "
             "runs through pfmi_hmc_enqueue");
    PF_CHECK(Tg.d == c->d, PFMI_ERR_STATE, "hmc_fused_enqueue: the target's dimension %d is not the fit's %d", Tg.d, c->d);
    PF_CHECK(K >= 1 && points && seeds && step_size && (cont || x0), PFMI_ERR_ARG, "hmc_fused_enqueue: K < 1 or a null argument");
    PF_CHECK(nleapfrog >= 1 && T >= 1, PFMI_ERR_ARG, "hmc_fused_enqueue: nleapfrog %d and ntransitions %lld must be >= 1", nleapfrog, (long long)T);
    PF_TRY(chain_check_chains(c, HMC_FUSED_KIND, A));
    // (the metric kernels are not fused: a staged scale, or resident chains that carry one, have no kernel here)
    PF_CHECK(c->scale_staged.empty() && !(cont && H.scaled), PFMI_ERR_UNSUPPORTED,
             "hmc_fused_enqueue: chains with a per-coordinate scale (pfmi_chain_scale_set) are not supported");
    PF_CHECK(((double)W + (double)T) * (double)nleapfrog < 9.0e15, PFMI_ERR_UNSUPPORTED, "hmc_fused_enqueue: %.3g rounds in one call",
             ((double)W + (double)T) * (double)nleapfrog);
    const size_t vec = sizeof(double) * (size_t)K * c->d;
    std::vector<ChainBuf> own;
    for (DevBuf *b : {&c->hm_x, &c->hm_wg, &c->hm_wt, &c->hm_v}) own.push_back({b, vec, CHAIN_BUF});
    own.push_back({&c->hm_st, pf_hmc_chain_bytes() * (size_t)K, CHAIN_BUF, false});
    int64_t rounds = 0;
    PF_TRY(chain_begin(c, HMC_FUSED_KIND, A, nleapfrog, "", own, nullptr, &rounds));
    H.nleap = nleapfrog; H.finished = true;
    if (!cont) PF_TRY(pf_launch_hmc_init(c, c->stream));
    // Trips: every evaluation is one, and a CONTINUE starts with the trip that only opens the next trajectory (round -1).  Cut into
    // launches of at most `cap` trips; a launch re-enters from the HmChain state and the vectors the one before left.
    const int64_t cap = fused_round_cap();
    for (int64_t r = cont ? -1 : 0; r < rounds;) {
        const int64_t n = rounds - r < cap ? rounds - r : cap;
        pf_kernel_begin(c);
        PF_TRY(pf_launch_hmc_fused(c, r, (int)n, c->stream));
        pf_kernel_end(c, "hmc_fused");
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
    if (rc == PFMI_OK) rc = hmc_fused_enqueue(c, K, points, x0, seeds, step_size, nleapfrog, nwarmup, ntransitions, nwarmup ? target_accept : 0.0, flags);
    return chain_refused(c, rc);
}

}  // extern "C"
