// api_chees.hip -- ChEES-HMC on a fitted metric for gradient closures: the entry points of include/pfmi.h over chees_kernel.hip.  The chains,
// the closure buffers, the record buffers and the warm-up traces are static HMC's (api_hmc.hip, api_adapt.hip: pfmi_hmc_get, pfmi_adapt_get,
// pfmi_hmc_get_path and pfmi_chain_diagnostics serve a ChEES run unchanged), the enqueue path is chain_begin and the rounds are pumped by
// the samplers' one pump (chain_issue_rounds, api_hmc.hip); what is ChEES's own is here: the shared state, its traces and the host builds
// of the rule (adapt.h).
#include "api_internal.h"
#include "hmc_rows.h"

#include <math.h>
#include <vector>

static const char *chees_closure_stage(const HmcState &) { return "chees_closure"; }

// what follows the closure in a round: the step launch and -- while warm-up transitions are still to come, as far as the last progress word
// read says -- the cross-chain update's launches and the one that opens the next trajectory, which all do nothing unless the step launch
// ended a warm-up transition
static int32_t chees_round(pfmi_ctx *c, int64_t round, int64_t prow) {
    const HmcState &H = c->hmc;
    pf_kernel_begin(c);
    PF_TRY(pf_launch_chees_step(c, round, prow, false, c->stream));
    pf_kernel_end(c, "chees");
    if (H.word_low & 2) {
        pf_kernel_begin(c);
        PF_TRY(pf_launch_chees_update(c, c->stream));
        PF_TRY(pf_launch_chees_step(c, round, -1, true, c->stream));
        pf_kernel_end(c, "chees_update");
    }
    return PFMI_OK;
}
static const ChainPump CHEES_PUMP = {"chees", chees_closure_stage, chees_round};
static int32_t chees_drain(pfmi_ctx *c) { return chain_drain(c, CHEES_PUMP); }

static const ChainKind CHEES_KIND = {"chees", "HMC", "hmc", 2};

static int32_t chees_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, double eps0, double tau0,
                             int32_t Lmax, int64_t W, int64_t T, double delta, int32_t flags) {
    HmcState &H = c->hmc;
    const bool cont = (flags & PFMI_HMC_CONTINUE) != 0, rec_upd = (flags & PFMI_CHEES_RECORD_UPDATE) != 0;
    const std::vector<double> epsv((size_t)(K >= 1 ? K : 1), eps0);
    const ChainCall A = {K, points, x0, seeds, epsv.data(), T, flags & ~PFMI_CHEES_RECORD_UPDATE, W, delta};
    PF_TRY(chain_check_target(c, CHEES_KIND, A));
    PF_CHECK(Lmax >= 1 && Lmax <= PF_CHEES_MAX_LEAPFROG && T >= 1, PFMI_ERR_ARG, "chees_enqueue: max_leapfrog %d outside 1 .. %d or ntransitions %lld < 1",
             Lmax, PF_CHEES_MAX_LEAPFROG, (long long)T);
    PF_CHECK(W >= 0 && delta > 0.0 && delta < 1.0, PFMI_ERR_ARG, "chees_enqueue: nwarmup %lld < 0 or target_accept %g outside (0, 1)", (long long)W, delta);
    PF_CHECK(tau0 >= 0.0 && isfinite(tau0), PFMI_ERR_ARG, "chees_enqueue: traj_length0 is negative or not finite");
    PF_CHECK(!(cont && W > 0), PFMI_ERR_ARG, "chees_enqueue: PFMI_HMC_CONTINUE with nwarmup %lld (a warm-up belongs to a fresh run)", (long long)W);
    PF_TRY(chain_check_chains(c, CHEES_KIND, A));
    // (a CONTINUE is on ChEES chains, which never carry a scale: a staged one is the only way to ask for it)
    PF_CHECK(c->scale_staged.empty(), PFMI_ERR_UNSUPPORTED, "chees_enqueue: chains with a per-coordinate scale are not supported");
    PF_CHECK((double)W + (double)T < 2147483648.0, PFMI_ERR_UNSUPPORTED, "chees_enqueue: %.0f transitions in one call", (double)W + (double)T);
    const int d = c->d;
    const int64_t nrec = W > 0 ? (rec_upd ? W : 1) : 0;
    const CheesLayout Y(K, d, W, T, nrec);
    const size_t vec = sizeof(double) * (size_t)K * d;
    std::vector<ChainBuf> own;
    for (DevBuf *b : {&c->hm_x, &c->hm_wg, &c->hm_wt, &c->hm_v}) own.push_back({b, vec, CHAIN_BUF});
    own.push_back({&c->hm_st, pf_hmc_chain_bytes() * (size_t)K, CHAIN_BUF, false});
    own.push_back({&c->hm_chees, Y.bytes, CALL_BUF});
    char detail[40];
    snprintf(detail, sizeof detail, ", max_leapfrog %d", Lmax);
    int64_t rounds = 0;
    PF_TRY(chain_begin(c, CHEES_KIND, A, Lmax, detail, own, chees_drain, &rounds));
    if (!c->nt_status) PF_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->nt_status), sizeof(int64_t), hipHostMallocCoherent | hipHostMallocMapped));
    H.nleap = 0;
    H.ch_W = W; H.ch_T = T; H.ch_nrec = nrec; H.ch_Lmax = Lmax; H.ch_rec = rec_upd && W > 0;
    H.issued = 0; H.seen = 0; H.max_rounds = rounds; H.finished = false;
    H.word_low = W > 0 ? 3 : 1;
    __atomic_store_n(c->nt_status, H.word_low, __ATOMIC_RELEASE);                // round 0: running (and warming up)
    // the shared state, the empty traces and L_t
    PfChees C = {};
    C.eps = eps0; C.tau = tau0 > 0.0 ? tau0 : eps0; C.s = 0.0; C.b = 1.0; C.ltb = 0.0;
    C.da = pf_adapt_init(eps0, delta);
    C.t_upd = -1; C.fin_round = 0; C.Lmax = Lmax;
    PF_HIP(hipMemsetAsync(c->hm_chees.p, 0, Y.bytes, c->stream));
    PF_TRY(pf_upload(c, c->hm_chees.p, &C, sizeof C));
    if (!cont) PF_TRY(pf_launch_hmc_init(c, c->stream));
    else {
        pf_kernel_begin(c);
        PF_TRY(pf_launch_chees_step(c, 0, -1, true, c->stream));
        pf_kernel_end(c, "chees");
    }
    return chain_issue_rounds(c, CHEES_PUMP);
}

// the finished run's shared state
static int32_t chees_state(pfmi_ctx *c, PfChees *C) { return d2h(c, C, c->hm_chees.p, sizeof *C); }

extern "C" {

int32_t pfmi_chees_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, double step_size0,
                           double traj_length0, int32_t max_leapfrog, int64_t nwarmup, int64_t ntransitions, double target_accept, int32_t flags) {
    PF_CTX_MUT(c);
    return chain_refused(c, chees_enqueue(c, K, points, x0, seeds, step_size0, traj_length0, max_leapfrog, nwarmup, ntransitions, target_accept, flags));
}

int32_t pfmi_chees_pump(pfmi_ctx *c, int32_t *finished) {
    PF_CHECK(c != nullptr && finished != nullptr, PFMI_ERR_ARG, "chees_pump: null argument");
    PF_CHECK(c->hmc.have && c->hmc.kind == 2, PFMI_ERR_STATE, "chees_pump: no pfmi_chees_enqueue outstanding");
    PF_HIP(hipSetDevice(c->device));
    return chain_refused(c, chain_pump_pass(c, CHEES_PUMP, finished));          // a failed pass ends the run: what is in flight is drained
}

int32_t pfmi_chees_wait(pfmi_ctx *c) {
    PF_CTX(c);
    HmcState &H = c->hmc;
    PF_CHECK(H.have && H.kind == 2, PFMI_ERR_STATE, "chees_wait: no pfmi_chees_enqueue outstanding");
    PF_TRY(chain_refused(c, chees_drain(c)));
    PF_TRY(pf_stream_sync(c));
    H.active = false;
    PfChees C;
    PF_TRY(chees_state(c, &C));
    H.rounds = C.fin_round;
    std::vector<int32_t> dead;
    PF_TRY(pf_hmc_dead_flags(c, dead));
    return chain_dead_check(c, "chees", dead);
}

int32_t pfmi_chees_get(pfmi_ctx *c, double *step_size, double *traj_length, double *tau_trace, double *grad_trace, double *hmean_trace,
                       int32_t *n_leapfrog, int32_t *status) {
    PF_CTX(c);
    const HmcState &H = c->hmc;
    PF_CHECK(H.have && H.kind == 2, PFMI_ERR_STATE, "chees_get: no ChEES run on this ctx");
    PF_CHECK(H.finished, PFMI_ERR_STATE, "chees_get: the run has rounds to go (pfmi_chees_wait)");
    const CheesLayout Y(H.K, c->d, H.ch_W, H.ch_T, H.ch_nrec);
    const double *b = c->hm_chees.as<double>();
    const size_t W = (size_t)H.ch_W;
    PfChees C;
    if (tau_trace) PF_TRY(pf_download(c, tau_trace, b + Y.trace, sizeof(double) * W));
    if (grad_trace) PF_TRY(pf_download(c, grad_trace, b + Y.trace + W, sizeof(double) * W));
    if (hmean_trace) PF_TRY(pf_download(c, hmean_trace, b + Y.trace + 2 * W, sizeof(double) * W));
    if (n_leapfrog) PF_TRY(pf_download(c, n_leapfrog, b + Y.nl, sizeof(int32_t) * (size_t)(H.ch_W + H.ch_T)));
    PF_TRY(chees_state(c, &C));
    c->hmc.active = false;
    if (step_size) *step_size = C.eps;
    if (traj_length) *traj_length = C.tau;
    if (status) *status = C.status | C.da.flags;
    return PFMI_OK;
}

int32_t pfmi_chees_get_update(pfmi_ctx *c, int64_t t0, int64_t n, double *x, double *xprop, double *vel) {
    PF_CTX(c);
    const HmcState &H = c->hmc;
    PF_CHECK(H.have && H.kind == 2 && H.ch_rec, PFMI_ERR_STATE, "chees_get_update: the last pfmi_chees_enqueue did not run with PFMI_CHEES_RECORD_UPDATE");
    PF_CHECK(H.finished, PFMI_ERR_STATE, "chees_get_update: the run has rounds to go (pfmi_chees_wait)");
    PF_CHECK(t0 >= 0 && n >= 0 && t0 + n <= H.ch_W, PFMI_ERR_ARG, "chees_get_update: updates [%lld, %lld) outside [0, %lld)", (long long)t0,
             (long long)(t0 + n), (long long)H.ch_W);
    const CheesLayout Y(H.K, c->d, H.ch_W, H.ch_T, H.ch_nrec);
    const double *u = c->hm_chees.as<double>() + Y.upd;
    double *dst[3] = {x, xprop, vel};
    for (int q = 0; q < 3; ++q)
        if (dst[q] && n > 0) PF_TRY(pf_download(c, dst[q], u + ((size_t)q * (size_t)H.ch_nrec + (size_t)t0) * Y.vec, sizeof(double) * Y.vec * (size_t)n));
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    return PFMI_OK;
}

int32_t pfmi_chees_stats(pfmi_ctx *c, int64_t *rounds, int64_t *closure_columns) {
    PF_CHECK(c != nullptr, PFMI_ERR_ARG, "null pfmi_ctx");
    PF_CHECK(c->hmc.have && c->hmc.kind == 2, PFMI_ERR_STATE, "chees_stats: no ChEES run on this ctx");
    if (rounds) *rounds = c->hmc.rounds;
    if (closure_columns) *closure_columns = c->hmc.columns;
    return PFMI_OK;
}

int32_t pfmi_host_chees_leapfrog(int64_t t, double traj_length, double step_size, int32_t max_leapfrog, int32_t *clamped) {
    PF_CHECK(t >= 0 && max_leapfrog >= 1 && max_leapfrog <= PF_CHEES_MAX_LEAPFROG, PFMI_ERR_ARG, "host_chees_leapfrog: t < 0 or max_leapfrog outside 1 .. %d",
             PF_CHEES_MAX_LEAPFROG);
    bool cl = false;
    const int32_t L = pf_chees_leapfrog(t, traj_length, step_size, max_leapfrog, &cl);
    if (clamped) *clamped = cl ? 1 : 0;
    return L;
}

int32_t pfmi_host_chees_update(int32_t K, int32_t d, const double *x, const double *xprop, const double *vel, const double *accept, double h,
                               int32_t max_leapfrog, int32_t last, pfmi_chees_state *state) {
    PF_CHECK(K >= 1 && d >= 1 && x && xprop && vel && accept && state, PFMI_ERR_ARG, "host_chees_update: K < 1, d < 1 or a null argument");
    PF_CHECK(max_leapfrog >= 1 && max_leapfrog <= PF_CHEES_MAX_LEAPFROG, PFMI_ERR_ARG, "host_chees_update: max_leapfrog outside 1 .. %d", PF_CHEES_MAX_LEAPFROG);
    std::vector<double> xbar(2 * (size_t)d), pqr(3 * (size_t)K, 0.0);
    for (int32_t i = 0; i < d; ++i) pf_chees_means(K, d, i, x, xprop, accept, &xbar[(size_t)i], &xbar[(size_t)d + i]);
    for (int32_t k = 0; k < K; ++k)
        for (int32_t i = 0; i < d; ++i) {
            const size_t j = (size_t)k * d + i;
            pf_chees_terms(x[j], xprop[j], vel[j], xbar[(size_t)i], xbar[(size_t)d + i], accept[k] == 0.0, pqr[(size_t)k], pqr[(size_t)K + k], pqr[2 * (size_t)K + k]);
        }
    PfChees C = {};
    C.eps = state->step_size; C.tau = state->traj_length; C.s = state->s; C.b = state->b; C.ltb = state->ltb;
    C.da.hbar = state->hbar; C.da.leb = state->leb; C.da.mu = state->mu; C.da.delta = state->delta; C.da.m = state->m; C.da.flags = 0;
    C.Lmax = max_leapfrog; C.status = 0;
    pf_chees_scalars(C, K, accept, pqr.data(), h, last != 0, &state->grad, &state->hmean);
    state->step_size = C.eps; state->traj_length = C.tau; state->s = C.s; state->b = C.b; state->ltb = C.ltb;
    state->hbar = C.da.hbar; state->leb = C.da.leb; state->m = C.da.m; state->status |= C.status | C.da.flags;
    return PFMI_OK;
}

}  // extern "C"
