// api_nuts.hip -- NUTS on a fitted metric for gradient closures: the entry points of include/pfmi.h over nuts_kernel.hip.  The chains, the
// closure buffers and the record buffers are static HMC's (api_hmc.hip: pfmi_hmc_get, pfmi_hmc_draws_dev and pfmi_chain_diagnostics serve a
// NUTS run unchanged), and so is the enqueue path (chain_begin, api_hmc.hip); what is NUTS's own is here: its buffers, the progress word
// and its rounds.  The rounds are scheduled by the one pump of the samplers whose round count the device decides (chain_issue_rounds, api_hmc.hip).
#include "api_internal.h"

#include <math.h>
#include <vector>

// a NUTS round: the closure's stage name, and the step launch behind the closure
static const char *nuts_closure_stage(const HmcState &H) { return H.scaled ? "nuts_metric_closure" : H.adapting ? "nuts_adapt_closure" : "nuts_closure"; }
static int32_t nuts_round(pfmi_ctx *c, int64_t round, int64_t prow) {
    const HmcState &H = c->hmc;
    pf_kernel_begin(c);
    PF_TRY((H.scaled ? pf_launch_nuts_metric_step : pf_launch_nuts_step)(c, round, prow, false, c->stream));
    pf_kernel_end(c, H.scaled ? "nuts_metric" : H.adapting ? "nuts_adapt" : "nuts");
    return PFMI_OK;
}
static const ChainPump NUTS_PUMP = {"nuts", nuts_closure_stage, nuts_round};
// the pump of the NUTS run on the ctx: a fused run's rounds are launches without a closure (api_nuts_fused.hip)
static const ChainPump &nuts_pump_of(const HmcState &H) { return H.fused ? nuts_fused_pump() : NUTS_PUMP; }
int32_t nuts_drain(pfmi_ctx *c) { return chain_drain(c, nuts_pump_of(c->hmc)); }

static const ChainKind NUTS_KIND = {"nuts", "NUTS", "hmc", 1};

int32_t nuts_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                     int32_t max_depth, int64_t T, int32_t flags, int64_t W, double delta, int metric) {
    HmcState &H = c->hmc;
    const bool cont = (flags & PFMI_NUTS_CONTINUE) != 0, rec = (flags & PFMI_NUTS_RECORD_PATH) != 0;
    const ChainCall A = {K, points, x0, seeds, step_size, T, flags, W, delta, metric};
    PF_TRY(chain_check_target(c, NUTS_KIND, A));
    PF_CHECK(max_depth >= 1 && max_depth <= 10 && T >= 1, PFMI_ERR_ARG, "nuts_enqueue: max_depth %d outside 1 .. 10 or ntransitions %lld < 1", max_depth,
             (long long)T);
    PF_TRY(chain_check_chains(c, NUTS_KIND, A));
    PF_CHECK(!cont || H.md_alloc >= max_depth, PFMI_ERR_ARG, "nuts_enqueue: PFMI_NUTS_CONTINUE with max_depth %d above the chains' %d", max_depth,
             H.md_alloc);
    PF_CHECK(((double)W + (double)T) * 1024.0 < 2147483648.0, PFMI_ERR_UNSUPPORTED, "nuts_enqueue: %lld transitions in one call", (long long)(W + T));
    const size_t vec = sizeof(double) * (size_t)K * c->d, rows = (size_t)K * (size_t)T;
    // (checkpoints and, with RECORD_PATH, one event per chain and round of the cap included)
    std::vector<ChainBuf> own = {{&c->nt_vec, vec * (size_t)pf_nuts_vec_slots(max_depth), CHAIN_BUF},
                                 {&c->nt_st, pf_nuts_chain_bytes() * (size_t)K, CHAIN_BUF, false},
                                 {&c->nt_ctr, sizeof(int32_t) * 2, CHAIN_BUF, false},
                                 {&c->nt_depth, sizeof(int32_t) * rows, CALL_BUF},
                                 {&c->nt_nleap, sizeof(int32_t) * rows, CALL_BUF},
                                 {&c->nt_pev, sizeof(pfmi_nuts_event) * (size_t)K, PATH_BUF}};
    char detail[32];
    snprintf(detail, sizeof detail, ", max_depth %d", max_depth);
    int64_t rounds = 0;
    PF_TRY(chain_begin(c, NUTS_KIND, A, ((int64_t)1 << max_depth) - 1, detail, own, nuts_drain, &rounds));
    if (!c->nt_status) PF_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->nt_status), sizeof(int64_t), hipHostMallocCoherent | hipHostMallocMapped));
    if (rec) PF_HIP(hipMemsetAsync(c->nt_pev.p, 0xff, sizeof(pfmi_nuts_event) * (size_t)K * (size_t)rounds, c->stream));   // t = -1: a column no running chain wrote
    H.nleap = 0;
    H.max_depth = max_depth;
    if (!cont) H.md_alloc = max_depth;                    // (a CONTINUE never asks for more checkpoints than the chains were given)
    H.fused = false;
    H.issued = 0; H.seen = 0; H.max_rounds = rounds; H.finished = false;
    __atomic_store_n(c->nt_status, (int64_t)K, __ATOMIC_RELEASE);               // round 0: every chain running
    PF_HIP(hipMemsetAsync(c->nt_ctr.p, 0, sizeof(int32_t) * 2, c->stream));
    if (!cont) PF_TRY(pf_launch_nuts_init(c, c->stream));
    else {
        pf_kernel_begin(c);
        PF_TRY((H.scaled ? pf_launch_nuts_metric_step : pf_launch_nuts_step)(c, 0, 0, true, c->stream));
        pf_kernel_end(c, H.scaled ? "nuts_metric" : "nuts");
    }
    return chain_issue_rounds(c, NUTS_PUMP);
}

extern "C" {

int32_t pfmi_nuts_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                          int32_t max_depth, int64_t ntransitions, int32_t flags) {
    PF_CTX_MUT(c);
    return chain_refused(c, nuts_enqueue(c, K, points, x0, seeds, step_size, max_depth, ntransitions, flags, 0, 0.0));
}

int32_t pfmi_nuts_pump(pfmi_ctx *c, int32_t *finished) {
    PF_CHECK(c != nullptr && finished != nullptr, PFMI_ERR_ARG, "nuts_pump: null argument");
    PF_CHECK(c->hmc.have && c->hmc.kind == 1, PFMI_ERR_STATE, "nuts_pump: no pfmi_nuts_enqueue outstanding");
    PF_HIP(hipSetDevice(c->device));
    return chain_refused(c, chain_pump_pass(c, nuts_pump_of(c->hmc), finished));  // a failed pass ends the run: what is in flight is drained
}

int32_t pfmi_nuts_wait(pfmi_ctx *c) {
    PF_CTX(c);
    HmcState &H = c->hmc;
    PF_CHECK(H.have && H.kind == 1, PFMI_ERR_STATE, "nuts_wait: no pfmi_nuts_enqueue outstanding");
    PF_TRY(chain_refused(c, nuts_drain(c)));
    PF_TRY(pf_stream_sync(c));
    H.active = false;
    std::vector<int32_t> dead;
    int64_t last = 0;
    PF_TRY(pf_nuts_chain_flags(c, dead, &last));
    H.rounds = last;
    return chain_dead_check(c, "nuts", dead);
}

int32_t pfmi_nuts_get_stats(pfmi_ctx *c, int32_t *tree_depth, int32_t *n_leapfrog) {
    PF_CTX(c);
    const HmcState &H = c->hmc;
    PF_CHECK(H.have && H.kind == 1, PFMI_ERR_STATE, "nuts_get_stats: no NUTS run on this ctx");
    PF_CHECK(H.finished, PFMI_ERR_STATE, "nuts_get_stats: the run has rounds to go (pfmi_nuts_wait)");
    const size_t rows = (size_t)H.K * (size_t)H.T;
    if (tree_depth) PF_TRY(pf_download(c, tree_depth, c->nt_depth.p, sizeof(int32_t) * rows));
    if (n_leapfrog) PF_TRY(pf_download(c, n_leapfrog, c->nt_nleap.p, sizeof(int32_t) * rows));
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    return PFMI_OK;
}

int32_t pfmi_nuts_get_path(pfmi_ctx *c, int64_t round0, int64_t nrounds, double *X, double *closure_out, double *v, pfmi_nuts_event *events) {
    PF_CTX(c);
    const HmcState &H = c->hmc;
    PF_CHECK(H.have && H.record && H.kind == 1, PFMI_ERR_STATE, "nuts_get_path: the last pfmi_nuts_enqueue did not run with PFMI_NUTS_RECORD_PATH");
    PF_CHECK(H.finished, PFMI_ERR_STATE, "nuts_get_path: the run has rounds to go (pfmi_nuts_wait)");
    int64_t bound = H.issued;                             // a row per round issued; a fused run: per trip of the chain that made the most
    if (H.fused) {
        std::vector<int32_t> dead;
        PF_TRY(pf_nuts_chain_flags(c, dead, &bound));
    }
    PF_CHECK(round0 >= 0 && nrounds >= 0 && round0 + nrounds <= bound, PFMI_ERR_ARG, "nuts_get_path: rounds [%lld, %lld) outside [0, %lld)",
             (long long)round0, (long long)(round0 + nrounds), (long long)bound);
    PF_TRY(chain_path_download(c, round0, nrounds, X, closure_out, v));
    if (events)
        PF_TRY(pf_download(c, events, c->nt_pev.as<pfmi_nuts_event>() + (size_t)round0 * H.K, sizeof(pfmi_nuts_event) * (size_t)H.K * (size_t)nrounds));
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    return PFMI_OK;
}

int32_t pfmi_nuts_stats(pfmi_ctx *c, int64_t *rounds, int64_t *closure_columns) {
    PF_CHECK(c != nullptr, PFMI_ERR_ARG, "null pfmi_ctx");
    PF_CHECK(c->hmc.kind == 1, PFMI_ERR_STATE, "nuts_stats: no NUTS run on this ctx");
    if (rounds) *rounds = c->hmc.rounds;
    if (closure_columns) *closure_columns = c->hmc.columns;
    return PFMI_OK;
}

}  // extern "C"
