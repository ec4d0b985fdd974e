// api_nuts_fused.hip -- NUTS on the BUILT-IN targets: pfmi_nuts_fused_enqueue of include/pfmi.h over nuts_fused_kernel.hip.  The run is a NUTS
// run (HmcState::kind 1) in the buffers and layouts of pfmi_nuts_enqueue / pfmi_nuts_adapt_enqueue: the checks, the buffer list, the uploads
// and the bookkeeping are api_hmc.hip's (chain_check_chains, chain_begin, chain_refused), waiting and reading stay pfmi_nuts_wait,
// pfmi_nuts_pump, pfmi_nuts_get_stats, pfmi_nuts_get_path, pfmi_hmc_get, pfmi_hmc_draws_dev, pfmi_adapt_get and pfmi_chain_diagnostics
// (api_nuts.hip picks this file's pump for a fused run: HmcState::fused).  What differs is the schedule: the pump has no closure stage, and
// a "round" of it is one LAUNCH of up to HM_FUSED_ROUNDS evaluations per chain.  The device decides how many launches a call takes (a chain
// leaves its launch when it has made its transitions), so they are pumped: at most PF_CHAIN_WINDOW ahead of the last progress word read,
// never more than ceil(evaluations a chain can make / cap).  pfmi_nuts_fused_metric_enqueue is the same body with a staged or resident
// scale allowed and, for nwarmup >= 1, the metric windows of adapt.h: the pump's round launches chains that carry a scale through
// nuts_fused_metric_kernel.hip, and pfmi_adapt_metric_get serves the windows.
//
// Fused and closure NUTS calls never meet on the same resident chains: the fused call needs a built-in target, the closure call a
// DEVICE_CALLBACK one, and every call that replaces the target (pfmi_set_target_*) forgets the chains (hmc_forget), so a CONTINUE of the
// other route finds no chains (PFMI_ERR_STATE).
#include "api_internal.h"
#include "hmc_rows.h"

#include <vector>

static const ChainKind NUTS_FUSED_KIND = {"nuts_fused", "NUTS", "hmc", 1};
static const ChainKind NUTS_FUSED_METRIC_KIND = {"nuts_fused_metric", "NUTS", "hmc", 1};

// the most evaluations of one launch: HM_FUSED_ROUNDS, or the test hook's value
static int64_t nuts_fused_cap() {
    if (const char *v = pf_debug_get("PFMI_NUTS_FUSED_ROUNDS")) {
        const long long n = atoll(v);
        if (n >= 1 && n <= 2147483647ll) return n;
    }
    return HM_FUSED_ROUNDS;
}

// launch number `launch` (1-based) of the call; the path rows are the chains' own trip counts, not the pump's.  Chains that carry a scale
// (HmcState::scaled) take the fused-metric kernel.
static int32_t nuts_fused_round(pfmi_ctx *c, int64_t launch, int64_t) {
    const HmcState &H = c->hmc;
    pf_kernel_begin(c);
    PF_TRY((H.scaled ? pf_launch_nuts_fused_metric : pf_launch_nuts_fused)(c, launch, (int)H.fused_cap, H.fused_reopen && launch == 1, c->stream));
    pf_kernel_end(c, H.scaled ? "nuts_fused_metric" : "nuts_fused");
    return PFMI_OK;
}
static const ChainPump NUTS_FUSED_PUMP = {"nuts", nullptr, nuts_fused_round};
const ChainPump &nuts_fused_pump() { return NUTS_FUSED_PUMP; }

// The one body of pfmi_nuts_fused_enqueue and pfmi_nuts_fused_metric_enqueue.  scale_ok: the entry point takes a staged scale and chains
// that carry one (the fused-metric kernel steps them); metric: CHAIN_METRIC_* of an adaptive run (W >= 1), the metric windows of
// chain_begin.  `closure_route`: the entry point that serves a callback target, for the refusal's message.
static int32_t nuts_fused_enqueue(pfmi_ctx *c, const ChainKind &S, const char *closure_route, int32_t K, const int64_t *points, const double *x0,
                                  const uint64_t *seeds, const double *step_size, int32_t max_depth, int64_t W, int64_t T, double delta, int32_t flags,
                                  bool scale_ok, int metric) {
    HmcState &H = c->hmc;
    const TargetDev &Tg = c->target;
    const bool cont = (flags & PFMI_NUTS_CONTINUE) != 0, rec = (flags & PFMI_NUTS_RECORD_PATH) != 0;
    const ChainCall A = {K, points, x0, seeds, step_size, T, flags, W, delta, metric};
    // (the order of pfmi_nuts_enqueue's checks: fit, target, dimension, null arguments; the sampler's parameter; flags, points, step sizes, CONTINUE)
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "%s_enqueue: call pfmi_fit_batch first", S.name);
    PF_CHECK(Tg.kind == PFMI_TARGET_GAUSS || Tg.kind == PFMI_TARGET_FUNNEL, PFMI_ERR_UNSUPPORTED,
             "%s_enqueue: needs a built-in target (PFMI_TARGET_GAUSS, PFMI_TARGET_FUNNEL); a DEVICE_CALLBACK target with a gradient closure "
             "runs through %s", S.name, closure_route);
    PF_CHECK(Tg.d == c->d, PFMI_ERR_STATE, "%s_enqueue: the target's dimension %d is not the fit's %d", S.name, Tg.d, c->d);
    PF_CHECK(K >= 1 && points && seeds && step_size && (cont || x0), PFMI_ERR_ARG, "%s_enqueue: K < 1 or a null argument", S.name);
    PF_CHECK(max_depth >= 1 && max_depth <= 10 && T >= 1, PFMI_ERR_ARG, "%s_enqueue: max_depth %d outside 1 .. 10 or ntransitions %lld < 1",
             S.name, max_depth, (long long)T);
    PF_TRY(chain_check_chains(c, S, A));
    // (pfmi_nuts_fused_enqueue launches the fused kernel alone: a staged scale, or resident chains that carry one, are the other entry point's)
    PF_CHECK(scale_ok || (c->scale_staged.empty() && !(cont && H.scaled)), PFMI_ERR_UNSUPPORTED,
             "%s_enqueue: chains with a per-coordinate scale (pfmi_chain_scale_set) are not supported; pfmi_nuts_fused_metric_enqueue runs them", S.name);
    PF_CHECK(!cont || H.md_alloc >= max_depth, PFMI_ERR_ARG, "%s_enqueue: PFMI_NUTS_CONTINUE with max_depth %d above the chains' %d", S.name, max_depth,
             H.md_alloc);
    PF_CHECK(((double)W + (double)T) * 1024.0 < 2147483648.0, PFMI_ERR_UNSUPPORTED, "%s_enqueue: %lld transitions in one call", S.name, (long long)(W + T));
    const size_t vec = sizeof(double) * (size_t)K * c->d, rows = (size_t)K * (size_t)T;
    // (pfmi_nuts_enqueue's list: checkpoints and, with RECORD_PATH, one event per chain and evaluation of the bound included)
    std::vector<ChainBuf> own = {{&c->nt_vec, vec * (size_t)pf_nuts_vec_slots(max_depth), CHAIN_BUF},
                                 {&c->nt_st, pf_nuts_chain_bytes() * (size_t)K, CHAIN_BUF, false},
                                 {&c->nt_ctr, sizeof(int32_t) * 2, CHAIN_BUF, false},
                                 {&c->nt_depth, sizeof(int32_t) * rows, CALL_BUF},
                                 {&c->nt_nleap, sizeof(int32_t) * rows, CALL_BUF},
                                 {&c->nt_pev, sizeof(pfmi_nuts_event) * (size_t)K, PATH_BUF}};
    char detail[32];
    snprintf(detail, sizeof detail, ", max_depth %d", max_depth);
    int64_t trips = 0;                                    // the most evaluations a chain can make in this call
    PF_TRY(chain_begin(c, S, A, ((int64_t)1 << max_depth) - 1, detail, own, nuts_drain, &trips));
    if (!c->nt_status) PF_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->nt_status), sizeof(int64_t), hipHostMallocCoherent | hipHostMallocMapped));
    if (rec) PF_HIP(hipMemsetAsync(c->nt_pev.p, 0xff, sizeof(pfmi_nuts_event) * (size_t)K * (size_t)trips, c->stream));   // t = -1: a row no running chain wrote
    const int64_t cap = nuts_fused_cap();
    H.nleap = 0;
    H.max_depth = max_depth;
    if (!cont) H.md_alloc = max_depth;
    H.fused = true; H.fused_reopen = cont; H.fused_cap = cap;
    H.issued = 0; H.seen = 0; H.max_rounds = (trips + cap - 1) / cap; H.finished = false;
    __atomic_store_n(c->nt_status, (int64_t)K, __ATOMIC_RELEASE);               // launch 0: every chain running
    PF_HIP(hipMemsetAsync(c->nt_ctr.p, 0, sizeof(int32_t) * 2, c->stream));
    if (!cont) PF_TRY(pf_launch_nuts_init(c, c->stream));
    return chain_issue_rounds(c, NUTS_FUSED_PUMP);
}

extern "C" {

int32_t pfmi_nuts_fused_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                                int32_t max_depth, int64_t nwarmup, int64_t ntransitions, double target_accept, int32_t flags) {
    PF_CTX_MUT(c);
    int32_t rc = PFMI_OK;
    if (nwarmup != 0) rc = adapt_args("nuts_fused_enqueue", nwarmup, target_accept, flags);      // (nwarmup < 0: its PFMI_ERR_ARG)
    if (rc == PFMI_OK)
        rc = nuts_fused_enqueue(c, NUTS_FUSED_KIND, "pfmi_nuts_enqueue", K, points, x0, seeds, step_size, max_depth, nwarmup, ntransitions,
                                nwarmup ? target_accept : 0.0, flags, false, CHAIN_METRIC_NONE);
    return chain_refused(c, rc);
}

int32_t pfmi_nuts_fused_metric_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                                       int32_t max_depth, int64_t nwarmup, int64_t ntransitions, double target_accept, int32_t flags) {
    PF_CTX_MUT(c);
    int32_t rc = PFMI_OK;
    int metric = CHAIN_METRIC_NONE;
    if (nwarmup != 0) {                 // an adaptive run is a fresh run: its one flag selects the record of the whitened rows
        rc = adapt_args("nuts_fused_metric_enqueue", nwarmup, target_accept, flags, PFMI_ADAPT_RECORD_WHITENED);
        metric = (flags & PFMI_ADAPT_RECORD_WHITENED) ? CHAIN_METRIC_RECORD : CHAIN_METRIC_WINDOWS;
        flags = 0;
    }
    if (rc == PFMI_OK)
        rc = nuts_fused_enqueue(c, NUTS_FUSED_METRIC_KIND, "pfmi_nuts_adapt_metric_enqueue (a plain run on a scale: pfmi_nuts_enqueue)", K, points, x0, seeds,
                                step_size, max_depth, nwarmup, ntransitions, nwarmup ? target_accept : 0.0, flags, true, metric);
    return chain_refused(c, rc);
}

}  // extern "C"
