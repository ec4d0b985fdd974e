// api_adapt.hip -- the device-resident warm-up: static HMC and NUTS whose first W transitions adapt the step size on the device (adapt.h,
// the warm kernels of hmc_kernel.hip / nuts_kernel.hip), behind the enqueues of api_hmc.hip / api_nuts.hip.  One enqueue runs warm-up and
// sampling back to back; waiting, pumping and reading rows stay pfmi_hmc_wait, pfmi_nuts_pump / pfmi_nuts_wait and pfmi_hmc_get.
#include "api_internal.h"
#include "adapt.h"
#include "hmc_rows.h"

#include <math.h>
#include <vector>

// PfAdapt [K], PfWarmRow [K][W], then the [K] final step sizes a plain CONTINUE would otherwise overwrite
static size_t adapt_eps_offset(int32_t K, int64_t W) { return sizeof(PfAdapt) * (size_t)K + sizeof(PfWarmRow) * (size_t)K * (size_t)W; }
size_t adapt_bytes(int32_t K, int64_t W) { return adapt_eps_offset(K, W) + sizeof(double) * (size_t)K; }

int32_t adapt_keep_step_sizes(pfmi_ctx *c) {
    HmcState &H = c->hmc;
    if (H.W <= 0 || H.eps_kept) return PFMI_OK;
    PF_HIP(hipMemcpyAsync(c->hm_adapt.as<char>() + adapt_eps_offset(H.K, H.W), c->hm_eps.p, sizeof(double) * (size_t)H.K, hipMemcpyDeviceToDevice,
                          c->stream));
    H.eps_kept = true;
    return PFMI_OK;
}

// the adaptation states of K chains that start at step_size[k], and their empty traces (hm_adapt holds adapt_bytes(K, W): chain_begin)
int32_t adapt_reset(pfmi_ctx *c, int32_t K, int64_t W, const double *step_size, double delta, int32_t status0) {
    std::vector<PfAdapt> st((size_t)K);
    for (int k = 0; k < K; ++k) { st[(size_t)k] = pf_adapt_init(step_size[k], delta); st[(size_t)k].flags = status0; }
    PF_TRY(pf_upload(c, c->hm_adapt.p, st.data(), sizeof(PfAdapt) * (size_t)K));
    PF_HIP(hipMemsetAsync(c->hm_adapt.as<PfAdapt>() + K, 0, sizeof(PfWarmRow) * (size_t)K * (size_t)W, c->stream));
    return PFMI_OK;
}

// ---- the metric windows (adapt.h) and the chains' scale
int32_t metric_plan(pfmi_ctx *c, const ChainCall &A, std::vector<ChainBuf> &bufs, MetricPlan &P) {
    const size_t vec = sizeof(double) * (size_t)A.K * c->d;
    P.scale = std::move(c->scale_staged);
    c->scale_staged.clear();
    if (A.metric != CHAIN_METRIC_NONE) {
        int64_t term = 0;
        P.nwin = pf_adapt_windows(A.W, &P.init, &term, P.ends);
        PF_CHECK(P.nwin <= PF_ADAPT_MAX_WINDOWS && A.W < 2147483648ll, PFMI_ERR_UNSUPPORTED, "adapt_metric_enqueue: nwarmup %lld is beyond 2^31", (long long)A.W);
    }
    if (!P.scale.empty() || P.nwin > 0) bufs.push_back({&c->hm_scale, vec, CALL_BUF});
    if (P.nwin > 0) {
        const int64_t nwt = A.metric == CHAIN_METRIC_RECORD ? P.ends[P.nwin - 1] - P.init : 0;
        bufs.push_back({&c->hm_metric, pf_metric_bytes(A.K, c->d, P.nwin, nwt), CALL_BUF});
    }
    return PFMI_OK;
}

int32_t metric_begin(pfmi_ctx *c, const ChainCall &A, const MetricPlan &P) {
    HmcState &H = c->hmc;
    const size_t n = (size_t)A.K * c->d;
    if (!P.scale.empty()) {
        PF_TRY(pf_upload(c, c->hm_scale.p, P.scale.data(), sizeof(double) * n));
        H.scaled = true;
    } else if (P.nwin > 0 && !H.scaled) {
        const std::vector<double> ones(n, 1.0);
        PF_TRY(pf_upload(c, c->hm_scale.p, ones.data(), sizeof(double) * n));
        H.scaled = true;
    }
    if (A.metric == CHAIN_METRIC_NONE) return PFMI_OK;
    H.metric_run = true; H.nwin = P.nwin; H.win_init = P.init; H.rec_u = A.metric == CHAIN_METRIC_RECORD && P.nwin > 0;
    for (int j = 0; j < P.nwin; ++j) H.win_ends[j] = P.ends[j];
    if (P.nwin > 0) {
        int32_t tab[2 + PF_ADAPT_MAX_WINDOWS] = {P.nwin, (int32_t)P.init};
        for (int j = 0; j < P.nwin; ++j) tab[2 + j] = (int32_t)P.ends[j];
        PF_TRY(pf_upload(c, c->hm_metric.p, tab, sizeof tab));
        const size_t bytes = pf_metric_bytes(A.K, c->d, P.nwin, H.rec_u ? P.ends[P.nwin - 1] - P.init : 0);
        PF_HIP(hipMemsetAsync(c->hm_metric.as<char>() + PF_METRIC_HEAD, 0, bytes - PF_METRIC_HEAD, c->stream));   // Welford state and traces
    }
    return PFMI_OK;
}

int32_t adapt_args(const char *who, int64_t W, double delta, int32_t flags, int32_t allowed) {
    PF_CHECK((flags & ~allowed) == 0, PFMI_ERR_ARG, "%s: flags %d not among %d (an adaptive run is a fresh run without a recorded path)", who, flags, allowed);
    PF_CHECK(W >= 1, PFMI_ERR_ARG, "%s: nwarmup %lld must be >= 1", who, (long long)W);
    PF_CHECK(delta > 0.0 && delta < 1.0, PFMI_ERR_ARG, "%s: target_accept %g outside (0, 1)", who, delta);
    return PFMI_OK;
}

extern "C" {

int32_t pfmi_hmc_adapt_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size0,
                               int32_t nleapfrog, int64_t nwarmup, int64_t ntransitions, double target_accept, int32_t flags) {
    PF_CTX_MUT(c);
    int32_t rc = adapt_args("hmc_adapt_enqueue", nwarmup, target_accept, flags);
    if (rc == PFMI_OK) rc = hmc_enqueue(c, K, points, x0, seeds, step_size0, nleapfrog, ntransitions, 0, nwarmup, target_accept);
    return chain_refused(c, rc);        // (as every other error of the enqueues, a refused argument leaves no chains and no traces behind)
}

int32_t pfmi_nuts_adapt_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size0,
                                int32_t max_depth, int64_t nwarmup, int64_t ntransitions, double target_accept, int32_t flags) {
    PF_CTX_MUT(c);
    int32_t rc = adapt_args("nuts_adapt_enqueue", nwarmup, target_accept, flags);
    if (rc == PFMI_OK) rc = nuts_enqueue(c, K, points, x0, seeds, step_size0, max_depth, ntransitions, 0, nwarmup, target_accept);
    return chain_refused(c, rc);
}

int32_t pfmi_hmc_adapt_metric_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size0,
                                      int32_t nleapfrog, int64_t nwarmup, int64_t ntransitions, double target_accept, int32_t flags) {
    PF_CTX_MUT(c);
    int32_t rc = adapt_args("hmc_adapt_metric_enqueue", nwarmup, target_accept, flags, PFMI_ADAPT_RECORD_WHITENED);
    const int metric = (flags & PFMI_ADAPT_RECORD_WHITENED) ? CHAIN_METRIC_RECORD : CHAIN_METRIC_WINDOWS;
    if (rc == PFMI_OK) rc = hmc_enqueue(c, K, points, x0, seeds, step_size0, nleapfrog, ntransitions, 0, nwarmup, target_accept, metric);
    return chain_refused(c, rc);
}

int32_t pfmi_nuts_adapt_metric_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size0,
                                       int32_t max_depth, int64_t nwarmup, int64_t ntransitions, double target_accept, int32_t flags) {
    PF_CTX_MUT(c);
    int32_t rc = adapt_args("nuts_adapt_metric_enqueue", nwarmup, target_accept, flags, PFMI_ADAPT_RECORD_WHITENED);
    const int metric = (flags & PFMI_ADAPT_RECORD_WHITENED) ? CHAIN_METRIC_RECORD : CHAIN_METRIC_WINDOWS;
    if (rc == PFMI_OK) rc = nuts_enqueue(c, K, points, x0, seeds, step_size0, max_depth, ntransitions, 0, nwarmup, target_accept, metric);
    return chain_refused(c, rc);
}

int32_t pfmi_chain_scale_set(pfmi_ctx *c, int32_t K, const double *scale) {
    PF_CHECK(c != nullptr, PFMI_ERR_ARG, "null pfmi_ctx");
    c->scale_staged.clear();
    c->scale_staged_K = 0;
    if (!scale) return PFMI_OK;
    PF_CHECK(c->d >= 1, PFMI_ERR_STATE, "chain_scale_set: no traces, so no dimension");
    const size_t n = K >= 1 ? (size_t)K * c->d : 0;
    bool ok = K >= 1;
    for (size_t i = 0; ok && i < n; ++i) ok = scale[i] > 0.0 && isfinite(scale[i]);
    if (!ok) {                                            // as every refused enqueue: no chains are left to run on a scale the caller did not mean
        PF_HIP(hipSetDevice(c->device));
        (void)chain_refused(c, PFMI_ERR_ARG);
        PF_CHECK(false, PFMI_ERR_ARG, "chain_scale_set: K %d < 1 or a scale that is not positive and finite", K);
    }
    c->scale_staged.assign(scale, scale + n);
    c->scale_staged_K = K;
    return PFMI_OK;
}

int32_t pfmi_adapt_metric_get(pfmi_ctx *c, int32_t *nwindows, int64_t *ends, double *scale_trace, double *whitened) {
    PF_CTX(c);
    const HmcState &H = c->hmc;
    PF_CHECK(H.have && H.W > 0 && H.metric_run, PFMI_ERR_STATE, "adapt_metric_get: no run with metric windows on this ctx");
    PF_CHECK(H.finished, PFMI_ERR_STATE, "adapt_metric_get: the NUTS run has rounds to go (pfmi_nuts_wait)");
    PF_CHECK(whitened == nullptr || H.rec_u || H.nwin == 0, PFMI_ERR_STATE, "adapt_metric_get: the run did not keep its whitened rows (PFMI_ADAPT_RECORD_WHITENED)");
    if (nwindows) *nwindows = H.nwin;
    for (int j = 0; ends && j < H.nwin; ++j) ends[j] = H.win_ends[j];
    const size_t vec = (size_t)H.K * c->d;
    if (H.nwin > 0) {
        if (scale_trace) PF_TRY(pf_download(c, scale_trace, pf_metric_strace(c), sizeof(double) * vec * (size_t)H.nwin));
        if (whitened)
            PF_TRY(pf_download(c, whitened, pf_metric_strace(c) + vec * (size_t)H.nwin, sizeof(double) * vec * (size_t)(H.win_ends[H.nwin - 1] - H.win_init)));
    }
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    return PFMI_OK;
}

int32_t pfmi_adapt_windows(int64_t nwarmup, int64_t *init, int64_t *term, int64_t *ends, int32_t cap, int32_t *nwindows) {
    PF_CHECK(nwarmup >= 1 && init && term && nwindows && cap >= 0 && (ends || cap == 0), PFMI_ERR_ARG, "adapt_windows: nwarmup < 1 or a null argument");
    int64_t e[PF_ADAPT_MAX_WINDOWS];
    const int n = pf_adapt_windows(nwarmup, init, term, e);
    PF_CHECK(n <= cap && n <= PF_ADAPT_MAX_WINDOWS, PFMI_ERR_ARG, "adapt_windows: %d windows, room for %d", n, cap);
    for (int j = 0; j < n; ++j) ends[j] = e[j];
    *nwindows = n;
    return PFMI_OK;
}

int32_t pfmi_host_metric_update(int64_t n, int32_t d, const double *u, const double *scale_in, double *scale_out, int32_t *status) {
    PF_CHECK(n >= 2 && d >= 1 && u && scale_in && scale_out, PFMI_ERR_ARG, "host_metric_update: n < 2, d < 1 or a null argument");
    bool bad = false;
    for (int32_t i = 0; i < d; ++i) {
        double mean = 0.0, m2 = 0.0;
        for (int64_t t = 0; t < n; ++t) pf_welford_update((double)(t + 1), u[(size_t)t * d + i], mean, m2);
        const double D = pf_metric_var((double)n, m2);
        bad = bad || !pf_metric_var_ok(D);
        scale_out[i] = sqrt(D);
    }
    if (bad) for (int32_t i = 0; i < d; ++i) scale_out[i] = scale_in[i];
    if (status) *status = bad ? PF_ADAPT_KEPT_METRIC : 0;
    return PFMI_OK;
}

int32_t pfmi_adapt_get(pfmi_ctx *c, double *step_size, double *eps_trace, double *accept_trace, int32_t *divergent, int32_t *n_leapfrog,
                       int32_t *status) {
    PF_CTX(c);
    const HmcState &H = c->hmc;
    PF_CHECK(H.have && H.W > 0, PFMI_ERR_STATE, "adapt_get: no adaptive run on this ctx");
    PF_CHECK(H.finished, PFMI_ERR_STATE, "adapt_get: the NUTS run has rounds to go (pfmi_nuts_wait)");
    const size_t K = (size_t)H.K, W = (size_t)H.W;
    std::vector<PfAdapt> st(K);
    std::vector<PfWarmRow> tr(K * W);
    std::vector<double> eps(K);
    PF_TRY(pf_stream_sync(c));
    PF_HIP(hipMemcpy(st.data(), c->hm_adapt.p, sizeof(PfAdapt) * K, hipMemcpyDeviceToHost));
    PF_HIP(hipMemcpy(tr.data(), c->hm_adapt.as<PfAdapt>() + K, sizeof(PfWarmRow) * K * W, hipMemcpyDeviceToHost));
    const void *eps_src = H.eps_kept ? (const void *)(c->hm_adapt.as<char>() + adapt_eps_offset(H.K, H.W)) : (const void *)c->hm_eps.p;
    PF_HIP(hipMemcpy(eps.data(), eps_src, sizeof(double) * K, hipMemcpyDeviceToHost));
    c->hmc.active = false;
    for (size_t k = 0; k < K; ++k) {
        if (step_size) step_size[k] = eps[k];
        if (status) status[k] = st[k].flags;
        for (size_t t = 0; t < W; ++t) {
            const PfWarmRow &r = tr[k * W + t];
            if (eps_trace) eps_trace[k * W + t] = r.eps;
            if (accept_trace) accept_trace[k * W + t] = r.acc;
            if (divergent) divergent[k * W + t] = r.div;
            if (n_leapfrog) n_leapfrog[k * W + t] = r.nleap;
        }
    }
    return PFMI_OK;
}

int32_t pfmi_host_dual_averaging(int64_t n, double eps0, double target_accept, const double *accept, double *eps, double *eps_bar) {
    PF_CHECK(n >= 0 && (accept != nullptr || n == 0) && eps != nullptr, PFMI_ERR_ARG, "host_dual_averaging: n < 0 or a null argument");
    PF_CHECK(isfinite(eps0) && eps0 > 0.0, PFMI_ERR_ARG, "host_dual_averaging: eps0 is not positive and finite");
    PF_CHECK(target_accept > 0.0 && target_accept < 1.0, PFMI_ERR_ARG, "host_dual_averaging: target_accept %g outside (0, 1)", target_accept);
    PfAdapt S = pf_adapt_init(eps0, target_accept);
    eps[0] = eps0;
    for (int64_t t = 0; t < n; ++t) {
        const double le = pf_adapt_update(S, accept[t]);
        eps[t + 1] = pf_adapt_pick(S, le, eps[t]);
        if (eps_bar) eps_bar[t] = exp(S.leb);
    }
    return PFMI_OK;
}

}  // extern "C"
