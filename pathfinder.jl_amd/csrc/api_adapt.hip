// api_adapt.hip -- the device-resident warm-up: static HMC and NUTS whose first W transitions adapt the step size on the device (adapt.h,
// the warm kernels of hmc_kernel.hip / nuts_kernel.hip), behind the enqueues of api_hmc.hip / api_nuts.hip.  One enqueue runs warm-up and
// sampling back to back; waiting, pumping and reading rows stay pfmi_hmc_wait, pfmi_nuts_pump / pfmi_nuts_wait and pfmi_hmc_get.
#include "api_internal.h"
#include "adapt.h"

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
int32_t adapt_reset(pfmi_ctx *c, int32_t K, int64_t W, const double *step_size, double delta) {
    std::vector<PfAdapt> st((size_t)K);
    for (int k = 0; k < K; ++k) st[(size_t)k] = pf_adapt_init(step_size[k], delta);
    PF_TRY(pf_upload(c, c->hm_adapt.p, st.data(), sizeof(PfAdapt) * (size_t)K));
    PF_HIP(hipMemsetAsync(c->hm_adapt.as<PfAdapt>() + K, 0, sizeof(PfWarmRow) * (size_t)K * (size_t)W, c->stream));
    return PFMI_OK;
}

static int32_t adapt_args(const char *who, int64_t W, double delta, int32_t flags) {
    PF_CHECK(flags == 0, PFMI_ERR_ARG, "%s: flags must be 0 (an adaptive run is a fresh run without a recorded path), got %d", who, flags);
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
