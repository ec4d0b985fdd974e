// api_fit.hip -- the fits of every trace point: pfmi_fit_batch*, pfmi_set_hinit, pfmi_get_fit*.
#include "api_internal.h"
#include "fit_args.h"
#include <limits.h>

#include <memory>
#include <vector>

int32_t fit_reserve(pfmi_ctx *c, size_t P, int32_t K, size_t d, int32_t J, int32_t kpad) {
    const size_t kk = (size_t)kpad * kpad;
    PF_TRY(c->alpha_all.ensure(sizeof(double) * P * d));
    PF_TRY(c->hist_len.ensure(sizeof(int32_t) * P));
    PF_TRY(c->hist_src.ensure(sizeof(int32_t) * P * J));
    PF_TRY(c->hist_acc.ensure(sizeof(int32_t) * P));
    PF_TRY(c->n_rej.ensure(sizeof(int32_t) * K));
    PF_TRY(c->vh.ensure(sizeof(double) * P * d * kpad));
    PF_TRY(c->tmat.ensure(sizeof(double) * P * kk));
    PF_TRY(c->vchol.ensure(sizeof(double) * P * kk));
    PF_TRY(c->rq.ensure(sizeof(double) * P * kk));
    PF_TRY(c->dmat.ensure(sizeof(double) * P * kk));
    PF_TRY(c->sqrt_alpha.ensure(sizeof(double) * P * d));
    PF_TRY(c->mu.ensure(sizeof(double) * P * d));
    PF_TRY(c->logdet.ensure(sizeof(double) * P));
    PF_TRY(c->status.ensure(sizeof(int32_t) * P));
    PF_HIP(hipMemsetAsync(c->hist_src.p, 0, sizeof(int32_t) * P * J, c->stream));
    return PFMI_OK;
}

static int32_t fit_batch_impl(pfmi_ctx *c, int32_t J, double eps) {
    PF_CHECK(c->P > 0, PFMI_ERR_STATE, "fit_batch: no traces set");
    PF_CHECK(J >= 1, PFMI_ERR_ARG, "history_length must be >= 1");
    // (column padding 64 = history_length 17 .. 32: the slow-but-correct route -- memory-resident fit kernel with its small matrices in
    //  global memory, lane-per-draw kernel for every draw / scan; the tuned kernels stop at 32 columns)
    const int kpad = pf_kpad_for(J);
    PF_CHECK(kpad != 0, PFMI_ERR_UNSUPPORTED, "history_length %d > 32 unsupported", J);
    hmc_forget(c);                                            // the chains' metrics are about to be rewritten
    c->J = J; c->kpad = kpad;
    PF_TRY(fit_reserve(c, (size_t)c->P, c->K, (size_t)c->d, J, kpad));
    if (c->virt) {                                            // streaming layout: every path's slots, the absent ones marked as such
        const HistSeg sg{c->st_npts.as<int32_t>(), 0, INT_MAX, nullptr, nullptr, c->hinit};
        PF_TRY(pf_launch_history(c, eps, &sg));
        PF_TRY(pf_launch_fit(c, 0, (int)c->vcap));
    } else {
        PF_TRY(pf_launch_history(c, eps));
        PF_TRY(pf_launch_fit(c));
    }
    c->fitted = true; c->elbo_done = false; c->pooled = false;
    return PFMI_OK;
}

extern "C" {

// ---- fit ----------------------------------------------------------------------------------------------
int32_t pfmi_set_hinit(pfmi_ctx *c, int32_t hinit) {
    PF_CTX(c);
    PF_CHECK(hinit == PFMI_HINIT_GILBERT || hinit == PFMI_HINIT_SCALAR_YS_OVER_YY, PFMI_ERR_ARG, "set_hinit: unknown Hinit %d", hinit);
    c->hinit = hinit;
    return PFMI_OK;
}
int32_t pfmi_fit_batch(pfmi_ctx *c, int32_t J, double eps) {
    PF_CTX_MUT(c);
    return fit_batch_impl(c, J, eps);
}
int32_t pfmi_fit_batch_ex(pfmi_ctx *c, int32_t J, double eps, int32_t hinit) {
    PF_CTX_MUT(c);
    PF_CHECK(hinit == PFMI_HINIT_GILBERT || hinit == PFMI_HINIT_SCALAR_YS_OVER_YY, PFMI_ERR_ARG, "fit_batch_ex: unknown Hinit %d", hinit);
    const int keep = c->hinit;
    c->hinit = hinit;                                       // for THIS call (pfmi_set_hinit is the persistent setting)
    const int32_t rc = fit_batch_impl(c, J, eps);
    c->hinit = keep;
    return rc;
}

int32_t pfmi_get_fit_status(pfmi_ctx *c, int32_t *status, int32_t *j_eff, double *logdet, int64_t *n_rejected) {
    PF_CTX(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "get_fit_status: call pfmi_fit_batch first");
    auto r = std::make_shared<std::vector<int32_t>>((size_t)c->K);
    if (status) PF_TRY(pf_download(c, status, c->status.p, sizeof(int32_t) * c->P));
    if (j_eff) PF_TRY(pf_download(c, j_eff, c->hist_len.p, sizeof(int32_t) * c->P));
    if (logdet) PF_TRY(pf_download(c, logdet, c->logdet.p, sizeof(double) * c->P));
    if (n_rejected) PF_TRY(pf_download(c, r->data(), c->n_rej.p, sizeof(int32_t) * c->K));
    const int K = c->K;
    auto widen = [r, n_rejected, K]() -> int32_t {
        if (n_rejected)
            for (int k = 0; k < K; ++k) n_rejected[k] = (*r)[(size_t)k];
        return PFMI_OK;
    };
    if (c->defer) { c->post_sync.push_back(widen); return PFMI_OK; }
    PF_TRY(pf_stream_sync(c));
    return widen();
}

int32_t pfmi_get_fit(pfmi_ctx *c, int64_t p, double *alpha, double *B, double *D, double *qr_factors, double *T,
                     double *V, double *mu, double *logdet) {
    PF_CTX(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "get_fit: call pfmi_fit_batch first");
    PF_CHECK(p >= 0 && p < c->P, PFMI_ERR_ARG, "get_fit: point %lld out of range", (long long)p);
    const int d = c->d, J = c->J, kp = c->kpad;
    int32_t j = 0;
    PF_TRY(d2h(c, &j, c->hist_len.as<int32_t>() + p, sizeof(int32_t)));
    const int m = 2 * j, k = d < m ? d : m;
    std::vector<double> al((size_t)d);
    PF_TRY(d2h(c, al.data(), c->alpha_all.as<double>() + (size_t)p * d, sizeof(double) * d));
    if (alpha) memcpy(alpha, al.data(), sizeof(double) * d);
    if (mu) PF_TRY(d2h(c, mu, c->mu.as<double>() + (size_t)p * d, sizeof(double) * d));
    if (logdet) PF_TRY(d2h(c, logdet, c->logdet.as<double>() + p, sizeof(double)));
    const size_t kk = (size_t)kp * kp;
    std::vector<double> small(kk);
    if (B && j > 0) {   // B = [alpha .* Y  S], columns oldest -> newest  (src/inverse_hessian.jl:105-118)
        std::vector<int32_t> src((size_t)J);
        PF_TRY(d2h(c, src.data(), c->hist_src.as<int32_t>() + (size_t)p * J, sizeof(int32_t) * J));
        const int64_t p0 = c->off[(size_t)c->path_of[(size_t)p]];
        std::vector<double> t0((size_t)d), t1((size_t)d), g0((size_t)d), g1((size_t)d);
        for (int cidx = 0; cidx < j; ++cidx) {
            const size_t q0 = (size_t)(p0 + src[(size_t)cidx]) * d, q1 = q0 + d;
            PF_TRY(d2h(c, t0.data(), c->th() + q0, sizeof(double) * d));
            PF_TRY(d2h(c, t1.data(), c->th() + q1, sizeof(double) * d));
            PF_TRY(d2h(c, g0.data(), c->gr() + q0, sizeof(double) * d));
            PF_TRY(d2h(c, g1.data(), c->gr() + q1, sizeof(double) * d));
            for (int i = 0; i < d; ++i) {
                B[i + (size_t)d * cidx] = al[(size_t)i] * (g0[(size_t)i] - g1[(size_t)i]);
                B[i + (size_t)d * (j + cidx)] = t1[(size_t)i] - t0[(size_t)i];
            }
        }
    }
    if (D && m > 0) {
        PF_TRY(d2h(c, small.data(), c->dmat.as<double>() + (size_t)p * kk, sizeof(double) * kk));
        for (int a = 0; a < m; ++a)
            for (int b = 0; b < m; ++b) D[a + (size_t)m * b] = small[(size_t)a * kp + b];
    }
    if (T && k > 0) {
        PF_TRY(d2h(c, small.data(), c->tmat.as<double>() + (size_t)p * kk, sizeof(double) * kk));
        for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b) T[a + (size_t)k * b] = small[(size_t)a * kp + b];
    }
    if (V && k > 0) {
        PF_TRY(d2h(c, small.data(), c->vchol.as<double>() + (size_t)p * kk, sizeof(double) * kk));
        for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b) V[a + (size_t)k * b] = small[(size_t)a * kp + b];
    }
    if (qr_factors && m > 0) {
        std::vector<double> vh((size_t)d * kp);
        PF_TRY(d2h(c, vh.data(), c->vh.as<double>() + (size_t)p * d * kp, sizeof(double) * d * kp));
        PF_TRY(d2h(c, small.data(), c->rq.as<double>() + (size_t)p * kk, sizeof(double) * kk));
        for (int b = 0; b < m; ++b)
            for (int i = 0; i < d; ++i) {
                double v;
                if (i <= b && i < k) v = small[(size_t)i * kp + b];          // R (upper trapezoid)
                else if (b < k) v = vh[(size_t)i * kp + b];                  // Householder vector
                else v = 0.0;
                qr_factors[i + (size_t)d * b] = v;
            }
    }
    return PFMI_OK;
}

}  // extern "C"
