// logpdf_lane.h -- logpdf(MvNormal(mu_p, W_p), x) of one column x, computed by one lane.  Used by pf_logpdf_kernel
// (pfmi_logpdf) and by the general path of the mixture kernels (mixture_kernels.hip), which therefore agree bit for bit.
#pragma once
#include "pfmi_common.h"

// logpdf(MvNormal(mu, W), x) = -(d log2pi + logdet)/2 - |L \ (x - mu)|^2 / 2; NaN for a fit whose status is not PFMI_FIT_OK.
// ldiv!(L): z = U'^{-1}(x - mu); z <- Q'z = z - Vh T'(Vh' z); z[1:k] <- V'^{-1} z[1:k]  (src/woodbury.jl:158-165)
template <int KPAD>
__device__ __forceinline__ double pf_logpdf_lane(int d, int p, const double *__restrict__ X, const double *__restrict__ vh,
                                                 const double *__restrict__ tmat, const double *__restrict__ vchol,
                                                 const double *__restrict__ sqrt_alpha, const double *__restrict__ mu_all,
                                                 const double *__restrict__ logdet, const int32_t *__restrict__ status) {
    if (status[p] != PFMI_FIT_OK) return NAN;
    const double *Vh = vh + (size_t)p * d * KPAD, *T = tmat + (size_t)p * KPAD * KPAD, *Vc = vchol + (size_t)p * KPAD * KPAD;
    const double *sqa = sqrt_alpha + (size_t)p * d, *mu = mu_all + (size_t)p * d;
    double w[KPAD], tv[KPAD], zh[KPAD];
#pragma unroll
    for (int j = 0; j < KPAD; ++j) w[j] = 0.0;
    for (int i = 0; i < d; ++i) {
        const double e = (X[i] - mu[i]) / sqa[i];
        const double *row = Vh + (size_t)i * KPAD;
#pragma unroll
        for (int j = 0; j < KPAD; ++j) w[j] += row[j] * e;
    }
#pragma unroll
    for (int a = 0; a < KPAD; ++a) {   // tv = T' w
        double s = 0.0;
#pragma unroll
        for (int b = 0; b <= a; ++b) s += T[b * KPAD + a] * w[b];
        tv[a] = s;
    }
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < KPAD; ++i) {
        zh[i] = 0.0;
        if (i < d) {
            const double *row = Vh + (size_t)i * KPAD;
            double v = (X[i] - mu[i]) / sqa[i];
#pragma unroll
            for (int j = 0; j < KPAD; ++j) v -= row[j] * tv[j];
            zh[i] = v;
        }
    }
    for (int i = KPAD; i < d; ++i) {
        const double *row = Vh + (size_t)i * KPAD;
        double v = (X[i] - mu[i]) / sqa[i];
#pragma unroll
        for (int j = 0; j < KPAD; ++j) v -= row[j] * tv[j];
        ss += v * v;
    }
#pragma unroll
    for (int a = 0; a < KPAD; ++a) {   // forward substitution V' y = zh (identity padded)
        double v = zh[a];
#pragma unroll
        for (int b = 0; b < a; ++b) v -= Vc[b * KPAD + a] * zh[b];
        zh[a] = v / Vc[a * KPAD + a];
        ss += zh[a] * zh[a];
    }
    return -((double)d * PF_LOG2PI + logdet[p]) / 2.0 - ss / 2.0;
}
