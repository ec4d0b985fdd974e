// hmc_target.h -- log density and gradient of the built-in targets inside a chain kernel (hmc_fused_kernel.hip): one workgroup of HM_NT
// threads evaluates its chain's trial point.  lb_eval's formulas (lbfgs_kernels.hip) with the sign of logp, those of GaussTarget /
// FunnelTarget.logp_and_grad (pfmi/targets.py).
//
// Row ownership is that of the operator passes (hmc_rows.h): thread tid owns rows tid, tid + HM_NT, ...  ONE fixed-order block reduction
// (pf_block_sum_mv: six butterfly steps in a wave, then the four waves' partials in wave order), read back by every thread, so every
// thread holds the same bits of every sum; everything after it is row-local: a thread writes g only at rows it owns.
//
//   Gaussian family (TG = rank padding 0, 8, 16; e = x - mean):
//       qa = sum_i a_i e_i^2,  we_j = sum_i Wd[i][j] e_i                          (the reduction: TG + 1 values, padded to TG + 4)
//       gg = G we (G lower triangular, row j: terms l = 0 .. j in that order),  corr = sum_j gg_j^2 (j ascending),
//       h = G'gg (entry l: terms j = l .. TG - 1 in that order)                   (every thread, redundantly, from G's copy in LDS)
//       lp = offset - (qa - corr) / 2,   g_i = -(a_i e_i - sum_j Wd[i][j] h_j)    (j ascending, fused multiply-adds)
//   Funnel (TG = HM_TG_FUNNEL; tau = x_0, ss = sum_{i >= 1} x_i^2):
//       lp = -((tau / 3)^2 + (d - 1) tau + e^-tau ss) / 2,  g_0 = -(2 tau / 9 + (d - 1) - e^-tau ss) / 2,  g_i = -e^-tau x_i
//
// A non-finite coordinate makes lp or an entry of g non-finite: hm_apply_R counts those, the step treats them as the closure's.
#pragma once
#include "hmc_rows.h"

#define HM_TG_NONE (-2)                // no built-in target: a step kernel, which reads a closure's output
#define HM_TG_FUNNEL (-1)

// what the evaluation reads of the target (TargetDev, pfmi_common.h): mean, a [d], Wd [d][rpad] row-major, G [rpad][rpad] row-major lower
struct HmTarget {
    const double *mean, *a, *wd, *gm;
    double offset;
};

// values of the evaluation's reduction (a multiple of 4), and the doubles of G's copy in LDS
template <int TG> struct HmTargetShape {
    static constexpr int NV = TG > 0 ? TG + 4 : 4;
    static constexpr int NG = TG > 0 ? TG * TG : 1;
};

// the step's static LDS (HmLds, hmc_rows.h) with G's copy behind it
template <int KPAD, int NRED, int TG>
struct HmTargetLds : HmLds<KPAD, NRED> {
    alignas(16) double sG[HmTargetShape<TG>::NG];
};

#ifdef __HIPCC__
// G into the kernel's LDS copy, once per launch (the caller's next barrier -- every reduction has one -- publishes it)
template <int TG, class Lds>
__device__ __forceinline__ void hm_target_stage(const HmTarget &Tg, Lds &L) {
    if constexpr (TG > 0)
        for (int i = threadIdx.x; i < TG * TG; i += HM_NT) L.sG[i] = Tg.gm[i];
}

// logp at X [d], its gradient into g [d] (each thread: its own rows); returns logp, the same bits in every thread.  Lds: the kernel's
// one object (red: the ping-pong reduction buffers for NRED values, sG: hm_target_stage's copy).
template <int TG, int NRED, class Lds>
__device__ __forceinline__ double hm_target_eval(const HmTarget &Tg, Lds &L, const double *X, double *g, int d, int &flip) {
    constexpr int NV = HmTargetShape<TG>::NV;
    static_assert(NV <= NRED, "the kernel's reduction buffers hold the evaluation's sums");
    const int tid = threadIdx.x;
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0;
    if constexpr (TG == HM_TG_FUNNEL) {
        for (int i = tid; i < d; i += HM_NT) {
            const double xi = X[i];
            if (i == 0) v[1] = xi; else v[0] = fma(xi, xi, v[0]);
        }
        pf_block_sum_mv<NV, NRED>(v, L.red, flip);
        const double ss = v[0], tau = v[1], ee = exp(-tau), dm1 = (double)(d - 1), es = ee * ss;
        const double lp = -0.5 * ((tau / 3.0) * (tau / 3.0) + dm1 * tau + es);
        const double g0 = -0.5 * (2.0 * tau / 9.0 + dm1 - es);
        for (int i = tid; i < d; i += HM_NT) g[i] = i == 0 ? g0 : -(ee * X[i]);
        return lp;
    } else {
        constexpr int R = TG > 0 ? TG : 1;
        for (int i = tid; i < d; i += HM_NT) {
            const double e = X[i] - Tg.mean[i], ae = Tg.a[i] * e;
            v[TG] = fma(ae, e, v[TG]);
            if constexpr (TG > 0) {
                const double *row = Tg.wd + (size_t)i * TG;
#pragma unroll
                for (int c = 0; c < TG; c += 4) {
                    const double4 r = *reinterpret_cast<const double4 *>(row + c);
                    v[c] = fma(r.x, e, v[c]); v[c + 1] = fma(r.y, e, v[c + 1]); v[c + 2] = fma(r.z, e, v[c + 2]); v[c + 3] = fma(r.w, e, v[c + 3]);
                }
            }
        }
        pf_block_sum_mv<NV, NRED>(v, L.red, flip);
        const double qa = v[TG];
        double corr = 0.0;
        [[maybe_unused]] double h[R];
        if constexpr (TG > 0) {
            double gg[R];
#pragma unroll
            for (int j = 0; j < TG; ++j) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l <= j; ++l) s = fma(L.sG[j * TG + l], v[l], s);
                gg[j] = s;
                corr = fma(s, s, corr);
            }
#pragma unroll
            for (int l = 0; l < TG; ++l) {
                double s = 0.0;
#pragma unroll
                for (int j = l; j < TG; ++j) s = fma(L.sG[j * TG + l], gg[j], s);
                h[l] = s;
            }
        }
        for (int i = tid; i < d; i += HM_NT) {
            double gv = Tg.a[i] * (X[i] - Tg.mean[i]);
            if constexpr (TG > 0) {
                const double *row = Tg.wd + (size_t)i * TG;
#pragma unroll
                for (int c = 0; c < TG; c += 4) {
                    const double4 r = *reinterpret_cast<const double4 *>(row + c);
                    gv = fma(-r.x, h[c], gv); gv = fma(-r.y, h[c + 1], gv); gv = fma(-r.z, h[c + 2], gv); gv = fma(-r.w, h[c + 3], gv);
                }
            }
            g[i] = -gv;
        }
        return Tg.offset - 0.5 * (qa - corr);
    }
}
#endif
