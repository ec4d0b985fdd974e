// pool_transform_kernels.hip -- one affine map for every column of the pool, and the built-in target at the moved columns
// (pfmi_pool_transform; the pass of importance-weighted moment matching).
//
// For every column s of the pool AS BUILT x0 (d x (K N_r), column-major) and row i:
//   x1[i][s] = fma(scale[i], x0[i][s], shift[i]),     lp[s] = logp(x1[:, s])   (built-in targets; closures run afterwards on x1)
// then pf_pool_transform_ratio_kernel: lq1 = lq0 - sum log scale, lr1 = lp1 - lq1 and, with mixture ratios, lr_mix1 = lp1 - (lmix0 - sum log scale).
//
// One pass, bound by HBM: every element of x0 is read once and every element of x1 written once.
//   d >= 64   a WAVE owns a column: lanes run along rows (row = (64 t + lane) V, the layout of pool_geometry.h with every wave a row
//             wave), so a load or store of the wave is 64 V consecutive doubles; V = 2 (16-byte accesses) for even d >= 128, where
//             every column starts 16-byte aligned (the rank-16 Gaussian family keeps V = 1, see pt_launch).  A wave carries PT_CB
//             columns through one walk over the rows: the row's coefficients (scale, shift, mean, a and the RPAD doubles of Wd)
//             are loaded once per PT_CB columns, which keeps the low-rank operand's L2 traffic at the order of the pool's own.
//             The lanes' partial sums are added on the DPP path (pf_wave_sum).
//   d <  64   a LANE owns a column and walks its rows in order; the 64 columns of a wave are one span of 512 d bytes, so every line
//             fetched or written is used in full, and the row's coefficients are wave-uniform (scalar loads).
//
// Ordering rule: for a given target the terms of a column's logp are added in an order that is a function of d ALONE (d >= 64:
// lane l adds its rows (64 t + l) V, + 1 in row order, then the fixed DPP tree; d < 64: rows in order) -- never of K, N_r, the column's position, the
// columns it shares a wave with, the grid or the device.  A run's numbers have the same bits on whichever context owns it.
#include "pfmi_common.h"
#include "pool_geometry.h"

#define PT_THREADS 256
#define PT_CB 4                 // columns per wave and walk (d >= 64)

struct PtTarget {
    const double *mean, *a, *wd /* [d][RPAD] row-major */, *g /* [RPAD][RPAD] row-major, lower */;
    double offset;
};

// TGT: 0 none (a closure evaluates afterwards), 1 Gaussian family with RPAD low-rank columns, 2 funnel -- the sums of one column (or
// one lane's share of them) and what logp is of the complete sums: the formulas of TargetAcc (elbo_kernels.hip)
template <int TGT, int RPAD>
struct PtAcc {
    double q, tau, tr[RPAD > 0 ? RPAD : 1];
    __device__ __forceinline__ void init() {
        q = 0.0; tau = 0.0;
#pragma unroll
        for (int j = 0; j < (RPAD > 0 ? RPAD : 1); ++j) tr[j] = 0.0;
    }
    // row i of the column: x its moved value; mean_i, a_i, wr[RPAD]: the row's target coefficients (read for TGT == 1 only)
    __device__ __forceinline__ void row(int i, double x, double mean_i, double a_i, const double *wr) {
        if (TGT == 1) {
            const double e = x - mean_i;
            q += a_i * e * e;
#pragma unroll
            for (int j = 0; j < RPAD; ++j) tr[j] += wr[j] * e;
        } else if (TGT == 2) {
            if (i == 0) tau = x; else q += x * x;
        }
    }
    __device__ __forceinline__ double finish(const PtTarget &T, int d) const {
        if (TGT == 1) {
            double corr = 0.0;
#pragma unroll
            for (int j = 0; j < RPAD; ++j) {
                double g = 0.0;
#pragma unroll
                for (int l = 0; l <= j; ++l) g += T.g[j * RPAD + l] * tr[l];
                corr += g * g;
            }
            return T.offset - 0.5 * (q - corr);
        } else if (TGT == 2) {
            const double t3 = tau / 3.0;
            return (t3 * t3 + (double)(d - 1) * tau + q * exp(-tau)) / -2.0;
        }
        return NAN;
    }
};

// d >= 64: grid-stride over groups of PT_CB columns, one group per wave and trip
template <int TGT, int RPAD, int V>
__global__ __launch_bounds__(PT_THREADS) void pf_pool_transform_rows_kernel(int d, int64_t S, const double *__restrict__ x0,
                                                                            const double *__restrict__ scale,
                                                                            const double *__restrict__ shift, double *__restrict__ x1,
                                                                            double *__restrict__ lp, PtTarget T) {
    constexpr int RP = RPAD > 0 ? RPAD : 1;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (PT_THREADS / 64), ngroups = (S + PT_CB - 1) / PT_CB;
    for (int64_t grp = (int64_t)blockIdx.x * (PT_THREADS / 64) + (threadIdx.x >> 6); grp < ngroups; grp += nwaves) {
        const int64_t s0 = grp * PT_CB;
        bool on[PT_CB];
        size_t base[PT_CB];
#pragma unroll
        for (int c = 0; c < PT_CB; ++c) {
            on[c] = s0 + c < S;
            base[c] = (size_t)(on[c] ? s0 + c : s0) * (size_t)d;        // (clamped: an in-range column, never stored)
        }
        PtAcc<TGT, RPAD> acc[PT_CB];
#pragma unroll
        for (int c = 0; c < PT_CB; ++c) acc[c].init();
        for (int r = lane * V; r < d; r += 64 * V) {                    // (V = 2: d is even, so row r + 1 is inside too)
            double x[PT_CB][V], sc[V], sh[V], mean[V], a[V], wr[V][RP];
#pragma unroll
            for (int c = 0; c < PT_CB; ++c) {                           // the pool's loads are issued first
                if constexpr (V == 2) {
                    const double2 t = *reinterpret_cast<const double2 *>(x0 + base[c] + r);
                    x[c][0] = t.x; x[c][V - 1] = t.y;
                } else {
                    x[c][0] = x0[base[c] + r];
                }
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                sc[v] = scale[r + v]; sh[v] = shift[r + v];
                mean[v] = a[v] = 0.0;
                if (TGT == 1) {
                    mean[v] = T.mean[r + v]; a[v] = T.a[r + v];
#pragma unroll
                    for (int j = 0; j < RPAD; ++j) wr[v][j] = T.wd[(size_t)(r + v) * RPAD + j];
                }
            }
#pragma unroll
            for (int c = 0; c < PT_CB; ++c) {
                double y[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    y[v] = fma(sc[v], x[c][v], sh[v]);
                    acc[c].row(r + v, y[v], mean[v], a[v], wr[v]);
                }
                if (on[c]) {
                    if constexpr (V == 2) *reinterpret_cast<double2 *>(x1 + base[c] + r) = make_double2(y[0], y[V - 1]);
                    else x1[base[c] + r] = y[0];
                }
            }
        }
        if (TGT != 0) {                                                 // every lane of the wave is here: the DPP tree sees all 64
#pragma unroll
            for (int c = 0; c < PT_CB; ++c) {
                acc[c].q = pf_wave_sum(acc[c].q);
                if (TGT == 2) acc[c].tau = pf_readlane_f64(acc[c].tau, 0);      // row 0 is lane 0's
#pragma unroll
                for (int j = 0; j < RPAD; ++j) acc[c].tr[j] = pf_wave_sum(acc[c].tr[j]);
                const double v = acc[c].finish(T, d);
                if (lane == 0 && on[c]) lp[s0 + c] = v;
            }
        }
    }
}

// d < 64: one column per lane, grid-stride
template <int TGT, int RPAD>
__global__ __launch_bounds__(PT_THREADS) void pf_pool_transform_cols_kernel(int d, int64_t S, const double *__restrict__ x0,
                                                                            const double *__restrict__ scale,
                                                                            const double *__restrict__ shift, double *__restrict__ x1,
                                                                            double *__restrict__ lp, PtTarget T) {
    const int64_t stride = (int64_t)gridDim.x * PT_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x; s < S; s += stride) {
        const double *xi = x0 + (size_t)s * d;
        double *xo = x1 + (size_t)s * d;
        PtAcc<TGT, RPAD> acc;
        acc.init();
        for (int i = 0; i < d; ++i) {
            const double y = fma(scale[i], xi[i], shift[i]);
            xo[i] = y;
            acc.row(i, y, TGT == 1 ? T.mean[i] : 0.0, TGT == 1 ? T.a[i] : 0.0, TGT == 1 && RPAD > 0 ? T.wd + (size_t)i * RPAD : nullptr);
        }
        if (TGT != 0) lp[s] = acc.finish(T, d);
    }
}

// the densities of the moved pool from those of the pool as built.  sla = sum_i log scale_i (formed once on the host, in index
// order).  A column whose proposal density is NaN (its fit failed: the pool holds no draw there) keeps logp = NaN.
__global__ void pf_pool_transform_ratio_kernel(int64_t n, double sla, const double *__restrict__ lq0, const double *__restrict__ lmix0,
                                               double *__restrict__ lp, double *__restrict__ lq, double *__restrict__ lr,
                                               double *__restrict__ lr_mix) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double q0 = lq0[i];
    double p = lp[i];
    if (q0 != q0) { p = NAN; lp[i] = p; }
    const double q = q0 - sla;
    lq[i] = q;
    lr[i] = p - q;
    if (lmix0) lr_mix[i] = p - (lmix0[i] - sla);
}

template <int TGT, int RPAD>
static void pt_launch(pfmi_ctx *c, int d, int64_t S, const double *x0, const double *scale, const double *shift, double *x1, double *lp,
                      const PtTarget &T) {
    const int ncu = c->ncu > 0 ? c->ncu : 256;
    if (d < 64) {
        int64_t nb = (S + PT_THREADS - 1) / PT_THREADS;
        if (nb > 8 * (int64_t)ncu) nb = 8 * (int64_t)ncu;
        hipLaunchKernelGGL((pf_pool_transform_cols_kernel<TGT, RPAD>), dim3((unsigned)nb), dim3(PT_THREADS), 0, c->stream, d, S, x0, scale,
                           shift, x1, lp, T);
        return;
    }
    const int64_t ngroups = (S + PT_CB - 1) / PT_CB;
    int64_t nb = (ngroups + PT_THREADS / 64 - 1) / (PT_THREADS / 64);
    if (nb > 8 * (int64_t)ncu) nb = 8 * (int64_t)ncu;
    // the V of mom_geometry; the rank-16 family stays at V = 1: its 68 accumulators and two rows of Wd would take the wave past 256
    // registers and with that to one wave per SIMD
    if constexpr (RPAD < 16) {
        if (d % 2 == 0 && d >= 128) {
            hipLaunchKernelGGL((pf_pool_transform_rows_kernel<TGT, RPAD, 2>), dim3((unsigned)nb), dim3(PT_THREADS), 0, c->stream, d, S, x0,
                               scale, shift, x1, lp, T);
            return;
        }
    }
    hipLaunchKernelGGL((pf_pool_transform_rows_kernel<TGT, RPAD, 1>), dim3((unsigned)nb), dim3(PT_THREADS), 0, c->stream, d, S, x0, scale,
                       shift, x1, lp, T);
}

// x1 = scale .* x0 + shift over the ctx's K N_r columns and, for a built-in target, lp = logp(x1); d_scale, d_shift: d doubles on the device
int32_t pf_launch_pool_transform(pfmi_ctx *c, const double *x0, const double *d_scale, const double *d_shift, double *x1, double *lp) {
    const int d = c->d;
    const int64_t S = (int64_t)c->K * c->N_r;
    if (S <= 0) return PFMI_OK;
    const TargetDev &t = c->target;
    PtTarget T{t.mean.as<double>(), t.a.as<double>(), t.wd.as<double>(), t.g.as<double>(), t.offset};
    PF_CHECK(t.kind != PFMI_TARGET_GAUSS || t.rpad == 0 || t.rpad == 8 || t.rpad == 16, PFMI_ERR_UNSUPPORTED,
             "pool_transform: unsupported target padding %d", t.rpad);
    pf_kernel_begin(c);
    if (t.kind == PFMI_TARGET_GAUSS) {
        if (t.rpad == 0) pt_launch<1, 0>(c, d, S, x0, d_scale, d_shift, x1, lp, T);
        else if (t.rpad == 8) pt_launch<1, 8>(c, d, S, x0, d_scale, d_shift, x1, lp, T);
        else pt_launch<1, 16>(c, d, S, x0, d_scale, d_shift, x1, lp, T);
    } else if (t.kind == PFMI_TARGET_FUNNEL) {
        pt_launch<2, 0>(c, d, S, x0, d_scale, d_shift, x1, lp, T);
    } else {
        pt_launch<0, 0>(c, d, S, x0, d_scale, d_shift, x1, lp, T);
    }
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "pool_transform");
    return PFMI_OK;
}

int32_t pf_launch_pool_transform_ratio(pfmi_ctx *c, double sla, const double *lq0, const double *lmix0, double *lp, double *lq, double *lr,
                                       double *lr_mix) {
    const int64_t S = (int64_t)c->K * c->N_r;
    if (S <= 0) return PFMI_OK;
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_pool_transform_ratio_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, c->stream, S, sla, lq0, lmix0, lp,
                       lq, lr, lr_mix);
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "pool_transform_ratio");
    return PFMI_OK;
}
