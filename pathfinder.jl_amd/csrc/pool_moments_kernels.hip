// pool_moments_kernels.hip -- weighted first and second moments of the pool, per run and coordinate (pfmi_pool_moments).
//
// For every local run k and row i of the pool (d x (K N_r), column-major, one column per draw), with t = x_i - center_i:
//   s1[k][i] = sum_n w t,  s2[k][i] = sum_n w t^2,  s2w[k][i] = sum_n w^2 t^2,  wsum[k] = (sum_n w, sum_n w^2)
// w = weights[col_offset + k N_r + n] (the ctx's PSIS weights of the GLOBAL pool), or 1 without importance weighting.  A column whose
// weight is exactly 0 is skipped by a select (never 0 * NaN); without importance weighting nothing is skipped.
//
// One pass over the pool, bound by HBM, in the cut, thread layout and column walk of pool_geometry.h (stated there once).  The slots'
// sums are combined through LDS in slot order and written as the chunk's partial; pf_pool_moments_sum_kernel adds the chunks in chunk
// order.  No atomics.
//
// Ordering rule: the geometry (V, RW, NS, chunk length) is a function of (d, N_r) ALONE -- never of K, col_offset, the run's position or
// the device -- so the sums of one run are formed in the same order, and have the same bits, on whichever context owns the run.
#include "pfmi_common.h"
#include "pool_geometry.h"

// partial sums of one (row tile, chunk, run): part[((k C + c) 3 + q) d + i], q = 0: s1, 1: s2, 2: s2w; pw[(k C + c) 2 + j]
template <int V>
__global__ __launch_bounds__(MOM_THREADS) void pf_pool_moments_kernel(int d, int64_t N_r, int64_t L, int G, int NS,
                                                                      const double *__restrict__ pool, const double *__restrict__ wts,
                                                                      const double *__restrict__ center, double *__restrict__ part,
                                                                      double *__restrict__ pw) {
    __shared__ __attribute__((aligned(16))) double red[3 * MOM_THREADS * V];   // [q][slot][row of the tile]
    __shared__ double wred[2 * MOM_THREADS];                                   // [slot][2]: the slots' sums of w and w^2
    const int tid = threadIdx.x, k = blockIdx.z;
    const int64_t C = gridDim.y, n0 = (int64_t)blockIdx.y * L, n1 = (n0 + L < N_r) ? n0 + L : N_r;
    const PoolLane p = pool_lane<V>(d, G, NS);
    const int slot = p.slot, rloc = p.rloc, rows_per_wg = p.rows_per_wg, row = p.row;
    const bool active = p.active;
    double s1[V], s2[V], s2w[V], sw = 0.0, sw2 = 0.0, cen[V];
#pragma unroll
    for (int v = 0; v < V; ++v) s1[v] = s2[v] = s2w[v] = cen[v] = 0.0;
    if (active) {
        if (center) {
#pragma unroll
            for (int v = 0; v < V; ++v) cen[v] = center[row + v];
        }
        pool_walk<V>(pool + (size_t)k * N_r * d + row, wts ? wts + (size_t)k * N_r : nullptr, d, n0 + slot, n1, NS,
                     [&](const double (&x)[V], double w, bool on) {
                         const double wu = on ? w : 0.0;
                         sw += wu;
                         sw2 += wu * wu;
#pragma unroll
                         for (int v = 0; v < V; ++v) {
                             const double t = x[v] - cen[v];
                             const double a = w * t;
                             s1[v] += on ? a : 0.0;
                             s2[v] += on ? a * t : 0.0;
                             s2w[v] += on ? a * a : 0.0;
                         }
                     });
        if (slot > 0) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                red[(0 * NS + slot) * rows_per_wg + rloc + v] = s1[v];
                red[(1 * NS + slot) * rows_per_wg + rloc + v] = s2[v];
                red[(2 * NS + slot) * rows_per_wg + rloc + v] = s2w[v];
            }
        }
        if (rloc == 0) { wred[2 * slot] = sw; wred[2 * slot + 1] = sw2; }
    }
    __syncthreads();
    if (active && slot == 0) {         // slots in slot order
        for (int s = 1; s < NS; ++s) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                s1[v] += red[(0 * NS + s) * rows_per_wg + rloc + v];
                s2[v] += red[(1 * NS + s) * rows_per_wg + rloc + v];
                s2w[v] += red[(2 * NS + s) * rows_per_wg + rloc + v];
            }
        }
        double *o = part + ((size_t)k * C + blockIdx.y) * 3 * d + row;
#pragma unroll
        for (int v = 0; v < V; ++v) { o[v] = s1[v]; o[(size_t)d + v] = s2[v]; o[2 * (size_t)d + v] = s2w[v]; }
    }
    if (blockIdx.x == 0 && tid < 2) {  // the chunk's sums of w and w^2: row tile 0 only, slots in slot order
        double s = wred[tid];
        for (int t = 1; t < NS; ++t) s += wred[2 * t + tid];
        pw[((size_t)k * C + blockIdx.y) * 2 + tid] = s;
    }
}

// chunks in chunk order: out = [wsum K 2][s1 K d][s2 K d][s2w K d]
__global__ void pf_pool_moments_sum_kernel(int d, int K, int64_t C, const double *__restrict__ part, const double *__restrict__ pw,
                                           double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i < d) {
        const double *p = part + (size_t)k * C * 3 * d + i;
        double a = p[0], b = p[(size_t)d], c = p[2 * (size_t)d];
        for (int64_t ch = 1; ch < C; ++ch) {
            const double *q = p + (size_t)ch * 3 * d;
            a += q[0]; b += q[(size_t)d]; c += q[2 * (size_t)d];
        }
        double *o = out + 2 * (size_t)K + (size_t)k * d + i;
        o[0] = a; o[(size_t)K * d] = b; o[2 * (size_t)K * d] = c;
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        const double *q = pw + (size_t)k * C * 2 + threadIdx.x;
        double s = q[0];
        for (int64_t ch = 1; ch < C; ++ch) s += q[2 * ch];
        out[2 * (size_t)k + threadIdx.x] = s;
    }
}

// c->mom = [wsum K 2][s1 K d][s2 K d][s2w K d] of the ctx's pool; d_center: d doubles on the device, or NULL
int32_t pf_launch_pool_moments(pfmi_ctx *c, int64_t col_offset, int importance, const double *d_center) {
    const int K = c->K, d = c->d;
    const int64_t N_r = c->N_r;
    const MomGeom g = mom_geometry(d, N_r);
    PF_CHECK(mom_grid_fits(K, g), PFMI_ERR_ARG, "pool_moments: too many runs for one launch");
    PF_TRY(c->mom.ensure(sizeof(double) * ((size_t)K * 2 + 3 * (size_t)K * d)));
    PF_TRY(c->mom_part.ensure(sizeof(double) * (size_t)K * g.C * (3 * (size_t)d + 2)));
    double *part = c->mom_part.as<double>(), *pw = part + (size_t)K * g.C * 3 * d;
    const double *wts = pf_pool_weights(c, col_offset, importance);
    const dim3 grid((unsigned)g.row_tiles, (unsigned)g.C, (unsigned)K);
    pf_kernel_begin(c);
    if (g.V == 2)
        hipLaunchKernelGGL(pf_pool_moments_kernel<2>, grid, dim3(MOM_THREADS), 0, c->stream, d, N_r, g.L, g.G, g.NS,
                           c->pool.as<double>(), wts, d_center, part, pw);
    else
        hipLaunchKernelGGL(pf_pool_moments_kernel<1>, grid, dim3(MOM_THREADS), 0, c->stream, d, N_r, g.L, g.G, g.NS,
                           c->pool.as<double>(), wts, d_center, part, pw);
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "pool_moments");
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_pool_moments_sum_kernel, dim3((unsigned)((d + 255) / 256), (unsigned)K), dim3(256), 0, c->stream, d, K, g.C,
                       part, pw, c->mom.as<double>());
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "pool_moments_sum");
    return PFMI_OK;
}
