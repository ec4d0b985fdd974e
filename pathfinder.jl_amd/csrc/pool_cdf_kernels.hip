// pool_cdf_kernels.hip -- weighted empirical CDF of the pool at given thresholds, per coordinate (pfmi_pool_cdf; the quantities are
// defined in include/pfmi.h).
//
// One pass over the pool whatever the number of thresholds: every thread keeps, for each of its rows, NT thresholds and three
// accumulators per threshold (weight at or below, largest value at or below, smallest value above) in registers, and an element costs
// two compares, three selects of a double, one add, one max and one min per threshold.  The cut of a run into workgroups is the moments kernel's
// (pool_geometry.h): NS column slots per workgroup, chunks of L columns, slots combined through LDS in slot order, chunks and runs
// added in order by pf_pool_cdf_combine_kernel.  No atomics.
// The thread layout and the column walk are the ones stated in pool_geometry.h, with two choices of this file: the 4 waves are NS slots
// x 4 / NS row waves whatever V is (the row tiling is free: the order in which a row's terms are added is fixed by (NS, L) alone), and
// a lane holds two rows (V = 2) only when NT <= CDF_NT_PAIRED: two rows of more thresholds do not fit the register file at more than
// one wave per SIMD.
// Instantiations: NT = 4, 8, 16 thresholds per thread; nthr is padded up with +inf thresholds whose results are never written.  32
// thresholds with their accumulators exceed the 256 VGPRs a thread can address, so above 16 the workgroup is doubled (TS = 2): its
// second 4 waves repeat the first 4 waves' loads and own thresholds 16 to 31: the pool still leaves HBM once, but a CU loads every
// element twice (from the cache the second time).
//
// Ordering rule: NS and L come from mom_geometry(d, N_r, CDF_WG_PER_RUN), a function of (d, N_r) alone, so a run's weight sums have
// the same bits on whichever context owns the run, whatever nthr is.  A chunk's partial results are 3 nthr d doubles per run, so the
// chunks are longer than the moments' (CDF_WG_PER_RUN): at L = 250 and nthr = 32 they are 3 * 32 / 250 of the pool's bytes.
#include "pfmi_common.h"
#include "pool_geometry.h"

#define CDF_WG_PER_RUN 4            // row tiles x chunks aimed at per run
#define CDF_NT_PAIRED 8             // most thresholds per thread at which a lane still holds two rows

// partial results of one (row tile, chunk, run): part[(((k C + c) 3 + q) nthr + j) d + i], q = 0: wle, 1: below, 2: above;
// pnan[(k C + c) d + i]
template <int V, int NT, int TS>
__global__ __launch_bounds__(MOM_THREADS * TS) void pf_pool_cdf_kernel(int d, int64_t N_r, int64_t L, int G, int NS, int nthr,
                                                                  const double *__restrict__ pool, const double *__restrict__ wts,
                                                                  const double *__restrict__ thr, double *__restrict__ part,
                                                                  int32_t *__restrict__ pnan) {
    __shared__ __attribute__((aligned(16))) double red_all[TS * 3 * MOM_THREADS * V];   // per threshold group: [q][slot][row of the tile]
    __shared__ int32_t nred[MOM_THREADS * V];                                  // [row of the tile]: a counted NaN in any slot
    const int tid = threadIdx.x % MOM_THREADS;
    const int joff = (threadIdx.x / MOM_THREADS) * NT;             // this thread's thresholds: joff + [0, NT)
    const int jmax = nthr < NT ? nthr : NT;                        // (uniform over the workgroup)
    double *red = red_all + (threadIdx.x / MOM_THREADS) * 3 * MOM_THREADS * V;
    const int k = blockIdx.z;
    const int64_t C = gridDim.y, n0 = (int64_t)blockIdx.y * L, n1 = (n0 + L < N_r) ? n0 + L : N_r;
    const double inf = __builtin_huge_val();
    const PoolLane p = pool_lane<V>(d, G, NS);
    const int slot = p.slot, rloc = p.rloc, rows_per_wg = p.rows_per_wg, row = p.row;
    const bool active = p.active;
    double T[NT][V], wle[NT][V], below[NT][V], above[NT][V];
    int32_t nan[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        nan[v] = 0;
        nred[tid * V + v] = 0;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            T[j][v] = (active && joff + j < nthr) ? thr[(size_t)(joff + j) * d + row + v] : inf;
            wle[j][v] = 0.0;
            below[j][v] = -inf;
            above[j][v] = inf;
        }
    }
    if (active) {
        pool_walk<V>(pool + (size_t)k * N_r * d + row, wts ? wts + (size_t)k * N_r : nullptr, d, n0 + slot, n1, NS,
                     [&](const double (&x)[V], double w, bool on) {
#pragma unroll
                         for (int v = 0; v < V; ++v) {
                             nan[v] |= (on && x[v] != x[v]) ? 1 : 0;
                             // a skipped column becomes a NaN here, once per element: like a counted NaN it compares false on both sides
                             const double xv = on ? x[v] : __builtin_nan("");
#pragma unroll
                             for (int j = 0; j < NT; ++j) {
                                 const bool le = xv <= T[j][v], gt = xv > T[j][v];
                                 wle[j][v] += le ? w : 0.0;
                                 below[j][v] = fmax(below[j][v], le ? xv : -inf);
                                 above[j][v] = fmin(above[j][v], gt ? xv : inf);
                             }
                         }
                     });
    }
    if (NS > 1) {                      // slots in slot order, one threshold at a time (3 NT sets of a tile's slots exceed the LDS)
        __syncthreads();
        if (active) {
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (nan[v]) nred[rloc + v] = 1;                     // (every writer stores the same 1)
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (j < jmax) {            // (uniform)
                if (active && slot > 0) {
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        red[(0 * NS + slot) * rows_per_wg + rloc + v] = wle[j][v];
                        red[(1 * NS + slot) * rows_per_wg + rloc + v] = below[j][v];
                        red[(2 * NS + slot) * rows_per_wg + rloc + v] = above[j][v];
                    }
                }
                __syncthreads();
                if (active && slot == 0) {
                    for (int s = 1; s < NS; ++s) {
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            wle[j][v] += red[(0 * NS + s) * rows_per_wg + rloc + v];
                            below[j][v] = fmax(below[j][v], red[(1 * NS + s) * rows_per_wg + rloc + v]);
                            above[j][v] = fmin(above[j][v], red[(2 * NS + s) * rows_per_wg + rloc + v]);
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (active && slot == 0) {
#pragma unroll
            for (int v = 0; v < V; ++v) nan[v] = nred[rloc + v];
        }
    }
    if (active && slot == 0) {
        const size_t kc = (size_t)k * C + blockIdx.y, plane = (size_t)nthr * d;
        double *o = part + kc * 3 * plane + row;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (joff + j < nthr) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    o[(size_t)(joff + j) * d + v] = wle[j][v];
                    o[plane + (size_t)(joff + j) * d + v] = below[j][v];
                    o[2 * plane + (size_t)(joff + j) * d + v] = above[j][v];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (joff == 0) pnan[kc * d + row + v] = nan[v];
    }
}

// per (j, i): wle = ((carry + run 0) + run 1) + ..., a run being its chunks added in chunk order; below / above: max / min over all
// chunks; nanflag[i]: any chunk.  out = [wle nthr d][below nthr d][above nthr d], onan = [d]
__global__ void pf_pool_cdf_combine_kernel(int d, int K, int64_t C, int nthr, const double *__restrict__ part,
                                           const int32_t *__restrict__ pnan, const double *__restrict__ carry, double *__restrict__ out,
                                           int32_t *__restrict__ onan) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= d) return;
    const size_t plane = (size_t)nthr * d, e = (size_t)j * d + i;
    double acc = carry ? carry[e] : 0.0, lo = -__builtin_huge_val(), hi = __builtin_huge_val();
    int32_t bad = 0;
    for (int k = 0; k < K; ++k) {
        double run = 0.0;
        for (int64_t ch = 0; ch < C; ++ch) {
            const size_t kc = (size_t)k * C + ch;
            const double *p = part + kc * 3 * plane + e;
            run = ch == 0 ? p[0] : run + p[0];
            lo = fmax(lo, p[plane]);
            hi = fmin(hi, p[2 * plane]);
            if (j == 0) bad |= pnan[kc * d + i];
        }
        acc += run;
    }
    out[e] = acc;
    out[plane + e] = lo;
    out[2 * plane + e] = hi;
    if (j == 0) onan[i] = bad;
}

template <int V, int NT, int TS>
static void cdf_launch(pfmi_ctx *c, const MomGeom &g, int nthr, const double *wts, const double *thr, double *part, int32_t *pnan) {
    const int d = c->d;
    const int rows_per_wg = g.G ? d : (MOM_WAVES / g.NS) * 64 * V;
    const dim3 grid((unsigned)((d + rows_per_wg - 1) / rows_per_wg), (unsigned)g.C, (unsigned)c->K);
    hipLaunchKernelGGL((pf_pool_cdf_kernel<V, NT, TS>), grid, dim3(MOM_THREADS * TS), 0, c->stream, d, c->N_r, g.L, g.G, g.NS, nthr,
                       c->pool.as<double>(), wts, thr, part, pnan);
}

// c->pcdf = [wle nthr d][below nthr d][above nthr d][nanflag d (int32)] of the ctx's pool at the thresholds d_thr (device, nthr d);
// d_carry: device, nthr d doubles or NULL
int32_t pf_launch_pool_cdf(pfmi_ctx *c, int64_t col_offset, int importance, int nthr, const double *d_thr, const double *d_carry) {
    const int K = c->K, d = c->d;
    const MomGeom g = mom_geometry(d, c->N_r, CDF_WG_PER_RUN);
    PF_CHECK(mom_grid_fits(K, g), PFMI_ERR_ARG, "pool_cdf: too many runs for one launch");
    const size_t plane = (size_t)nthr * d, kc = (size_t)K * g.C;
    PF_TRY(c->pcdf.ensure(sizeof(double) * 3 * plane + sizeof(int32_t) * d));
    PF_TRY(c->pcdf_part.ensure(sizeof(double) * kc * 3 * plane + sizeof(int32_t) * kc * d));
    double *part = c->pcdf_part.as<double>(), *out = c->pcdf.as<double>();
    int32_t *pnan = reinterpret_cast<int32_t *>(part + kc * 3 * plane), *onan = reinterpret_cast<int32_t *>(out + 3 * plane);
    const double *wts = pf_pool_weights(c, col_offset, importance);
    const bool paired = g.G == 0 && g.V == 2 && nthr <= CDF_NT_PAIRED;
    pf_kernel_begin(c);
    if (nthr <= 4) {
        if (paired) cdf_launch<2, 4, 1>(c, g, nthr, wts, d_thr, part, pnan);
        else cdf_launch<1, 4, 1>(c, g, nthr, wts, d_thr, part, pnan);
    } else if (nthr <= 8) {
        if (paired) cdf_launch<2, 8, 1>(c, g, nthr, wts, d_thr, part, pnan);
        else cdf_launch<1, 8, 1>(c, g, nthr, wts, d_thr, part, pnan);
    } else if (nthr <= 16) {
        cdf_launch<1, 16, 1>(c, g, nthr, wts, d_thr, part, pnan);
    } else {
        cdf_launch<1, 16, 2>(c, g, nthr, wts, d_thr, part, pnan);
    }
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "pool_cdf");
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_pool_cdf_combine_kernel, dim3((unsigned)((d + 255) / 256), (unsigned)nthr), dim3(256), 0, c->stream, d, K, g.C,
                       nthr, part, pnan, d_carry, out, onan);
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "pool_cdf_combine");
    return PFMI_OK;
}
