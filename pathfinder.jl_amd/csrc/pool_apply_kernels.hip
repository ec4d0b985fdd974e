// pool_apply_kernels.hip -- the pooled weighted second moment applied to a thin block of vectors without being formed
// (pfmi_pool_apply; the quantities are defined in include/pfmi.h): two tall-skinny contractions over the pool on the f64 matrix cores.
//
// For the ctx's pool (d x (K N_r), column-major, one column per draw), r <= 32 directions v[j d + i], t_i(n) = fl(x_i(n) - center[i]):
//   scores   z_j(n)  = sum_i t_i(n) v[j d + i]                                        (0 for every j when the column is skipped)
//   apply    Y[j][i] = y_in[j d + i] + sum_runs k (in run order) sum_n fl(w t_i(n)) z_j(n)
// w and the zero-weight rule are those of every pass over the pool (pool_geometry.h: pf_pool_weights, pool_weight, pool_counts).  The
// d x d matrix sum (w t) t' costs d^2 S multiply-adds; Y costs 2 d r S and the pool streams through once per contraction.
//
// Both kernels use v_mfma_f64_16x16x4_f64 (A: lane (q = lane>>4, c = lane&15) holds A[row c][k = q]; B: B[k = q][column c]; C/D:
// register rr holds row q + 4 rr of column c).  The block of directions is padded with zero directions to RP = 16 RB, RB = 1 or 2.
//   pf_pool_scores_kernel<RB, V>   contracts over ROWS.  A workgroup (256 threads = 4 waves) owns 64 consecutive columns of the pool,
//             taken as one flat list of K N_r columns; a wave owns 16 of them and holds the RP x 16 scores as RB accumulators.  A = the
//             directions (16 of them x 4 rows), B = t (4 rows x 16 columns).  The workgroup walks d in chunks of 64 rows: the chunk of
//             its columns and of the directions is loaded with lanes along rows (V = 2, 16-byte loads, when d is even: the alignment
//             rule of pool_geometry.h), centred ONCE and written to LDS as [column][row] / [direction][row] with rows of 64 + 4 doubles
//             (the 16 columns x 4 rows a wave reads together fall on different banks).  The loads of chunk c + 1 are in flight while
//             the MFMAs of chunk c run.  Rows >= d are 0 in both operands; a skipped column is never read and its scores are written as
//             exact zeros.  Scores are stored as z[(k N_r + n) r + j].
//   pf_pool_apply_kernel<RB, V>    contracts over DRAWS: the cross kernel (pool_cross_kernels.hip) with its B slab taken from the scores.
//             A workgroup owns a tile of 64 rows of ONE run, a wave 16 of them x RP directions.  Per group of 4 columns A = w t (16
//             rows x 4 columns), B = z (4 columns x 16 directions).  The run is walked in chunks of NC columns staged as in the cross
//             kernel (LDS rows of 64 + 16 doubles); a run's last group of 4 is completed with zero columns in both operands.  The
//             tile of the run's sum goes to a partial buffer part[k][j d + i].
//   pf_pool_apply_combine_kernel   Y = y_in, then + part[0], + part[1], ... in run order, one thread per entry.
// Column splitting: the runs are the split -- grid (d / 64, K), 1024 workgroups at d = 1000, K = 64 -- and a run is not cut further, so
// a pool of few long runs keeps few workgroups busy (K = 1, d = 1000: 16).  profiles/pool_lowrank.md says what that costs.
//
// Guarantees (include/pfmi.h; tests/test_gpu_pool_apply.py holds the kernels to them):
//   - Independence of the block: an entry of D is one chain of MFMAs over A's row and B's column alone, and the padding directions
//     are zeros that are never written back, so z_j(n) and Y[j][.] have the same bits whatever r is and whatever the other directions hold.
//   - Ordering of scores: a score is ONE chain over the groups of 4 rows 0 .. d - 1 in order: it depends on its column, its direction,
//     center and d only -- not on K, N_r, col_offset, the run's position or the device.
//   - Ordering of apply (the contract of pfmi_pool_cross): no atomics; a run's sum is ONE chain, from zero, over the run's groups of 4
//     columns in order, so it depends on (d, N_r) only; the runs' sums are added in run order on top of y_in, which is added first.  So
//     contexts chained in run order through y_in return the bits of one context holding all the runs.
//   - A NaN anywhere in a column of weight exactly 0 is invisible (the column is not read).  A NaN in a counted column makes the
//     column's r scores NaN (NaN times a zero of v is NaN) and with them every entry of Y.
//   - 0 bytes of scratch and no spills in every instantiation (tests/test_pool_apply_cpu.py).
#include "pfmi_common.h"
#include "pool_geometry.h"       // pool_weight, pool_counts, pf_pool_weights

#define APPLY_THREADS 256
#define APPLY_T 64                  // rows of a chunk (scores) and of a row tile (apply)
#define APPLY_SCORE_COLS 64         // columns of a workgroup of the scores kernel
#define APPLY_SCORE_PAD 4           // doubles added to an LDS row of the scores kernel
#define APPLY_PAD 16                // doubles added to an LDS row of the apply kernel (CROSS_PAD)

typedef double apply_d4 __attribute__((ext_vector_type(4)));

template <int RB, int V>
__global__ __launch_bounds__(APPLY_THREADS) void pf_pool_scores_kernel(int d, int64_t S, int r, const double *__restrict__ pool,
                                                                       const double *__restrict__ wts, const double *__restrict__ center,
                                                                       const double *__restrict__ dirs, double *__restrict__ zs) {
    constexpr int RP = 16 * RB, T = APPLY_T, NC = APPLY_SCORE_COLS;
    constexpr int LR = T / V;                        // threads along the rows of one column
    constexpr int NSL = APPLY_THREADS / LR;          // columns loaded side by side
    constexpr int U = NC / NSL, UD = RP / NSL;       // columns, directions per thread and chunk
    constexpr int TS = T + APPLY_SCORE_PAD;
    __shared__ __attribute__((aligned(16))) double x_s[NC * TS], v_s[RP * TS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
    const int64_t s0 = (int64_t)blockIdx.x * NC;
    const bool imp = wts != nullptr;

    apply_d4 acc[RB];
#pragma unroll
    for (int a = 0; a < RB; ++a) acc[a] = apply_d4{0.0, 0.0, 0.0, 0.0};

    // staging: this thread's V rows of a chunk and its column slot; which of its columns count does not change with the chunk
    const int rloc = (tid % LR) * V, cslot = tid / LR;
    unsigned on = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t s = s0 + cslot + NSL * u;
        const bool use = s < S;
        const double w = pool_weight(imp, wts, use ? s : s0);
        if (pool_counts(imp, use, w)) on |= 1u << u;                // a zero weight skips the column whatever it holds
    }
    const double *col0 = pool + (size_t)(s0 + cslot) * d + rloc;    // column slot u, chunk row i0: col0 + NSL u d + i0
    const int NCH = (d + T - 1) / T;
    double x[U][V], dv[UD][V], cen[V];
    bool ok = false;
    auto load = [&](int ch) {
        const int i = ch * T + rloc;
        ok = i < d;                                                 // (V = 2: d is even, so the pair is inside too)
#pragma unroll
        for (int v = 0; v < V; ++v) cen[v] = (center && ok) ? center[i + v] : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int v = 0; v < V; ++v) x[u][v] = 0.0;
            if (ok && ((on >> u) & 1u)) {
                const double *p = col0 + (size_t)(NSL * u) * d + (size_t)ch * T;
                if constexpr (V == 2) { const double2 t = *reinterpret_cast<const double2 *>(p); x[u][0] = t.x; x[u][V - 1] = t.y; }
                else x[u][0] = p[0];
            }
        }
#pragma unroll
        for (int u = 0; u < UD; ++u) {
            const int j = cslot + NSL * u;
#pragma unroll
            for (int v = 0; v < V; ++v) dv[u][v] = 0.0;
            if (ok && j < r) {                                      // a ragged r: zero directions
                const double *p = dirs + (size_t)j * d + i;
                if constexpr (V == 2) { const double2 t = *reinterpret_cast<const double2 *>(p); dv[u][0] = t.x; dv[u][V - 1] = t.y; }
                else dv[u][0] = p[0];
            }
        }
    };
    load(0);
    for (int ch = 0; ch < NCH; ++ch) {
        __syncthreads();                                            // the previous chunk's operands have been read
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double *xp = x_s + (cslot + NSL * u) * TS + rloc;
#pragma unroll
            for (int v = 0; v < V; ++v) xp[v] = (ok && ((on >> u) & 1u)) ? x[u][v] - cen[v] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < UD; ++u) {
            double *vp = v_s + (cslot + NSL * u) * TS + rloc;
#pragma unroll
            for (int v = 0; v < V; ++v) vp[v] = dv[u][v];
        }
        __syncthreads();
        const int left = d - ch * T;
        const int ng = ((left < T ? left : T) + 3) / 4;             // groups of 4 rows of this chunk (uniform)
        if (ch + 1 < NCH) load(ch + 1);                             // in flight while the MFMAs run
        const double *xp = x_s + (16 * wv + c) * TS + q, *vp = v_s + c * TS + q;
        for (int g = 0; g < ng; ++g) {
            const double bv = xp[4 * g];
#pragma unroll
            for (int a = 0; a < RB; ++a) acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(vp[16 * a * TS + 4 * g], bv, acc[a], 0, 0, 0);
        }
    }
    const int64_t s = s0 + 16 * wv + c;
    if (s >= S) return;
    const double w = pool_weight(imp, wts, s);
    const bool counts = pool_counts(imp, true, w);
#pragma unroll
    for (int a = 0; a < RB; ++a)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int j = 16 * a + q + 4 * rr;
            if (j < r) zs[(size_t)s * r + j] = counts ? acc[a][rr] : 0.0;
        }
}

// grid (row tiles, K): the sum of run blockIdx.y over rows [64 blockIdx.x, + 64) into part[k][j d + i]
template <int RB, int V>
__global__ __launch_bounds__(APPLY_THREADS) void pf_pool_apply_kernel(int d, int64_t N_r, int r, const double *__restrict__ pool,
                                                                      const double *__restrict__ wts, const double *__restrict__ center,
                                                                      const double *__restrict__ zs, double *__restrict__ part) {
    constexpr int RP = 16 * RB, T = APPLY_T;
    constexpr int NC = RB == 1 ? 64 : 48;            // columns of a chunk (the chain of an entry does not depend on it)
    constexpr int LR = T / V, NSL = APPLY_THREADS / LR, U = NC / NSL;
    constexpr int TS = T + APPLY_PAD;
    constexpr int ZS = RB == 1 ? 16 : 48;            // LDS row of the scores: 16 (mod 32) doubles, as TS is
    constexpr int UZ = NC * RP / APPLY_THREADS;      // scores per thread and chunk
    __shared__ __attribute__((aligned(16))) double a_s[NC * TS], z_s[NC * ZS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
    const int i0 = blockIdx.x * T;
    const int64_t k = blockIdx.y;
    const bool imp = wts != nullptr;
    const double *run = pool + (size_t)k * N_r * d;                 // column n of the run: run + n d
    const double *wk = imp ? wts + (size_t)k * N_r : nullptr;
    const double *zk = zs + (size_t)k * N_r * r;                    // scores of column n: zk + n r

    apply_d4 acc[RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[b] = apply_d4{0.0, 0.0, 0.0, 0.0};

    const int rloc = (tid % LR) * V, cslot = tid / LR;
    const bool okA = i0 + rloc < d;                                 // (V = 2: d is even, so the pair is inside too)
    double cen[V];
#pragma unroll
    for (int v = 0; v < V; ++v) cen[v] = (center && okA) ? center[i0 + rloc + v] : 0.0;
    const int64_t CH = (N_r + NC - 1) / NC;
    double xa[U][V], w[U], zr[UZ];
    bool on[U];
    auto load = [&](int64_t it) {
        const int64_t n0 = it * NC;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t n = n0 + cslot + NSL * u;
            const bool use = n < N_r;
            const int64_t nc = use ? n : n0;                        // (clamped: an in-range column)
            w[u] = pool_weight(imp, wk, nc);
            on[u] = pool_counts(imp, use, w[u]);                     // a zero weight skips the column whatever it holds
#pragma unroll
            for (int v = 0; v < V; ++v) xa[u][v] = 0.0;
            if (okA && on[u]) {
                const double *p = run + (size_t)nc * d + i0 + rloc;
                if constexpr (V == 2) { const double2 t = *reinterpret_cast<const double2 *>(p); xa[u][0] = t.x; xa[u][V - 1] = t.y; }
                else xa[u][0] = p[0];
            }
        }
#pragma unroll
        for (int u = 0; u < UZ; ++u) {
            const int e = tid + APPLY_THREADS * u, n = e / RP, j = e % RP;
            zr[u] = (j < r && n0 + n < N_r) ? zk[(size_t)(n0 + n) * r + j] : 0.0;      // zero directions, zero columns past the run
        }
    };
    load(0);
    for (int64_t it = 0; it < CH; ++it) {
        __syncthreads();                                            // the previous chunk's operands have been read
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double *ap = a_s + (cslot + NSL * u) * TS + rloc;
#pragma unroll
            for (int v = 0; v < V; ++v) ap[v] = (on[u] && okA) ? w[u] * (xa[u][v] - cen[v]) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < UZ; ++u) {
            const int e = tid + APPLY_THREADS * u;
            z_s[(e / RP) * ZS + e % RP] = zr[u];
        }
        __syncthreads();
        const int64_t n0 = it * NC;
        const int ng = (int)(((N_r - n0 < NC ? N_r - n0 : NC) + 3) / 4);      // groups of 4 columns of this chunk (uniform)
        if (it + 1 < CH) load(it + 1);                              // in flight while the MFMAs run
        const double *ap = a_s + q * TS + 16 * wv + c, *zp = z_s + q * ZS + c;
        for (int g = 0; g < ng; ++g) {
            const double av = ap[4 * g * TS];
#pragma unroll
            for (int b = 0; b < RB; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, zp[4 * g * ZS + 16 * b], acc[b], 0, 0, 0);
        }
    }
    double *out = part + (size_t)k * r * d;
#pragma unroll
    for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int i = i0 + 16 * wv + q + 4 * rr, j = 16 * b + c;
            if (i < d && j < r) out[(size_t)j * d + i] = acc[b][rr];
        }
}

// y[e] = carry[e] (NULL: 0) + part[0][e] + part[1][e] + ... in run order, e < n = r d; carry and y may be the same buffer
__global__ __launch_bounds__(APPLY_THREADS) void pf_pool_apply_combine_kernel(int64_t n, int K, const double *__restrict__ part,
                                                                              const double *carry, double *y) {
    const int64_t e = (int64_t)blockIdx.x * APPLY_THREADS + threadIdx.x;
    if (e >= n) return;
    double s = carry ? carry[e] : 0.0;
    for (int k = 0; k < K; ++k) s += part[(size_t)k * n + e];
    y[e] = s;
}

template <int RB, int V>
static void apply_launch(pfmi_ctx *c, const double *wts, const double *d_center, int r, const double *d_v, bool scores) {
    const int64_t S = (int64_t)c->K * c->N_r;
    if (scores)
        hipLaunchKernelGGL((pf_pool_scores_kernel<RB, V>), dim3((unsigned)((S + APPLY_SCORE_COLS - 1) / APPLY_SCORE_COLS)),
                           dim3(APPLY_THREADS), 0, c->stream, c->d, S, r, c->pool.as<double>(), wts, d_center, d_v, c->apply_z.as<double>());
    else
        hipLaunchKernelGGL((pf_pool_apply_kernel<RB, V>), dim3((unsigned)((c->d + APPLY_T - 1) / APPLY_T), (unsigned)c->K),
                           dim3(APPLY_THREADS), 0, c->stream, c->d, c->N_r, r, c->pool.as<double>(), wts, d_center,
                           c->apply_z.as<double>(), c->apply_part.as<double>());
}

// c->apply_z = the scores (K N_r x r) and c->apply_y = Y (r x d) of the ctx's pool; d_center: device, d doubles or NULL; d_v: device,
// r d doubles; d_carry: device, r d doubles (it may be c->apply_y itself) or NULL (zeros)
int32_t pf_launch_pool_apply(pfmi_ctx *c, int64_t col_offset, int importance, const double *d_center, int r, const double *d_v,
                             const double *d_carry) {
    const int d = c->d, K = c->K;
    const int64_t S = (int64_t)K * c->N_r;
    PF_CHECK((S + APPLY_SCORE_COLS - 1) / APPLY_SCORE_COLS <= 0x7fffffffLL && K <= 65535, PFMI_ERR_ARG,
             "pool_apply: too many columns or runs for one launch");
    PF_TRY(c->apply_z.ensure(sizeof(double) * (size_t)S * r));
    PF_TRY(c->apply_part.ensure(sizeof(double) * (size_t)K * r * d));
    PF_TRY(c->apply_y.ensure(sizeof(double) * (size_t)r * d));
    const double *wts = pf_pool_weights(c, col_offset, importance);
    for (int pass = 0; pass < 2; ++pass) {
        pf_kernel_begin(c);
        if (r <= 16) {
            if (d % 2 == 0) apply_launch<1, 2>(c, wts, d_center, r, d_v, pass == 0);
            else apply_launch<1, 1>(c, wts, d_center, r, d_v, pass == 0);
        } else {
            if (d % 2 == 0) apply_launch<2, 2>(c, wts, d_center, r, d_v, pass == 0);
            else apply_launch<2, 1>(c, wts, d_center, r, d_v, pass == 0);
        }
        PF_HIP(hipGetLastError());
        pf_kernel_end(c, pass == 0 ? "pool_scores" : "pool_apply");
    }
    const int64_t n = (int64_t)r * d;
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_pool_apply_combine_kernel, dim3((unsigned)((n + APPLY_THREADS - 1) / APPLY_THREADS)), dim3(APPLY_THREADS), 0,
                       c->stream, n, K, c->apply_part.as<double>(), d_carry, c->apply_y.as<double>());
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "pool_apply_combine");
    return PFMI_OK;
}
