// pool_cross_kernels.hip -- weighted cross moments of the pool: the lower triangle of sum_n (w t_i) t_j, mirrored (pfmi_pool_cross; the
// quantities are defined in include/pfmi.h).
//
// For the ctx's pool (d x (K N_r), column-major, one column per draw), t = x - center and i >= j:
//   C[i][j] = C_in[i][j] + sum_runs k (in run order) sum_n fl(w fl(x_i - c_i)) * fl(x_j - c_j)
// w and the zero-weight rule are those of every pass over the pool (pool_geometry.h: pf_pool_weights, pool_weight, pool_counts): weights[col_offset +
// k N_r + n], or 1 without importance weighting; a skipped column makes both operands 0.
//
// One workgroup (256 threads = 4 waves) owns one T x T tile of the lower triangle, diagonal tiles included, for the whole launch.  The
// tile is cut 2 x 2 among the waves; a wave holds its T/2 x T/2 quarter as (T/32)^2 accumulators of v_mfma_f64_16x16x4_f64 (C/D: lane
// (q = lane>>4, c = lane&15), register r holds row q + 4 r of column c), initialised from C_in.  The contraction index is the draw:
// per group of 4 columns n0 .. n0+3 the A operand is w t of a 16-row block of the tile's rows (lane: A[row c][n0 + q]) and the B operand
// is t of a 16-row block of the tile's columns (lane: B[n0 + q][column c]).
//   staging   the workgroup walks the runs in order and each run in chunks of NC = 2048 / T columns.  A chunk's two slabs (T rows of the
//             row block, T rows of the column block) are loaded with lanes along rows (V = 2, 16-byte loads, when d is even: the
//             alignment rule of pool_geometry.h; tiles start at even rows), centred and weighted ONCE, and written to LDS as
//             [column][row] with rows of T + 16 doubles (the 4 columns a wave reads together then fall on different banks).  The loads of
//             chunk c + 1 are in flight while the MFMAs of chunk c run (16 doubles per thread whatever T and V are).
//   tails     rows >= d are 0 in both slabs.  A run's last chunk holds N_r % NC columns; its groups of 4 are completed with zero
//             columns, which add exact zeros.  The padding is per run: the next run starts a new group.
//   epilogue  entries with i >= j are written to C[i][j] and copied to C[j][i]: the two triangles have the same bits.  In a diagonal
//             tile the wave above the diagonal does no MFMAs and writes nothing.
// T = 64 (16 accumulator doubles per lane) or 128 (64 doubles): the tile never changes the bits, only how often the pool is re-read
// (pool bytes x d / T, from L2 / Infinity Cache) and how many workgroups there are (pf_launch_pool_cross picks).
//
// Ordering contract (the one of pfmi_pool_cdf):
//   - No atomics.
//   - The terms of one run are added in an order that depends on (d, N_r) only.  It does not depend on K, col_offset, the run's position
//     or the device: an entry is ONE chain of MFMAs over the run's groups of 4 columns, whatever T, V and NC are.
//   - Runs are added in run order on top of C_in, which is added first.
//   - So contexts chained in run order, each passing its result to the next, return the bits of one context holding all the runs.
// Small d gives few workgroups (one at d <= 64) and a slow pass; there is no second kernel for it.
#include "pfmi_common.h"
#include "pool_geometry.h"       // pool_weight, pool_counts, pf_pool_weights

#include <stdlib.h>

#define CROSS_THREADS 256
#define CROSS_STAGE 2048            // doubles of one slab of a chunk: NC = CROSS_STAGE / T columns
#define CROSS_PAD 16                // doubles added to an LDS row
#define CROSS_T128_MIN_D 4096       // d from which the 128 x 128 tile is used (profiles/pool_covariance.md)

typedef double cross_d4 __attribute__((ext_vector_type(4)));

// carry and out may be the same buffer: a workgroup reads only its own entries with i >= j, all of them before it writes any, and
// nobody reads an entry with i < j
template <int T, int V>
__global__ __launch_bounds__(CROSS_THREADS) void pf_pool_cross_kernel(int d, int K, int64_t N_r, const double *__restrict__ pool,
                                                                      const double *__restrict__ wts, const double *__restrict__ center,
                                                                      const double *carry, double *out) {
    constexpr int TB = T / 32;                       // 16-blocks of a wave's quarter, per side
    constexpr int NC = CROSS_STAGE / T;              // columns of a chunk
    constexpr int LR = T / V;                        // threads along the rows of one column
    constexpr int NSL = CROSS_THREADS / LR;          // columns loaded side by side
    constexpr int U = NC / NSL;                      // columns per thread and chunk
    constexpr int TS = T + CROSS_PAD;
    __shared__ __attribute__((aligned(16))) double a_s[NC * TS], b_s[NC * TS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
    // tile (bi, bj), bi >= bj, of the lower triangle: blockIdx.x = bi (bi + 1) / 2 + bj
    const int64_t p = blockIdx.x;
    int64_t bi = (int64_t)((__builtin_sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (bi * (bi + 1) / 2 > p) --bi;
    while ((bi + 1) * (bi + 2) / 2 <= p) ++bi;
    const int64_t bj = p - bi * (bi + 1) / 2;
    const int i0 = (int)(bi * T), j0 = (int)(bj * T);
    const int wr = wv >> 1, wc = wv & 1;
    const bool idle = bi == bj && wc > wr;           // the quarter above the diagonal
    const bool imp = wts != nullptr;

    cross_d4 acc[TB][TB];
#pragma unroll
    for (int a = 0; a < TB; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wr * (T / 2) + 16 * a + q + 4 * r, j = j0 + wc * (T / 2) + 16 * b + c;
                acc[a][b][r] = (carry && i < d && j < d && i >= j) ? carry[(size_t)i * d + j] : 0.0;
            }

    // staging: this thread's V rows of both slabs and its column slot
    const int rloc = (tid % LR) * V, cslot = tid / LR;
    const bool okA = i0 + rloc < d, okB = j0 + rloc < d;            // (V = 2: d is even, so the pair is inside too)
    double cenA[V], cenB[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        cenA[v] = (center && okA) ? center[i0 + rloc + v] : 0.0;
        cenB[v] = (center && okB) ? center[j0 + rloc + v] : 0.0;
    }
    const int64_t CH = (N_r + NC - 1) / NC, NIT = (int64_t)K * CH;
    double xa[U][V], xb[U][V], w[U];
    bool on[U];
    auto load = [&](int64_t it) {
        const int64_t k = it / CH, n0 = (it - k * CH) * NC;
        const double *run = pool + (size_t)k * N_r * d;             // column n of the run: run + n d
        const double *wk = imp ? wts + (size_t)k * N_r : nullptr;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t n = n0 + cslot + NSL * u;
            const bool use = n < N_r;
            const int64_t nc = use ? n : n0;                        // (clamped: an in-range column)
            w[u] = pool_weight(imp, wk, nc);
            on[u] = pool_counts(imp, use, w[u]);                     // a zero weight skips the column whatever it holds
            const double *col = run + (size_t)nc * d;
#pragma unroll
            for (int v = 0; v < V; ++v) xa[u][v] = xb[u][v] = 0.0;
            if constexpr (V == 2) {
                if (okA) { const double2 t = *reinterpret_cast<const double2 *>(col + i0 + rloc); xa[u][0] = t.x; xa[u][V - 1] = t.y; }
                if (okB) { const double2 t = *reinterpret_cast<const double2 *>(col + j0 + rloc); xb[u][0] = t.x; xb[u][V - 1] = t.y; }
            } else {
                if (okA) xa[u][0] = col[i0 + rloc];
                if (okB) xb[u][0] = col[j0 + rloc];
            }
        }
    };
    load(0);
    for (int64_t it = 0; it < NIT; ++it) {
        __syncthreads();                                            // the previous chunk's operands have been read
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double *ap = a_s + (cslot + NSL * u) * TS + rloc, *bp = b_s + (cslot + NSL * u) * TS + rloc;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double ta = xa[u][v] - cenA[v], tb = xb[u][v] - cenB[v];
                ap[v] = (on[u] && okA) ? w[u] * ta : 0.0;
                bp[v] = (on[u] && okB) ? tb : 0.0;
            }
        }
        __syncthreads();
        const int64_t n0 = (it % CH) * NC;
        const int ng = (int)(((N_r - n0 < NC ? N_r - n0 : NC) + 3) / 4);      // groups of 4 columns of this chunk (uniform)
        if (it + 1 < NIT) load(it + 1);                             // in flight while the MFMAs run
        if (!idle) {
            for (int g = 0; g < ng; ++g) {
                const double *ap = a_s + (4 * g + q) * TS + wr * (T / 2) + c, *bp = b_s + (4 * g + q) * TS + wc * (T / 2) + c;
                double av[TB], bv[TB];
#pragma unroll
                for (int a = 0; a < TB; ++a) { av[a] = ap[16 * a]; bv[a] = bp[16 * a]; }
#pragma unroll
                for (int a = 0; a < TB; ++a)
#pragma unroll
                    for (int b = 0; b < TB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
            }
        }
    }
    if (idle) return;
#pragma unroll
    for (int a = 0; a < TB; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wr * (T / 2) + 16 * a + q + 4 * r, j = j0 + wc * (T / 2) + 16 * b + c;
                if (i < d && j < d && i >= j) {
                    out[(size_t)i * d + j] = acc[a][b][r];
                    out[(size_t)j * d + i] = acc[a][b][r];
                }
            }
}

template <int T, int V>
static void cross_launch(pfmi_ctx *c, const double *wts, const double *d_center, const double *d_carry) {
    const int64_t nb = ((int64_t)c->d + T - 1) / T;
    hipLaunchKernelGGL((pf_pool_cross_kernel<T, V>), dim3((unsigned)(nb * (nb + 1) / 2)), dim3(CROSS_THREADS), 0, c->stream, c->d, c->K,
                       c->N_r, c->pool.as<double>(), wts, d_center, d_carry, c->cross.as<double>());
}

// c->cross = C (d x d, both triangles) of the ctx's pool; d_center: device, d doubles or NULL; d_carry: device, d d doubles (it may be
// c->cross itself) or NULL (zeros)
int32_t pf_launch_pool_cross(pfmi_ctx *c, int64_t col_offset, int importance, const double *d_center, const double *d_carry) {
    const int d = c->d;
    PF_TRY(c->cross.ensure(sizeof(double) * (size_t)d * d));
    const double *wts = pf_pool_weights(c, col_offset, importance);
    int tile = d >= CROSS_T128_MIN_D ? 128 : 64;
    if (const char *f = pf_debug_get("PFMI_POOL_CROSS_TILE")) { const int v = atoi(f); if (v == 64 || v == 128) tile = v; }   // A/B hook: same bits
    const int64_t nb = ((int64_t)d + tile - 1) / tile;
    PF_CHECK(nb * (nb + 1) / 2 <= 0x7fffffffLL, PFMI_ERR_ARG, "pool_cross: too many tiles for one launch");
    pf_kernel_begin(c);
    if (tile == 128) {
        if (d % 2 == 0) cross_launch<128, 2>(c, wts, d_center, d_carry);
        else cross_launch<128, 1>(c, wts, d_center, d_carry);
    } else {
        if (d % 2 == 0) cross_launch<64, 2>(c, wts, d_center, d_carry);
        else cross_launch<64, 1>(c, wts, d_center, d_carry);
    }
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "pool_cross");
    return PFMI_OK;
}
