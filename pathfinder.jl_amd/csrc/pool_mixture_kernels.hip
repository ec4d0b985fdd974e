// pool_mixture_kernels.hip -- mixture-proposal log ratios of the resident pool (pfmi_pool_mixture_ratios): for every pool column g
//   comp[k][g] = logpdf(fit pool_points[k], pool[:, g]),  lmix[g] = lse_k comp[k][g] - log K,  ratio[g] = pool_lp[g] - lmix[g]
// -- the weights p / qbar of the pool read as a stratified sample of the uniform mixture qbar = (1/K) sum_k q_k it was drawn from.
//
// Components.  d <= 1024 or kpad = 64: the kernels of mixture_kernels.hip (pf_launch_mixture_comp, the bits of pfmi_mixture_logpdf).
// d > 1024 and kpad <= 32: pf_pool_mixture_tiled_kernel below, pf_mixture_mfma_kernel cut into row tiles of 1024 rows.  One 512-thread
// workgroup (8 waves) owns a tile of 16 columns and a group of components.  A row tile is 64 blocks of 16 rows; wave w takes the
// blocks w + 8 u, u < 8, and lane (q = lane>>4, c = lane&15) holds the block's rows 4 q .. 4 q + 3 of column c, fetched with ONE 32-byte
// load (x, mu and sqrt(alpha) alike): a wave's load covers 128 contiguous bytes of each of its 16 columns, and the eight waves eight
// adjacent such pieces.  (With the lane map of pf_mixture_mfma_kernel, one double per lane and step, the same kernel took 182 ms at
// 32 000 columns x 32 components, d = 10 000, kpad 20 -- slower than the lane kernel's 169 ms; with this one 62 ms,
// profiles/pool_mixture.md.)  The lane's element j < 4 is the B operand of v_mfma_f64_16x16x4_f64 for the k-group of rows
// {4 q' + j : q' < 4} of the block.  Per component
//   pass 1  W[j][n] = sum_i Vh[i][j] e[i][n],  e = (x - mu) / sqrt(alpha)     accumulated in the wave's fragment over ALL row tiles
//   (LDS)   W summed over the waves in wave order, tv = T' W                   as in pf_mixture_mfma_kernel
//   pass 2  r[i][n] = e[i][n] - sum_j Vh[i][j] tv[j][n]                        row tile by row tile, one MFMA chain per 16-row block:
//           the C / D fragment's row q + 4 reg IS the lane's row 4 q + reg of the block, so e goes in as loaded and the A operand
//           supplies the rows of Vh in that order
//   rows i >= KPAD: sum of r^2; rows i < KPAD (blocks 0 and 1 of row tile 0): V' y = r forward substitution
// The one block of d that is not whole (d is no multiple of 16) takes clamped single loads and selects.
// Nothing of the column is held in registers between the passes: X is read twice per component, the factor (Vh, mu, sqrt(alpha)) twice
// per workgroup and component, the latter from L2 (the workgroups walk the components in step).  Traffic model per workgroup and
// component: 2 x 16 d doubles of X + 2 d (KPAD + 2) doubles of factor.  Two workgroups per CU at kpad <= 20 (<= 128 VGPRs).
//
// Ordering rule: a column's terms are added in an order that depends on (d, KPAD) alone -- a wave's blocks in order, row tiles in
// order, the four q lanes inside the MFMA, the waves in wave order -- never on the column's place in its tile or in the pool, on K, on
// N_r, on the chunk the column falls into or on the number of components a workgroup takes.
//
// pf_pool_mixture_ratio_kernel: one thread per column, the log-sum-exp of pf_mixture_lse_kernel (components in order, NaN if any
// component is NaN, -inf if all are -inf), minus log K (formed once on the host), and the subtraction of pf_logratio_kernel.
#include "pfmi_common.h"

#include <stdlib.h>

#define PMX_THREADS 512
#define PMX_WAVES 8
#define PMX_NS 32                       // 32-row steps of a row tile (a wave takes PMX_NS / 4 blocks of 16 rows)
#define PMX_TILE (32 * PMX_NS)          // rows of a row tile
#define PMX_SCRATCH_MAX ((size_t)64 << 20)   // bytes of comp [K][chunk]

typedef double pmx_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ pmx_d4 pmx_mfma(double a, double b, pmx_d4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// four consecutive doubles from an address that is only 8-byte aligned (d is any number: a column or a factor row starts anywhere)
typedef double pmx_d4u __attribute__((ext_vector_type(4), aligned(8)));

// rows R + 4 q .. R + 4 q + 3 of the vector at p: one 32-byte load where the whole 16-row block lies inside d (FULL), otherwise four
// clamped loads with the rows >= d set to `fill`
template <bool FULL>
__device__ __forceinline__ pmx_d4 pmx_rows4(const double *__restrict__ p, int row, int d, double fill) {
    if constexpr (FULL) {
        const pmx_d4u v = *reinterpret_cast<const pmx_d4u *>(p + row);
        return pmx_d4{v[0], v[1], v[2], v[3]};
    } else {
        pmx_d4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = row + j;
            const double x = p[(i < d) ? i : d - 1];
            v[j] = (i < d) ? x : fill;
        }
        return v;
    }
}

template <int KPAD>
__global__ __launch_bounds__(PMX_THREADS, (KPAD <= 20 ? 4 : 2)) void pf_pool_mixture_tiled_kernel(
    int d, int64_t N, int K, int comps_per_block, const double *__restrict__ X, const int32_t *__restrict__ points,
    const double *__restrict__ vh, const double *__restrict__ tmat, const double *__restrict__ vchol, const double *__restrict__ sqrt_alpha,
    const double *__restrict__ mu_all, const double *__restrict__ logdet, const int32_t *__restrict__ status, double *__restrict__ comp) {
    constexpr int KT = (KPAD + 15) / 16;       // 16-row output tiles of pass 1
    constexpr int KQ = KPAD / 4;               // k-steps of pass 2
    __shared__ double wred[PMX_WAVES * KT * 4 * 64];   // per-wave W fragments
    __shared__ double ntv[KPAD * 16];                  // -tv[j][n]
    __shared__ double wsum[KPAD * 16];                 // W[j][n]
    __shared__ double head[KPAD * 16];                 // r[i][n], i < KPAD
    __shared__ double sred[PMX_WAVES * 64];            // per-lane partial sums of r^2
    __shared__ double t_s[KPAD * KPAD], vc_s[KPAD * KPAD];

    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
    const int64_t n = (int64_t)blockIdx.x * 16 + c;
    const bool nv = n < N;
    const int ntile = (d + PMX_TILE - 1) / PMX_TILE;
    const int k0 = blockIdx.y * comps_per_block;
    const int k1 = (k0 + comps_per_block < K) ? k0 + comps_per_block : K;
    const double *xcol = X + (size_t)(nv ? n : N - 1) * d;   // (a column past the end reads the last one and is never written)

    for (int k = k0; k < k1; ++k) {
        const int p = points[k];
        if (status[p] != PFMI_FIT_OK) {        // uniform over the workgroup
            if (tid < 16 && nv) comp[(size_t)k * N + n] = NAN;
            continue;
        }
        const double *Vh = vh + (size_t)p * d * KPAD, *T = tmat + (size_t)p * KPAD * KPAD, *Vc = vchol + (size_t)p * KPAD * KPAD;
        const double *sqa = sqrt_alpha + (size_t)p * d, *mu = mu_all + (size_t)p * d;
        for (int x = tid; x < KPAD * KPAD; x += PMX_THREADS) {   // (ordered before their use by the barrier after pass 1)
            t_s[x] = T[x];
            vc_s[x] = Vc[x];
        }
        // lane indices through an opaque copy per component (pf_mixture_mfma_kernel: otherwise the row offsets are hoisted out of the
        // component loop and kept alive)
        int q4 = 4 * q, cl = c;
        __asm__ volatile("" : "+v"(q4), "+v"(cl));

        // e of the lane's four rows R + 4 q + j of the 16-row block at R (rows >= d: zero)
        auto e_of = [&](auto FULL, const int R) {
            const pmx_d4 x = pmx_rows4<FULL()>(xcol, R + q4, d, 0.0), m = pmx_rows4<FULL()>(mu, R + q4, d, 0.0),
                         s = pmx_rows4<FULL()>(sqa, R + q4, d, 1.0);
            pmx_d4 e = (x - m) / s;
            if constexpr (!FULL()) {
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = (R + q4 + j < d) ? e[j] : 0.0;
            }
            return e;
        };

        // pass 1: the block's four k-groups are the rows {4 q' + j : q' < 4}, j < 4
        pmx_d4 accw[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) accw[t] = pmx_d4{0.0, 0.0, 0.0, 0.0};
        auto pass1 = [&](auto FULL, const int R) {
            const pmx_d4 e = e_of(FULL, R);
            double a[KT][4];
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = R + q4 + j, col = 16 * t + cl;
                    const int ic = (FULL() || i < d) ? i : d - 1, jc = (col < KPAD) ? col : KPAD - 1;
                    const double v = Vh[(size_t)ic * KPAD + jc];
                    a[t][j] = ((FULL() || i < d) && col < KPAD) ? v : 0.0;
                }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < KT; ++t) accw[t] = pmx_mfma(a[t][j], e[j], accw[t]);
        };
        for (int rt = 0; rt < ntile; ++rt) {
            const int r0 = rt * PMX_TILE + 16 * w;               // the wave's blocks of this row tile: r0 + 128 u, u < 8
            const int left = d - r0;                             // (may be <= 0)
            const int nfull = left < 16 ? 0 : (left - 16) / 128 + 1 < PMX_NS / 4 ? (left - 16) / 128 + 1 : PMX_NS / 4;
            int u = 0;
            for (; u + 1 < nfull; u += 2) {                      // two blocks per trip: their loads are issued together
                pass1(std::true_type{}, r0 + 128 * u);
                pass1(std::true_type{}, r0 + 128 * u + 128);
            }
            if (u < nfull) pass1(std::true_type{}, r0 + 128 * u);
            if (nfull < PMX_NS / 4 && r0 + 128 * nfull < d) pass1(std::false_type{}, r0 + 128 * nfull);   // the one ragged block of d
        }
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) wred[((w * KT + t) * 4 + r) * 64 + lane] = accw[t][r];
        __syncthreads();
        // W[j][n]: fragment (t = j / 16, row jj = j % 16 = q' + 4 r) of lane q' * 16 + n, summed in wave order
        for (int x = tid; x < KPAD * 16; x += PMX_THREADS) {
            const int j = x >> 4, nn = x & 15, t = j >> 4, jj = j & 15, l = (jj & 3) * 16 + nn, r = jj >> 2;
            double s = 0.0;
#pragma unroll
            for (int v = 0; v < PMX_WAVES; ++v) s += wred[((v * KT + t) * 4 + r) * 64 + l];
            wsum[x] = s;
        }
        __syncthreads();
        for (int x = tid; x < KPAD * 16; x += PMX_THREADS) {   // tv = T' W
            const int a = x >> 4, nn = x & 15;
            double s = 0.0;
            for (int b = 0; b <= a; ++b) s += t_s[b * KPAD + a] * wsum[b * 16 + nn];
            ntv[x] = -s;
        }
        __syncthreads();

        // pass 2: r = e - Vh tv per 16-row block.  The C / D fragment holds internal row rho = q + 4 reg of column c in lane (q, c); with
        // reg = j that is the lane's row R + 4 q + j, so C is e as loaded, and the A operand gives Vh row R + 4 (rho & 3) + (rho >> 2)
        // as row rho = c.
        double bt[KQ];
#pragma unroll
        for (int jq = 0; jq < KQ; ++jq) bt[jq] = ntv[(4 * jq + q) * 16 + c];
        double ss = 0.0;
        const int arow = 4 * (cl & 3) + (cl >> 2);
        auto pass2 = [&](auto FULL, const int R) {
            pmx_d4 acc = e_of(FULL, R);
            const int ia = R + arow, iac = (FULL() || ia < d) ? ia : d - 1;
            double a[KQ];
#pragma unroll
            for (int jq = 0; jq < KQ; ++jq) {
                const double v = Vh[(size_t)iac * KPAD + 4 * jq + q];
                a[jq] = (FULL() || ia < d) ? v : 0.0;
            }
#pragma unroll
            for (int jq = 0; jq < KQ; ++jq) acc = pmx_mfma(a[jq], bt[jq], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = R + q4 + j;
                if (i < KPAD) head[i * 16 + c] = acc[j];       // (rows < KPAD <= 32: blocks 0 and 1 of the first row tile, always whole)
                ss += (i >= KPAD && (FULL() || i < d)) ? acc[j] * acc[j] : 0.0;
            }
        };
        for (int rt = 0; rt < ntile; ++rt) {
            const int r0 = rt * PMX_TILE + 16 * w;
            const int left = d - r0;
            const int nfull = left < 16 ? 0 : (left - 16) / 128 + 1 < PMX_NS / 4 ? (left - 16) / 128 + 1 : PMX_NS / 4;
            int u = 0;
            for (; u + 1 < nfull; u += 2) {                      // two blocks per trip: their loads are issued together
                pass2(std::true_type{}, r0 + 128 * u);
                pass2(std::true_type{}, r0 + 128 * u + 128);
            }
            if (u < nfull) pass2(std::true_type{}, r0 + 128 * u);
            if (nfull < PMX_NS / 4 && r0 + 128 * nfull < d) pass2(std::false_type{}, r0 + 128 * nfull);
        }
        sred[w * 64 + lane] = ss;
        __syncthreads();
        if (tid < 16) {
            double s = 0.0;
#pragma unroll
            for (int v = 0; v < PMX_WAVES; ++v)
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) s += sred[v * 64 + qq * 16 + c];
            double zh[KPAD];
#pragma unroll
            for (int a = 0; a < KPAD; ++a) zh[a] = head[a * 16 + c];
#pragma unroll
            for (int a = 0; a < KPAD; ++a) {   // forward substitution V' y = zh (identity padded)
                double v = zh[a];
#pragma unroll
                for (int b = 0; b < a; ++b) v -= vc_s[b * KPAD + a] * zh[b];
                zh[a] = v / vc_s[a * KPAD + a];
                s += zh[a] * zh[a];
            }
            if (nv) comp[(size_t)k * N + n] = -((double)d * PF_LOG2PI + logdet[p]) / 2.0 - s / 2.0;
        }
        __syncthreads();                       // the LDS buffers are rewritten by the next component
    }
}

// lmix[n] = lse_k comp[k * N + n] - log_k and ratio[n] = lp[n] - lmix[n] for the N columns of a chunk
__global__ void pf_pool_mixture_ratio_kernel(int64_t N, int K, double log_k, const double *__restrict__ comp, const double *__restrict__ lp,
                                             double *__restrict__ lmix, double *__restrict__ ratio) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double m = -INFINITY;
    bool nan = false;
    for (int k = 0; k < K; ++k) {
        const double v = comp[(size_t)k * N + n];
        if (isnan(v)) nan = true;
        else if (v > m) m = v;
    }
    double lse;
    if (nan) lse = NAN;
    else if (m == -INFINITY) lse = -INFINITY;
    else {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += exp(comp[(size_t)k * N + n] - m);
        lse = m + log(s);
    }
    const double lm = lse - log_k;
    lmix[n] = lm;
    ratio[n] = lp[n] - lm;
}

// comp [K][N] of the N columns d_x for the pool's own components by the row-tiled kernel (d > 1024, kpad <= 32)
static int32_t launch_tiled(pfmi_ctx *c, int64_t N, const double *d_x, double *d_comp) {
    const int d = c->d, K = c->K;
    const int64_t ntiles = (N + 15) / 16;
    PF_CHECK(ntiles <= INT32_MAX, PFMI_ERR_ARG, "pool_mixture_ratios: chunk too long");
    // enough workgroups for every CU several times over (pf_launch_mixture_logpdf's rule): the components are split into groups
    const int ncu = c->ncu > 0 ? c->ncu : 256;
    int64_t ng = (8 * (int64_t)ncu + ntiles - 1) / ntiles;
    if (ng < 1) ng = 1;
    if (ng > K) ng = K;
    int cpb = (int)((K + ng - 1) / ng);
    if (const char *f = pf_debug_get("PFMI_MIXTURE_CPB")) { const int v = atoi(f); cpb = v < 1 ? 1 : (v > K ? K : v); }   // test hook: the group size
    dim3 grid((unsigned)ntiles, (unsigned)((K + cpb - 1) / cpb));
    const bool ok = pf_dispatch_kpad<4, 8, 12, 16, 20, 32>(c->kpad, [&](auto KP) {
        hipLaunchKernelGGL(pf_pool_mixture_tiled_kernel<KP()>, grid, dim3(PMX_THREADS), 0, c->stream, d, N, K, cpb, d_x,
                           c->pool_points.as<int32_t>(), c->vh.as<double>(), c->tmat.as<double>(), c->vchol.as<double>(),
                           c->sqrt_alpha.as<double>(), c->mu.as<double>(), c->logdet.as<double>(), c->status.as<int32_t>(), d_comp);
    });
    PF_CHECK(ok, PFMI_ERR_UNSUPPORTED, "unsupported kpad %d", c->kpad);
    PF_HIP(hipGetLastError());
    return PFMI_OK;
}

// pool_lmix and pool_lr_mix of the ctx's pool.  Route: d <= 1024 or kpad = 64 -> the component kernels of mixture_kernels.hip; d > 1024 and
// kpad <= 32 -> the row-tiled kernel.  The pool is walked in chunks of columns so that comp [K][chunk] stays within PMX_SCRATCH_MAX
// (PFMI_POOL_MIX_CHUNK: the chunk length); a column's bits do not depend on the chunk it falls into.
int32_t pf_launch_pool_mixture_ratios(pfmi_ctx *c) {
    const int d = c->d, K = c->K, kp = c->kpad;
    const int64_t S = (int64_t)K * c->N_r;
    PF_CHECK(kp == 4 || kp == 8 || kp == 12 || kp == 16 || kp == 20 || kp == 32 || kp == 64, PFMI_ERR_UNSUPPORTED, "unsupported kpad %d", kp);
    const bool tiled = d > PMX_TILE && kp <= 32;
    int64_t chunk = (int64_t)(PMX_SCRATCH_MAX / (sizeof(double) * (size_t)K)) / 16 * 16;
    if (chunk < 16) chunk = 16;
    if (const char *f = pf_debug_get("PFMI_POOL_MIX_CHUNK")) { const long long v = atoll(f); if (v >= 1) chunk = v; }   // test hook
    if (chunk > S) chunk = S;
    PF_TRY(c->pool_mix_comp.ensure(sizeof(double) * (size_t)K * (size_t)chunk));
    PF_TRY(c->pool_lmix.ensure(sizeof(double) * (size_t)S));
    PF_TRY(c->pool_lr_mix.ensure(sizeof(double) * (size_t)S));
    const double log_k = log((double)K);
    double *comp = c->pool_mix_comp.as<double>();
    for (int64_t g0 = 0; g0 < S; g0 += chunk) {
        const int64_t n = (S - g0 < chunk) ? S - g0 : chunk;
        const double *x = c->pool.as<double>() + (size_t)g0 * d;
        pf_kernel_begin(c);
        if (tiled) PF_TRY(launch_tiled(c, n, x, comp));
        else PF_TRY(pf_launch_mixture_comp(c, K, c->pool_points.as<int32_t>(), n, x, comp));
        pf_kernel_end(c, "pool_mixture_comp");
        pf_kernel_begin(c);
        hipLaunchKernelGGL(pf_pool_mixture_ratio_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, K, log_k, comp,
                           c->pool_lp.as<double>() + g0, c->pool_lmix.as<double>() + g0, c->pool_lr_mix.as<double>() + g0);
        PF_HIP(hipGetLastError());
        pf_kernel_end(c, "pool_mixture_ratio");
    }
    return PFMI_OK;
}
