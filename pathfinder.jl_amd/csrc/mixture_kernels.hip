// mixture_kernels.hip -- logpdf of a uniform mixture of fits (pfmi_mixture_logpdf): comp[n + N k] = logpdf(fit points[k], X[:, n])
// and lse[n] = log sum_k exp(comp[n + N k]) (unnormalised: no - log K, so that the sums of several engines can be combined).
//
// Main kernel (d <= 1024, kpad <= 32): one 512-thread workgroup (8 waves) owns a tile of 16 points and a group of components.
// The tile of X is read from HBM once and held in registers; each component's factor (mu, sqrt(alpha), Vh, T, V) comes from L2
// (T and V through LDS; Vh, mu and sqrt(alpha) staged into LDS where they fit, see STAGE below).
// A lane is (q = lane>>4, c = lane&15): it holds rows i = 4 (w + 8 s) + q, s < 32, of point c of the tile -- for one s, four rows
// of all 16 points, which is the B operand of v_mfma_f64_16x16x4_f64 (B[k][n]: k = lane>>4, n = lane&15).  Per component:
//   e       = (x - mu) / sqrt(alpha)                                      VALU (formed in each pass; STAGE: times 1 / sqrt(alpha))
//   pass 1  W[j][n] = sum_i Vh[i][j] e[i][n]                              A = Vh^T (KPAD/16 rounded up MFMAs per 4 rows)
//   (LDS)   W summed over the waves in wave order, tv = T' W              one thread per (j, n), the order of pf_logpdf_lane
//   pass 2  r[i][n] = e[i][n] - sum_j Vh[i][j] tv[j][n]                   A = Vh (rows permuted), B = -tv, C = e: KPAD/4 MFMAs per 16 rows
//   rows i >= KPAD: sum of r^2 (lane, then the 4 lanes and 8 waves in fixed order); rows i < KPAD: V' y = r forward substitution
// The C/D fragment of the 16x16x4 f64 MFMA holds row q + 4 reg of column c in lane (q, c), register reg.  Pass 2 takes the four
// row steps s = 4u + reg as one 16-row block, so its C operand is exactly the e registers of those steps, and its A operand
// supplies Vh row 4 (w + 8 (4u + (rho>>2))) + (rho&3) as row rho.  Both passes are true contractions over the d x KPAD block.
// The sums run in a different order from pf_logpdf_lane's, so the two agree to rounding, not bit for bit.
// Where it fits beside the kernel's own buffers (32 ns (KPAD + 2) doubles + the static LDS <= 160 KB: kpad <= 12 at d <= 1024), each
// component's Vh, mu and sqrt(alpha) are first staged into LDS with wide loads (STAGE); otherwise the passes read them from L2 in
// chunks of steps whose loads are issued together.
//
// General path (d > 1024 or kpad = 64, or PFMI_MIXTURE_KERNEL=lane): pf_logpdf_lane with one grid row per component, the bits
// of pfmi_logpdf.
//
// lse kernel: one thread per point, components in order: m = max_k comp, lse = m + log sum_k exp(comp - m); NaN if any component
// is NaN, -inf if all are -inf.  The result does not depend on the grid of either kernel.
#include "pfmi_common.h"
#include "logpdf_lane.h"

#include <string.h>

#define MX_THREADS 512
#define MX_WAVES 8
#define MX_NS 32                 // row steps per lane: rows 4 (w + 8 s) + q < 32 * MX_NS = 1024
#define MX_DMAX (32 * MX_NS)
#define MX_LANE_THREADS 256
#define MX_LDS_MAX (160 * 1024)   // LDS of a CU
#define MX_HOIST2 2              // 16-row blocks of pass 2 whose loads are issued together

typedef double mx_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ mx_d4 mx_mfma(double a, double b, mx_d4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// static LDS of pf_mixture_mfma_kernel<KPAD> (doubles): wred, ntv, wsum, head, sred, t_s, vc_s
__host__ __device__ constexpr int mx_static_lds(int kpad) {
    return MX_WAVES * ((kpad + 15) / 16) * 4 * 64 + 3 * kpad * 16 + MX_WAVES * 64 + 2 * kpad * kpad;
}

// STAGE: each component's Vh, mu and 1 / sqrt(alpha) are first copied into LDS (dynamic, 8 * 32 ns (KPAD + 2) bytes) with wide
// coalesced loads -- one trip to L2 per component instead of one per chunk of steps, and one division per row instead of two per
// row and point; otherwise both passes read the factor from L2 and divide
template <int KPAD, bool STAGE>
__global__ __launch_bounds__(MX_THREADS) void pf_mixture_mfma_kernel(int d, int64_t N, int K, int comps_per_block,
                                                                     const double *__restrict__ X, const int32_t *__restrict__ points,
                                                                     const double *__restrict__ vh, const double *__restrict__ tmat,
                                                                     const double *__restrict__ vchol, const double *__restrict__ sqrt_alpha,
                                                                     const double *__restrict__ mu_all, const double *__restrict__ logdet,
                                                                     const int32_t *__restrict__ status, double *__restrict__ comp) {
    constexpr int KT = (KPAD + 15) / 16;       // 16-row output tiles of pass 1
    constexpr int KQ = KPAD / 4;               // k-steps of pass 2
    constexpr int MX_HOIST = (KT == 1) ? 8 : 4;   // row steps of pass 1 whose loads are issued together
    __shared__ double wred[MX_WAVES * KT * 4 * 64];   // per-wave partial W fragments
    __shared__ double ntv[KPAD * 16];                 // -tv[j][n]
    __shared__ double wsum[KPAD * 16];                // W[j][n]
    __shared__ double head[KPAD * 16];                // r[i][n], i < KPAD
    __shared__ double sred[MX_WAVES * 64];            // per-lane partial sums of r^2
    __shared__ double t_s[KPAD * KPAD], vc_s[KPAD * KPAD];   // T and V of the component (read in loops whose trip count is runtime)
    extern __shared__ __attribute__((aligned(16))) double mx_dyn[];   // STAGE: Vh [32 ns][KPAD], mu [32 ns], sqrt(alpha) [32 ns]
    static_assert(mx_static_lds(KPAD) == MX_WAVES * KT * 4 * 64 + 3 * KPAD * 16 + MX_WAVES * 64 + 2 * KPAD * KPAD, "static LDS");

    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
    const int64_t n = (int64_t)blockIdx.x * 16 + c;
    const bool nv = n < N;
    const int ns = (d + 31) >> 5;              // row steps that hold real rows (same for every wave)
    const int k0 = blockIdx.y * comps_per_block;
    const int k1 = (k0 + comps_per_block < K) ? k0 + comps_per_block : K;

    double xr[MX_NS];
#pragma unroll
    for (int s = 0; s < MX_NS; ++s) {
        const int i = 4 * (w + 8 * s) + q;
        const double v = X[(size_t)(nv ? n : N - 1) * d + ((i < d) ? i : d - 1)];
        xr[s] = (nv && i < d) ? v : 0.0;
    }

    for (int k = k0; k < k1; ++k) {
        const int p = points[k];
        if (status[p] != PFMI_FIT_OK) {        // uniform over the workgroup
            if (tid < 16 && nv) comp[(size_t)k * N + n] = NAN;
            continue;
        }
        const double *Vh = vh + (size_t)p * d * KPAD, *T = tmat + (size_t)p * KPAD * KPAD, *Vc = vchol + (size_t)p * KPAD * KPAD;
        const double *sqa = sqrt_alpha + (size_t)p * d, *mu = mu_all + (size_t)p * d;
        for (int x = tid; x < KPAD * KPAD; x += MX_THREADS) {   // (ordered before their use by the barrier after pass 1)
            t_s[x] = T[x];
            vc_s[x] = Vc[x];
        }
        if constexpr (STAGE) {
            const int rows = 32 * ns;          // rows >= d are zero (sqrt(alpha): one), so they contribute nothing
            double *vh_s = mx_dyn, *mu_s = vh_s + (size_t)rows * KPAD, *rsqa_s = mu_s + rows;
            const int npair = rows * KPAD / 2, lim = d * KPAD / 2;
            const double2 *src = reinterpret_cast<const double2 *>(Vh);
            for (int j0 = tid; j0 < npair; j0 += MX_THREADS * 4) {   // four 16-byte loads in flight per thread
                double2 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int j = j0 + u * MX_THREADS; v[u] = src[(j < lim) ? j : lim - 1]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * MX_THREADS;
                    if (j < npair) reinterpret_cast<double2 *>(vh_s)[j] = (j < lim) ? v[u] : make_double2(0.0, 0.0);
                }
            }
            for (int i = tid; i < rows; i += MX_THREADS) {
                mu_s[i] = (i < d) ? mu[i] : 0.0;
                rsqa_s[i] = (i < d) ? 1.0 / sqa[i] : 0.0;   // (one division per row, not two per row and point)
            }
            __syncthreads();
            Vh = vh_s; mu = mu_s; sqa = rsqa_s;
        }

        // lane indices through an opaque copy per component: otherwise the compiler hoists every step's row offsets (they do not
        // depend on the component) out of the component loop and keeps ~100 VGPRs of them alive
        int ib = 4 * w + q, cl = c;
        __asm__ volatile("" : "+v"(ib), "+v"(cl));

        // e and pass 1 (e is formed again in pass 2: holding it would double the registers of the X tile)
        auto e_of = [&](const int s) {
            const int i = ib + 32 * s, ic = (i < d) ? i : d - 1;   // (clamped loads and selects: no divergent branches)
            const double v = STAGE ? (xr[s] - mu[ic]) * sqa[ic] : (xr[s] - mu[ic]) / sqa[ic];   // (STAGE: sqa holds 1 / sqrt(alpha))
            return (i < d) ? v : 0.0;
        };
        mx_d4 accw[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) accw[t] = mx_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s0 = 0; s0 < MX_NS; s0 += MX_HOIST) {
            // chunks of MX_HOIST steps without a branch inside, so that a chunk's loads are all issued before its first MFMA waits.
            // They may not be hoisted further (all 32 steps' loads at once spill): the factor pointers pass through an opaque copy
            // per chunk, and no load can be issued before the copy that gives its address.
            if (s0 < ns) {
                if constexpr (!STAGE) __asm__ volatile("" : "+s"(mu), "+s"(sqa), "+s"(Vh));
#pragma unroll
                for (int s = s0; s < s0 + MX_HOIST; ++s) {
                    const int i = ib + 32 * s;
                    const double es = e_of(s);
#pragma unroll
                    for (int t = 0; t < KT; ++t) {
                        const int j = 16 * t + cl;
                        const int ic = (i < d) ? i : d - 1, jc = (j < KPAD) ? j : KPAD - 1;
                        const double v = Vh[(size_t)ic * KPAD + jc];
                        const double a = (i < d && j < KPAD) ? v : 0.0;
                        accw[t] = mx_mfma(a, es, accw[t]);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) wred[((w * KT + t) * 4 + r) * 64 + lane] = accw[t][r];
        __syncthreads();
        // W[j][n]: fragment (t = j / 16, row jj = j % 16 = q' + 4 r) of lane q' * 16 + n, summed in wave order
        for (int x = tid; x < KPAD * 16; x += MX_THREADS) {
            const int j = x >> 4, nn = x & 15, t = j >> 4, jj = j & 15, l = (jj & 3) * 16 + nn, r = jj >> 2;
            double s = 0.0;
#pragma unroll
            for (int v = 0; v < MX_WAVES; ++v) s += wred[((v * KT + t) * 4 + r) * 64 + l];
            wsum[x] = s;
        }
        __syncthreads();
        for (int x = tid; x < KPAD * 16; x += MX_THREADS) {   // tv = T' W
            const int a = x >> 4, nn = x & 15;
            double s = 0.0;
            for (int b = 0; b <= a; ++b) s += t_s[b * KPAD + a] * wsum[b * 16 + nn];
            ntv[x] = -s;
        }
        __syncthreads();

        // pass 2: r = e - Vh tv, 16 rows (steps 4u .. 4u + 3) per block (the same opaque pointer copies: one block's loads at a time)
        double bt[KQ];
#pragma unroll
        for (int jq = 0; jq < KQ; ++jq) bt[jq] = ntv[(4 * jq + q) * 16 + c];
        double ss = 0.0;
        const int arow_in_blk = 4 * w + 32 * (cl >> 2) + (cl & 3);   // A row rho = c: Vh row arow_in_blk + 128 u
#pragma unroll
        for (int u0 = 0; u0 < MX_NS / 4; u0 += MX_HOIST2) {
            if (4 * u0 < ns) {                 // (chunks as in pass 1)
                if constexpr (!STAGE) __asm__ volatile("" : "+s"(mu), "+s"(sqa), "+s"(Vh));
#pragma unroll
                for (int u = u0; u < u0 + MX_HOIST2; ++u) {
                    mx_d4 acc = mx_d4{e_of(4 * u), e_of(4 * u + 1), e_of(4 * u + 2), e_of(4 * u + 3)};
                    const int ia = arow_in_blk + 128 * u, iac = (ia < d) ? ia : d - 1;
#pragma unroll
                    for (int jq = 0; jq < KQ; ++jq) {
                        const double v = Vh[(size_t)iac * KPAD + 4 * jq + q];
                        const double a = (ia < d) ? v : 0.0;
                        acc = mx_mfma(a, bt[jq], acc);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = ib + 32 * (4 * u + r);
                        if (u == 0 && r == 0 && i < KPAD) head[i * 16 + c] = (i < d) ? acc[r] : 0.0;   // (KPAD <= 32: every head row)
                        ss += (i >= KPAD && i < d) ? acc[r] * acc[r] : 0.0;
                    }
                }
            }
        }
        sred[w * 64 + lane] = ss;
        __syncthreads();
        if (tid < 16) {
            double s = 0.0;
#pragma unroll
            for (int v = 0; v < MX_WAVES; ++v)
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
        __syncthreads();                       // wred / wsum / ntv / head / sred (and the staged factor) are rewritten by the next component
    }
}

template <int KPAD>
__global__ __launch_bounds__(MX_LANE_THREADS) void pf_mixture_lane_kernel(int d, int64_t N, const double *__restrict__ X,
                                                                          const int32_t *__restrict__ points, const double *__restrict__ vh,
                                                                          const double *__restrict__ tmat, const double *__restrict__ vchol,
                                                                          const double *__restrict__ sqrt_alpha, const double *__restrict__ mu_all,
                                                                          const double *__restrict__ logdet, const int32_t *__restrict__ status,
                                                                          double *__restrict__ comp) {
    const int64_t n = (int64_t)blockIdx.x * MX_LANE_THREADS + threadIdx.x;
    const int k = blockIdx.y;
    if (n >= N) return;
    comp[(size_t)k * N + n] = pf_logpdf_lane<KPAD>(d, points[k], X + (size_t)n * d, vh, tmat, vchol, sqrt_alpha, mu_all, logdet, status);
}

__global__ void pf_mixture_lse_kernel(int64_t N, int K, const double *__restrict__ comp, double *__restrict__ lse) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double m = -INFINITY;
    bool nan = false;
    for (int k = 0; k < K; ++k) {
        const double v = comp[(size_t)k * N + n];
        if (isnan(v)) nan = true;
        else if (v > m) m = v;
    }
    double out;
    if (nan) out = NAN;
    else if (m == -INFINITY) out = -INFINITY;
    else {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += exp(comp[(size_t)k * N + n] - m);
        out = m + log(s);
    }
    lse[n] = out;
}

// comp [K][N] from X (d, N) for the K fit points d_points (device, int32, validated by the caller): the launch alone, no timing pair
int32_t pf_launch_mixture_comp(pfmi_ctx *c, int K, const int32_t *d_points, int64_t N, const double *d_x, double *d_comp) {
    const int d = c->d, kp = c->kpad;
    const char *force = pf_debug_get("PFMI_MIXTURE_KERNEL");
    const bool lane = (force && strcmp(force, "lane") == 0) || d > MX_DMAX || kp > 32;
    if (lane) {
        PF_CHECK((N + MX_LANE_THREADS - 1) / MX_LANE_THREADS <= INT32_MAX, PFMI_ERR_ARG, "mixture_logpdf: N too large");
        dim3 grid((unsigned)((N + MX_LANE_THREADS - 1) / MX_LANE_THREADS), (unsigned)K);
        const bool ok = pf_dispatch_kpad<4, 8, 12, 16, 20, 32, 64>(kp, [&](auto KP) {
            hipLaunchKernelGGL(pf_mixture_lane_kernel<KP()>, grid, dim3(MX_LANE_THREADS), 0, c->stream, d, N, d_x, d_points,
                               c->vh.as<double>(), c->tmat.as<double>(), c->vchol.as<double>(), c->sqrt_alpha.as<double>(), c->mu.as<double>(),
                               c->logdet.as<double>(), c->status.as<int32_t>(), d_comp);
        });
        PF_CHECK(ok, PFMI_ERR_UNSUPPORTED, "unsupported kpad %d", kp);
    } else {
        const int64_t ntiles = (N + 15) / 16;
        PF_CHECK(ntiles <= INT32_MAX, PFMI_ERR_ARG, "mixture_logpdf: N too large");
        // enough workgroups for every CU several times over: the components are split into groups (each re-reads its X tile)
        const int ncu = c->ncu > 0 ? c->ncu : 256;
        int64_t ng = (8 * (int64_t)ncu + ntiles - 1) / ntiles;
        if (ng < 1) ng = 1;
        if (ng > K) ng = K;
        int cpb = (int)((K + ng - 1) / ng);
        if (const char *f = pf_debug_get("PFMI_MIXTURE_CPB")) { const int v = atoi(f); cpb = v < 1 ? 1 : (v > K ? K : v); }   // test hook: the group size
        const int ngroups = (K + cpb - 1) / cpb;
        dim3 grid((unsigned)ntiles, (unsigned)ngroups);
        int32_t rc = PFMI_OK;
        const bool ok = pf_dispatch_kpad<4, 8, 12, 16, 20, 32>(kp, [&](auto KPc) {
            constexpr int KP = KPc();
            const size_t dyn = sizeof(double) * (size_t)32 * ((d + 31) / 32) * (KP + 2);
            if (dyn + sizeof(double) * mx_static_lds(KP) <= MX_LDS_MAX) {           // the factor block staged in LDS
                rc = pf_raise_lds_limit(c, reinterpret_cast<const void *>(pf_mixture_mfma_kernel<KP, true>),
                                        (int)(MX_LDS_MAX - sizeof(double) * mx_static_lds(KP)));
                if (rc != PFMI_OK) return;
                hipLaunchKernelGGL((pf_mixture_mfma_kernel<KP, true>), grid, dim3(MX_THREADS), dyn, c->stream, d, N, K, cpb, d_x,
                                   d_points, c->vh.as<double>(), c->tmat.as<double>(), c->vchol.as<double>(),
                                   c->sqrt_alpha.as<double>(), c->mu.as<double>(), c->logdet.as<double>(), c->status.as<int32_t>(), d_comp);
            } else {
                hipLaunchKernelGGL((pf_mixture_mfma_kernel<KP, false>), grid, dim3(MX_THREADS), 0, c->stream, d, N, K, cpb, d_x,
                                   d_points, c->vh.as<double>(), c->tmat.as<double>(), c->vchol.as<double>(),
                                   c->sqrt_alpha.as<double>(), c->mu.as<double>(), c->logdet.as<double>(), c->status.as<int32_t>(), d_comp);
            }
        });
        PF_CHECK(ok, PFMI_ERR_UNSUPPORTED, "unsupported kpad %d", kp);
        PF_TRY(rc);
    }
    PF_HIP(hipGetLastError());
    return PFMI_OK;
}

// comp [K][N] and lse [N] from X (d, N) for the K fit points d_points (device, int32, validated by the caller)
int32_t pf_launch_mixture_logpdf(pfmi_ctx *c, int K, const int32_t *d_points, int64_t N, const double *d_x, double *d_lse,
                                 double *d_comp) {
    pf_kernel_begin(c);
    PF_TRY(pf_launch_mixture_comp(c, K, d_points, N, d_x, d_comp));
    pf_kernel_end(c, "mixture_logpdf");
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_mixture_lse_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, N, K, d_comp, d_lse);
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "mixture_lse");
    return PFMI_OK;
}
