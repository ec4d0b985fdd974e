// hmc_rows.h -- what the chain kernels (hmc_kernel.hip: static HMC, nuts_kernel.hip: NUTS) share, each stated ONCE here: the launch
// geometry and the LDS budget (HM_NT, HM_LDS_RES, pf_hmc_resident), the launch of a kernel family (hm_launch_step), the momentum normals,
// the two Woodbury passes of a step (hm_apply_R: wt = R g, both kernels; hm_apply_L: X <- base + e L v, static HMC -- NUTS keeps its copy
// written out, nuts_kernel.hip says why), the start-point copy of the init kernels and the end of a warm-up transition (hm_warm_end); for the
// metric kernels the third pass (hm_whiten: u = L \ dx) and what a window transition does with it (hm_metric_end).
#pragma once
#include "pfmi_common.h"
#include "adapt.h"

#define HM_NT 256                      // threads per chain (4 waves)
#define HM_NW (HM_NT / 64)
#define HM_LDS_RES (150 * 1024)        // most dynamic LDS the staged factor rows may take (of 160 KB, beside the kernels' static buffers)

// The most rounds one launch of the fused static-HMC kernel (hmc_fused_kernel.hip) makes: a longer call is several launches that re-enter
// from the chains' resident state.  Bounds the time one kernel holds the GPU; the test hook PFMI_HMC_FUSED_ROUNDS overrides it.
#define HM_FUSED_ROUNDS 1024

// the staged factor rows of one chain fit in LDS beside the reduction buffers
inline bool pf_hmc_resident(int d, int kpad) { return (size_t)d * kpad * sizeof(double) <= (size_t)HM_LDS_RES; }

// c->hm_chees of a ChEES call (adapt.h: PfChees), stated ONCE, in doubles from the buffer's start: the shared state (PF_CHEES_HEAD bytes),
// the traces tau, g, hm [W] each, the update's inputs a [K] and its sums p, q, r [K] each, xbar and xbar' [d] each, the vectors x, x' and u'
// of an update [nrec][K][d] each (nrec = W under PFMI_CHEES_RECORD_UPDATE, else 1 when W > 0), then L_t int32 [W + T]
#define PF_CHEES_HEAD 256
static_assert(sizeof(PfChees) <= PF_CHEES_HEAD, "the shared state fits its slot");
struct CheesLayout {
    size_t trace, ua, pqr, xbar, upd, nl, bytes, vec;
    CheesLayout(int K, int d, int64_t W, int64_t T, int64_t nrec) {
        vec = (size_t)K * d;
        trace = PF_CHEES_HEAD / sizeof(double);
        ua = trace + 3 * (size_t)W;
        pqr = ua + (size_t)K;
        xbar = pqr + 3 * (size_t)K;
        upd = xbar + 2 * (size_t)d;
        nl = upd + 3 * vec * (size_t)nrec;
        bytes = sizeof(double) * nl + sizeof(int32_t) * (size_t)(W + T);
    }
};

#ifdef __HIPCC__
// One step launch of a kernel family (Family::kernel<KPAD, RES, ADAPT>() is its step or warm kernel; Args carries d and K): one workgroup
// per chain, the factor rows in dynamic LDS when they fit, counted under the plan name "<plan>[_adapt]:<KPAD>:<res|stream>".  (A family
// without a warm kernel of its own -- has_warm false: the metric kernels -- serves plain and adaptive runs under one plan name.)
template <class Family, class Args>
static int32_t hm_launch_step(pfmi_ctx *c, const char *plan, const Args &A, hipStream_t s) {
    const bool res = pf_hmc_resident(A.d, c->kpad), adapt = Family::has_warm && c->hmc.adapting;
    auto go = [&](auto KP, auto RES, auto AD) -> int32_t {
        auto *kern = Family::template kernel<KP(), RES(), AD()>();
        if (RES()) PF_TRY(pf_raise_lds_limit(c, reinterpret_cast<const void *>(kern), HM_LDS_RES));
        char name[32];
        snprintf(name, sizeof name, "%s%s:%d:%s", plan, AD() ? "_adapt" : "", KP(), RES() ? "res" : "stream");
        ++c->hmc_plans[name];
        hipLaunchKernelGGL(kern, dim3(A.K), dim3(HM_NT), RES() ? (size_t)A.d * KP() * sizeof(double) : 0, s, A);
        return PFMI_OK;
    };
    int32_t rc = PFMI_OK;
    const bool ok = pf_dispatch_kpad<4, 8, 12, 16, 20, 32, 64>(c->kpad, [&](auto KP) {
        const std::true_type Y;
        const std::false_type N;
        rc = res ? (adapt ? go(KP, Y, Y) : go(KP, Y, N)) : (adapt ? go(KP, N, Y) : go(KP, N, N));
    });
    PF_CHECK(ok, PFMI_ERR_UNSUPPORTED, "unsupported kpad %d", c->kpad);
    PF_TRY(rc);
    PF_HIP(hipGetLastError());
    return PFMI_OK;
}

// the standard normal of row i of draw n under `seed`: the value pf_randn4(seed, i / 4, n, stream 0) gives row i (full table in global
// memory: the same values as the LDS copy's)
__device__ __forceinline__ double hm_normal(uint64_t seed, uint32_t n, int i) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), g = (uint32_t)i >> 2, q = (uint32_t)i & 3u;
    uint32_t x[4];
    pf_philox_normals(n, g, 0u, 0u, k0, k1, x);
    const uint32_t xw = q == 0 ? x[0] : q == 1 ? x[1] : q == 2 ? x[2] : x[3];
    uint32_t x2w = 0u;
    if ((xw & 0x7FFFFFFFu) < (1u << PF_ICDF_TAILBITS)) {
        uint32_t x2[4];
        pf_philox_normals(n, g, 0u, 1u, k0, k1, x2);
        x2w = q == 0 ? x2[0] : q == 1 ? x2[1] : q == 2 ? x2[2] : x2[3];
    }
    return pf_icdf_any(xw, x2w);
}

// w[j] += row[j] z and y - row . tv, KPAD columns in groups of 4 (one 32-byte load each)
template <int KPAD, int NV, bool KEEP>
__device__ __forceinline__ void hm_row_axpy(const double *row, double *keep, double z, double (&w)[NV]) {
#pragma unroll
    for (int c = 0; c < KPAD; c += 4) {
        const double4 r = *reinterpret_cast<const double4 *>(row + c);
        if (KEEP) *reinterpret_cast<double4 *>(keep + c) = r;           // the thread's own LDS copy of the row, for the later passes
        w[c] = fma(r.x, z, w[c]); w[c + 1] = fma(r.y, z, w[c + 1]); w[c + 2] = fma(r.z, z, w[c + 2]); w[c + 3] = fma(r.w, z, w[c + 3]);
    }
}
template <int KPAD>
__device__ __forceinline__ double hm_row_sub(const double *row, const double *tv, double y) {
#pragma unroll
    for (int c = 0; c < KPAD; c += 4) {
        const double4 r = *reinterpret_cast<const double4 *>(row + c);
        y = fma(-r.x, tv[c], y); y = fma(-r.y, tv[c + 1], y); y = fma(-r.z, tv[c + 2], y); y = fma(-r.w, tv[c + 3], y);
    }
    return y;
}

// What the two passes read of a chain: its fit point's factor (rows gVh [d][KPAD] in HBM, T, V's Cholesky factor Vc, the scaling sqa) ...
struct HmFactor {
    const double *gVh, *T, *Vc, *sqa;
};
// ... and the static LDS the kernel declares for them: the ping-pong buffers of the block reductions (NRED: the widest reduction of the
// kernel) and three KPAD-long vectors.  The passes name the members of the kernel's one object: an LDS array handed on as a plain pointer
// loses its address space, and a store to it is merged with the store to HBM in the other branch into one flat store of a selected address.
// (Lds of the passes: this struct, or a kernel's own with the same members -- the NUTS kernel orders them differently)
template <int KPAD, int NRED>
struct HmLds {
    alignas(16) double red[2 * HM_NW * NRED];
    alignas(16) double sHead[KPAD], sZ[KPAD], sTv[KPAD];       // (16 bytes: two doubles per LDS access, as for separate arrays)
};
// RES: the chain's factor rows [d][KPAD] in dynamic LDS.  A thread reads only the rows it owns (i = tid, tid + NT, ...), in every pass.  The
// first pass over the factor reads them from HBM and leaves them in LDS; the later ones read the thread's own copy: no staging pass, no
// barrier.
#define HM_STAGED_ROWS extern __shared__ __attribute__((aligned(32))) double sVh[]

// wt = R g: z = s . g, w = Vh'z (one block reduction), tv = T'w, y = z - Vh tv, head <- V head.  wt(i) is the caller's element i of the
// result (double &).  Returns the number of non-finite entries of g.  With RES this pass stages the rows, unless an earlier pass of the
// launch has (staged: the fused kernel, hmc_fused_kernel.hip, makes many rounds in one launch and stages once).
template <int KPAD, bool RES, int NT, int NRED, class Lds, class Wt>
__device__ __forceinline__ double hm_apply_R(const HmFactor &F, Lds &L, const double *g, int d, int &flip, Wt wt, bool staged = false) {
    HM_STAGED_ROWS;
    constexpr int NVM = KPAD + 4;                        // KPAD sums + one rider, padded to the multiple of 4 pf_block_sum_mv takes
    const int tid = threadIdx.x;
    double w[NVM];
#pragma unroll
    for (int j = 0; j < NVM; ++j) w[j] = 0.0;
    const double *rows = RES ? sVh : F.gVh;
    if (RES && !staged) {
        for (int i = tid; i < d; i += NT) {
            const double gi = g[i], zi = F.sqa[i] * gi;
            hm_row_axpy<KPAD, NVM, true>(F.gVh + (size_t)i * KPAD, sVh + (size_t)i * KPAD, zi, w);
            w[KPAD] += isfinite(gi) ? 0.0 : 1.0;
        }
    } else {
        for (int i = tid; i < d; i += NT) {
            const double gi = g[i], zi = F.sqa[i] * gi;
            hm_row_axpy<KPAD, NVM, false>(rows + (size_t)i * KPAD, nullptr, zi, w);
            w[KPAD] += isfinite(gi) ? 0.0 : 1.0;
        }
    }
    pf_block_sum_mv<NVM, NRED>(w, L.red, flip);
    const double nbad = w[KPAD];
    if (tid < KPAD) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < KPAD; ++b) if (b <= tid) s = fma(F.T[b * KPAD + tid], w[b], s);
        L.sTv[tid] = s;
    }
    __syncthreads();
    for (int i = tid; i < d; i += NT) {
        const double y = hm_row_sub<KPAD>(rows + (size_t)i * KPAD, L.sTv, F.sqa[i] * g[i]);
        if (i < KPAD) L.sHead[i] = y; else wt(i) = y;
    }
    if (tid < KPAD && tid >= d) L.sHead[tid] = 0.0;
    __syncthreads();
    if (tid < KPAD && tid < d) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < KPAD; ++b) if (b >= tid) s = fma(F.Vc[tid * KPAD + b], L.sHead[b], s);
        wt(tid) = s;                                     // (row tid is thread tid's own: every thread reads back only rows it wrote)
    }
    return nbad;
}

// X <- base + e L v: z = [V'v_head; v_tail], w = Vh'z (one block reduction), tv = T w, y = s . (z - Vh tv).  v(i) and base(i) are the
// caller's elements i (v: const double &).  `rider` is summed over the block along with w; summed(total) is called once the sums are
// there.  staged: an R pass came before in this launch (it did not in the opening launch of a CONTINUE, where this pass stages the rows).
template <int KPAD, bool RES, int NT, int NRED, class Lds, class Vv, class Base, class Summed>
__device__ __forceinline__ void hm_apply_L(const HmFactor &F, Lds &L, double *X, double e, double rider, bool staged, int d,
                                            int &flip, Vv v, Base base, Summed summed) {
    HM_STAGED_ROWS;
    constexpr int NVM = KPAD + 4;
    const int tid = threadIdx.x;
    const double *rows = RES ? sVh : F.gVh;
    const auto &sZ = L.sZ;                               // (const: z[i] below is ONE load from a selected address, not two in two branches)
    __syncthreads();                                     // the head product of the R pass has read sHead
    if (tid < KPAD) L.sHead[tid] = tid < d ? v(tid) : 0.0;
    __syncthreads();
    if (tid < KPAD) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < KPAD; ++b) if (b <= tid) s = fma(F.Vc[b * KPAD + tid], L.sHead[b], s);
        L.sZ[tid] = s;
    }
    __syncthreads();
    double w[NVM];
#pragma unroll
    for (int j = 0; j < NVM; ++j) w[j] = 0.0;
    if (RES && !staged) {
        for (int i = tid; i < d; i += NT)
            hm_row_axpy<KPAD, NVM, true>(F.gVh + (size_t)i * KPAD, sVh + (size_t)i * KPAD, i < KPAD ? sZ[i] : v(i), w);
    } else {
        for (int i = tid; i < d; i += NT) hm_row_axpy<KPAD, NVM, false>(rows + (size_t)i * KPAD, nullptr, i < KPAD ? sZ[i] : v(i), w);
    }
    w[KPAD] = rider;
    pf_block_sum_mv<NVM, NRED>(w, L.red, flip);
    summed(w[KPAD]);
    if (tid < KPAD) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < KPAD; ++b) if (b >= tid) s = fma(F.T[tid * KPAD + b], w[b], s);
        L.sTv[tid] = s;
    }
    __syncthreads();
    for (int i = tid; i < d; i += NT) {
        const double y = hm_row_sub<KPAD>(rows + (size_t)i * KPAD, L.sTv, i < KPAD ? sZ[i] : v(i));
        X[i] = fma(e, F.sqa[i] * y, base(i));
    }
}

// u = L \ dx (PFMI_OP_WHITEN): z = dx / s, w = Vh'z (one block reduction), tv = T'w, y = z - Vh tv, head <- V'^-1 head.  dx(i) is the
// caller's element i; use(i, u_i) is called once per element by the thread that owns row i (head row i: thread i).  An R pass came
// before in the launch, so with RES the rows are staged.
// The head solve is wave 0's, lane a holding y_a (V upper triangular, the identity beyond the fit's columns), for a = 0 .. KPAD - 1 in turn:
//     u_a = y_a / V[a][a];      y_b <- fma(-V[a][b], u_a, y_b) for every b > a
// i.e. u_a = ((..((y_a - V[0][a] u_0) - V[1][a] u_1) ..) - V[a-1][a] u_{a-1}) / V[a][a]: a fused multiply-adds in the order b = 0 .. a - 1,
// then one division.
template <int KPAD, bool RES, int NT, int NRED, class Lds, class Dx, class Use>
__device__ __forceinline__ void hm_whiten(const HmFactor &F, Lds &L, int d, int &flip, Dx dx, Use use) {
    HM_STAGED_ROWS;
    static_assert(KPAD <= 64, "the head solve is one wave's");
    constexpr int NVM = KPAD + 4;
    const int tid = threadIdx.x;
    const double *rows = RES ? sVh : F.gVh;
    double w[NVM];
#pragma unroll
    for (int j = 0; j < NVM; ++j) w[j] = 0.0;
    for (int i = tid; i < d; i += NT) hm_row_axpy<KPAD, NVM, false>(rows + (size_t)i * KPAD, nullptr, dx(i) / F.sqa[i], w);
    pf_block_sum_mv<NVM, NRED>(w, L.red, flip);
    if (tid < KPAD) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < KPAD; ++b) if (b <= tid) s = fma(F.T[b * KPAD + tid], w[b], s);
        L.sTv[tid] = s;
    }
    __syncthreads();
    for (int i = tid; i < d; i += NT) {
        const double y = hm_row_sub<KPAD>(rows + (size_t)i * KPAD, L.sTv, dx(i) / F.sqa[i]);
        if (i < KPAD) L.sHead[i] = y; else use(i, y);
    }
    if (tid < KPAD && tid >= d) L.sHead[tid] = 0.0;
    __syncthreads();
    if (tid < 64) {
        const bool mine = tid < KPAD;
        double y = mine ? L.sHead[tid] : 0.0;
#pragma unroll
        for (int a = 0; a < KPAD; ++a) {
            const double ua = __shfl(y, a) / F.Vc[a * KPAD + a];
            const double vab = (mine && tid > a) ? F.Vc[a * KPAD + tid] : 0.0;       // (no read beyond V's row)
            y = tid == a ? ua : fma(-vab, ua, y);
        }
        if (mine && tid < d) use(tid, y);
    }
}

// c_i w in a metric kernel (a chain with a per-coordinate scale c), w itself in every other
template <bool METRIC>
__device__ __forceinline__ double hm_scaled(const double *c, int i, double w) {
    if constexpr (METRIC) return c[i] * w;
    else return w;
}

// What a chain with a per-coordinate scale reads (the metric kernels: pf_hmc_metric_kernel, pf_nuts_metric_kernel): the scale itself and,
// in a run with metric windows (adapt.h), the windows, the Welford state of the open window and the traces.
struct HmMetric {
    double *scale;                     // [K][d] the chains' resident scale c
    const int32_t *win;                // {number of windows, start of the first, their ends (exclusive)}; null: a run without windows
    double *mean, *m2;                 // [K][d] Welford's running mean and M2 of u over the open window
    double *strace;                    // [K][windows][d] the scale each window left
    double *urec;                      // PFMI_ADAPT_RECORD_WHITENED: [K][nwt][d], the u of every window transition; else null
    int64_t nwt;                       // transitions in windows: the last window's end - the first's start
};
// c->hm_metric of a run with metric windows, stated ONCE: the window table (PF_METRIC_HEAD bytes), mean and M2 [K][d], the scale trace
// [K][nwin][d], then with PFMI_ADAPT_RECORD_WHITENED the rows u [K][nwt][d]
#define PF_METRIC_HEAD 256
static_assert(sizeof(int32_t) * (2 + PF_ADAPT_MAX_WINDOWS) <= PF_METRIC_HEAD, "the window table fits its slot");
inline size_t pf_metric_bytes(int K, int d, int nwin, int64_t nwt_recorded) {
    return PF_METRIC_HEAD + sizeof(double) * (size_t)K * d * (size_t)(2 + nwin + nwt_recorded);
}
inline double *pf_metric_strace(pfmi_ctx *c) { return reinterpret_cast<double *>(c->hm_metric.as<char>() + PF_METRIC_HEAD) + 2 * (size_t)c->hmc.K * c->d; }
inline HmMetric pf_chain_metric_args(pfmi_ctx *c) {
    const HmcState &H = c->hmc;
    HmMetric M = {};
    M.scale = c->hm_scale.as<double>();
    if (H.adapting && H.metric_run && H.nwin > 0) {
        const size_t vec = (size_t)H.K * c->d;
        M.win = reinterpret_cast<const int32_t *>(c->hm_metric.as<char>());
        M.mean = pf_metric_strace(c) - 2 * vec;
        M.m2 = M.mean + vec;
        M.strace = pf_metric_strace(c);
        M.nwt = H.win_ends[H.nwin - 1] - H.win_init;
        M.urec = H.rec_u ? M.strace + vec * (size_t)H.nwin : nullptr;
    }
    return M;
}

// The end of warm-up transition tt of chain k in a metric kernel, before hm_warm_end: inside a window, u = L \ (x - x0) and the Welford
// update of every coordinate; at the window's end the new scale (or the kept one), its trace, and the cleared Welford state.  xs(i):
// element i of the chain's state.  Returns whether a window ended: thread 0 then restarts the dual averaging (pf_adapt_restart).
template <int KPAD, bool RES, int NRED, class Lds, class Xs>
__device__ __forceinline__ bool hm_metric_end(const HmFactor &F, Lds &L, const HmMetric &M, PfAdapt *ad, int k, int d, int64_t tt64,
                                              const double *x0, int &flip, Xs xs) {
    if (!M.win) return false;
    const int tt = __builtin_amdgcn_readfirstlane((int)tt64), nwin = M.win[0], first = M.win[1];
    int j = -1, ws = 0, we = 0;
    for (int q = 0, start = first; q < nwin; ++q) {
        const int e = M.win[2 + q];
        if (tt >= start && tt < e) { j = q; ws = start; we = e; }
        start = e;
    }
    if (j < 0) return false;
    const int tid = threadIdx.x;
    const size_t kd = (size_t)k * d;
    const double n = (double)(tt - ws + 1);
    double *mean = M.mean + kd, *m2 = M.m2 + kd, *c = M.scale + kd;
    double *ur = M.urec ? M.urec + ((size_t)k * M.nwt + (size_t)(tt - first)) * d : nullptr;
    hm_whiten<KPAD, RES, HM_NT, NRED>(F, L, d, flip, [&](int i) { return xs(i) - x0[i]; }, [&](int i, double u) {
        double mi = mean[i], qi = m2[i];
        pf_welford_update(n, u, mi, qi);
        mean[i] = mi; m2[i] = qi;
        if (ur) ur[i] = u;
    });
    if (tt + 1 < we) return false;
    // ---- the window's end (every thread reads back only what it wrote: row i is thread i % HM_NT's in every pass)
    double bad = 0.0;
    for (int i = tid; i < d; i += HM_NT) bad += pf_metric_var_ok(pf_metric_var(n, m2[i])) ? 0.0 : 1.0;
    bad = pf_block_sum1_pp<NRED>(bad, L.red, flip);
    double *st = M.strace + ((size_t)k * nwin + j) * d;
    for (int i = tid; i < d; i += HM_NT) {
        const double ci = bad > 0.0 ? c[i] : sqrt(pf_metric_var(n, m2[i]));
        c[i] = ci; st[i] = ci; mean[i] = 0.0; m2[i] = 0.0;
    }
    if (tid == 0 && bad > 0.0) ad[k].flags |= PF_ADAPT_KEPT_METRIC;
    return true;
}

// the init kernels: the start point becomes the chain's state and the closure's first input
__device__ __forceinline__ void hm_copy_start(const double *x0, double *X, double *x, int d) {
    for (int i = threadIdx.x; i < d; i += HM_NT) { const double v = x0[i]; X[i] = v; x[i] = v; }
}

// The end of warm-up transition t - 1 (t transitions made, t0 of them warm-up), by thread 0 of the chain: its PfWarmRow (ad: [K] adaptation
// states, then the traces [K][t0]), the update on the statistic a, the state and the step size of transition t stored -- exp(le) while t
// is a warm-up transition, exp(leb) after the last one.  Returns that step size.
__device__ __forceinline__ double hm_warm_end(PfAdapt *ad, double *eps_out, int K, int k, int64_t t, int64_t t0, double eps, double a, int div,
                                              int nleap) {
    PfWarmRow *tr = reinterpret_cast<PfWarmRow *>(ad + K) + (size_t)k * t0 + (t - 1);
    tr->eps = eps; tr->acc = a; tr->div = div; tr->nleap = nleap;
    PfAdapt Ad = ad[k];
    const double le = pf_adapt_update(Ad, a);
    const double en = pf_adapt_pick(Ad, t < t0 ? le : Ad.leb, eps);
    ad[k] = Ad; eps_out[k] = en;
    return en;
}
#endif
