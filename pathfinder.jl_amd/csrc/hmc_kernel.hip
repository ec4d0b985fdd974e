// hmc_kernel.hip -- static HMC for DEVICE_CALLBACK targets that carry a value-and-gradient closure (pfmi_set_target_gradient), with the
// Woodbury factor of one fitted point as each chain's metric (the reference's "use Pathfinder's metric estimate for sampling",
// docs/src/examples/initializing-hmc.md, ext/PathfinderAdvancedHMCExt.jl:17-23).
//
// The function is the user's, so -- as in lbfgs_closure_kernel.hip -- the run is cut into ROUNDS: one call of the closure on all K
// columns of X, then one launch of pf_hmc_step_kernel (one workgroup per chain).  The round count is known up front (1 + T Lf: the
// start points, then Lf evaluations per transition), so the host enqueues everything and never waits.
//
// The fit is Sigma = L R, R = L': L = PFMI_OP_UNWHITEN, R = PFMI_OP_RMUL (modes 0 and 2 of pf_woodbury_kernel), both in the compact-WY
// form Q = I - Vh T Vh'.  The momentum is carried whitened, v = R p ~ N(0, I): the refresh needs no operator, the kinetic energy is
// |v|^2 / 2, a kick is v += e R grad logp and a drift x += e L v.
//
// A launch of chain k
//   * reads its column of the closure's output (logp, grad at the trial point it wrote in the previous launch),
//   * forms wt = R grad:  z = s . grad, w = Vh'z (block reduction 1), tv = T'w, y = z - Vh tv, head <- V head (hm_apply_R, hmc_rows.h),
//   * finishes the pending kick with it (a full one inside a trajectory, a half one at its end),
//   * at a trajectory's end sums |v|^2 (one more reduction), decides, records row t, draws the next momentum, gives it its first half
//     kick and takes |v|^2 of the fresh normals along in the reduction of the drift,
//   * applies L to v:  z = [V'v_head; v_tail], w = Vh'z (block reduction 2), tv = T w, and writes x~ + e s . (z - Vh tv) into column k of X.
//     (hm_apply_L, hmc_rows.h: both passes, the thread count, the LDS budget and the launch helper are shared with nuts_kernel.hip)
// The chain's rows of Vh are kept in LDS once per launch when they fit (RES): the first pass reads them from HBM and leaves each thread's
// rows in its own LDS slots, so that the other three passes (the second half of R, both halves of L) do not read HBM again.
//
// Every control-flow scalar comes out of a fixed-order block reduction (pf_block_sum_mv / pf_block_sum1_pp: six butterfly steps inside a
// wave, then the waves' partials in wave order, read back from LDS by every thread): all threads of a chain take the same branch, and a
// chain's output depends on nothing but its own inputs.
#include "pfmi_common.h"
#include "hmc_rows.h"
#include "hmc_target.h"
#include <float.h>
#include <type_traits>

enum { HM_OPEN = -1, HM_START = 0 };   // HmChain::i: open a trajectory without reading the closure; the start point is being evaluated;
                                       // 1 .. Lf: the leapfrog evaluation the next launch consumes

struct HmChain {                       // per-chain scalar state (HBM); read by every thread, written back by thread 0
    double lp, H0;
    int64_t t;                         // transitions made so far = draw index of the next momentum
    int32_t i, bad, dead, pad_;
};

struct HmArgs {
    int d, K, nleap, record;
    int64_t t0, t_end, T;              // this call records transitions t0 .. t_end - 1 as rows 0 .. T - 1
    int64_t round;                     // index of this launch among the call's closure rounds (row of the recorded path)
    const int32_t *pts;                // [K] fit point of each chain
    const uint64_t *seeds;             // [K]
    double *eps;                       // [K]; a warm-up launch that ends a transition writes the chain's next step size
    const double *x0;                  // [K][d] (init kernel)
    double *X;                         // closure input: d x K column-major
    const double *out;                 // closure output: logp [K], then grad [K][d]
    double *x, *wg, *wt, *v;           // [K][d]: state, R grad logp(x), R grad at the trial point (scratch), whitened momentum
    HmChain *st;                       // [K]
    double *draws, *rlp, *racc, *rde;  // records [K][T][d], [K][T]
    int32_t *rdiv;
    double *pX, *pout, *pv;            // PFMI_HMC_RECORD_PATH: [rounds][K][d], [rounds][K + K d], [rounds][K][d]
    const double *vh, *tmat, *vchol, *sqa;
    PfAdapt *ad;                       // adaptive runs: [K] adaptation states, then the warm-up traces PfWarmRow [K][t0]
};

#ifndef PF_CHAIN_METRIC_TU
__global__ __launch_bounds__(HM_NT) void pf_hmc_init_kernel(HmArgs A) {
    const int k = blockIdx.x, d = A.d;
    hm_copy_start(A.x0 + (size_t)k * d, A.X + (size_t)k * d, A.x + (size_t)k * d, d);
    if (threadIdx.x == 0) {
        HmChain S = {};
        S.i = HM_START;
        A.st[k] = S;
    }
}
#endif

// ADAPT (pf_hmc_warm_kernel): transitions t < t0 are the warm-up.  They write no row but a PfWarmRow, and thread 0 applies pf_adapt_update
// between recording transition t and opening transition t + 1, whose first half kick and drift already use the new step size.
//
// MODE HM_METRIC (pf_hmc_metric_kernel, hmc_metric_kernel.hip): the chain carries a per-coordinate scale c (HmMetric, hmc_rows.h): a kick is
// v += e c . (R g), a drift x += e L (c . v) -- wg, wt and v themselves stay what they are without a scale, so a new scale needs no
// conversion of the state -- and a warm-up transition inside a metric window ends with hm_metric_end.  Plain and adaptive runs share it.
//
// MODE HM_CHEES (pf_chees_step_kernel, chees_kernel.hip): the step size and the trajectory length are the run's shared ones (A.C, adapt.h:
// PfChees), the leapfrog count of transition t is pf_chees_leapfrog's -- the same in every chain, so the chains end their trajectories in
// the same launch.  A warm-up transition ends with the inputs of the cross-chain update (the state before it, the trial point, a and
// u' = L v') and does NOT open the next trajectory: the update's launches follow, then a launch with A.reopen that opens it.  A launch
// that finds its chain idle returns at once.  Workgroup 0 alone writes L_t, the status bits and the progress word.
enum { HM_PLAIN = 0, HM_WARM = 1, HM_METRIC = 2, HM_CHEES = 3 };

//
// ONE ROUND (hm_round) is what a launch of the step kernels does.  TG == HM_TG_NONE (the step kernels): the round reads the chain's scalar
// state and step size, consumes the closure's output and writes the state back.  TG a built-in target (pf_hmc_fused_kernel,
// hmc_fused_kernel.hip: HM_TG_FUNNEL or the Gaussian family's rank padding): the kernel enters the round once per trip of its loop; the
// round evaluates the target itself where a step kernel reads the closure's output (hm_target_eval, hmc_target.h; a trip that only opens a
// trajectory evaluates nothing), and the CALLER loads S and eps before the first trip and stores S after the last.  What a trip carries to
// the next is HmCarry: S, the step size (a warm-up transition's end changes it), `staged` (the factor rows are in LDS: staged ONCE per
// launch), the ping-pong side `flip` of the reduction buffers and `round`, the row of the recorded path.  The chain's vectors stay in HBM.
struct HmCarry { HmChain S; double eps; int64_t round; int flip; bool staged; };
template <int KPAD, bool RES, int MODE, int TG, class Args>
__device__ __forceinline__ void hm_round(const Args &A, HmCarry &C) {
    constexpr bool ADAPT = MODE != HM_PLAIN, METRIC = MODE == HM_METRIC, CHEES = MODE == HM_CHEES, FUSED = TG != HM_TG_NONE;
    // KPAD sums + one rider, padded to the multiple of 4 pf_block_sum_mv takes; FUSED: or the evaluation's reduction, if that is wider
    constexpr int NVM = FUSED && HmTargetShape<TG>::NV > KPAD + 4 ? HmTargetShape<TG>::NV : KPAD + 4;
    // (the kernel's one LDS object is declared where it is used: handed on by reference it would lose its address space)
    __shared__ std::conditional_t<FUSED, HmTargetLds<KPAD, NVM, TG>, HmLds<KPAD, NVM>> L;
    const int k = blockIdx.x, tid = threadIdx.x, d = A.d, K = A.K;
    int flip = 0;
    HmChain S;
    if constexpr (FUSED) { flip = C.flip; S = C.S; } else S = A.st[k];
    const int p = A.pts[k];
    const size_t kd = (size_t)k * d;
    const double *gVh = A.vh + (size_t)p * d * KPAD, *T = A.tmat + (size_t)p * KPAD * KPAD, *Vc = A.vchol + (size_t)p * KPAD * KPAD;
    const double *sqa = A.sqa + (size_t)p * d;
    double *X = A.X + kd, *x = A.x + kd, *wg = A.wg + kd, *wt = A.wt + kd, *v = A.v + kd;
    double eps;
    if constexpr (FUSED) eps = C.eps; else eps = A.eps[k];
    [[maybe_unused]] int64_t round = 0;
    if constexpr (FUSED) round = C.round;
    int nleap = A.nleap;
    [[maybe_unused]] bool clamped = false, ended = false, warm_end = false;
    [[maybe_unused]] size_t uo = kd;                     // CHEES: the chain's place among the vectors of the update this transition may end with
    if constexpr (CHEES) {
        // (the shared state is read beside the chain's own, before the branch: one load latency, not two in a row)
        const double ceps = A.C->eps, ctau = A.C->tau;
        const int32_t cLmax = A.C->Lmax;
        if (A.reopen ? (S.i != HM_OPEN || S.t >= A.t_end) : S.i == HM_OPEN) return;      // (the same in every thread and every chain)
        if (A.nrec > 1) uo += (size_t)S.t * A.vec;
        eps = ceps;
        nleap = pf_chees_leapfrog(S.t, ctau, ceps, cLmax, &clamped);
        if (k == 0 && tid == 0 && !A.reopen) {           // the chains run in lockstep: chain 0 speaks for the run
            // The progress word, by its single writer.  What this launch leaves is known before its work (it ends a trajectory iff
            // i has reached L_t), so the store to the page-locked word is issued first and its latency runs beside the passes.  Low
            // word: 0 idle, else 1, + 2 while warm-up transitions (and so cross-chain updates) are still to come.  Relaxed: the host
            // schedules by the word alone and reads results only behind a stream synchronisation.
            const bool ends = S.i != HM_START && S.i >= nleap;
            const int64_t tn = S.t + (ends ? 1 : 0);
            const bool running = !(ends && tn >= A.t_end);
            __hip_atomic_store(A.h_status, (int64_t)((A.pround << 32) | (running ? (tn < A.t0 ? 3 : 1) : 0)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    const uint64_t seed = A.seeds[k];
    const HmFactor F = {gVh, T, Vc, sqa};
    bool staged = false;                                 // a pass of this launch has left the factor rows in LDS (hmc_rows.h)
    if constexpr (FUSED) staged = C.staged;
    if constexpr (TG > 0) if (!staged) hm_target_stage<TG>(A.tg, L);     // G, once per launch: the first trip's first barrier publishes it
    bool open = S.i == HM_OPEN, drift = false;
    // METRIC: the chain's scale; c_i w of a kick is hm_scaled's (row i is the calling thread's own)
    const double *sc = nullptr;
    if constexpr (METRIC) sc = A.M.scale + kd;
    if (S.i != HM_OPEN) {
        double lpt;
        if constexpr (FUSED) lpt = hm_target_eval<TG, NVM>(A.tg, L, X, A.gout + K + kd, d, flip);
        else lpt = A.out[k];
        const double *g = A.out + K + kd;
        if (A.record) {                                  // what the closure saw and what it answered, before X is rewritten
            const int64_t rnd = FUSED ? round : A.round;
            double *pX = A.pX + ((size_t)rnd * K + k) * d, *pout = A.pout + (size_t)rnd * ((size_t)K * (d + 1));
            for (int i = tid; i < d; i += HM_NT) { pX[i] = X[i]; pout[K + kd + i] = g[i]; }
            if (tid == 0) pout[k] = lpt;
        }
        const double nbad = hm_apply_R<KPAD, RES, HM_NT, NVM>(F, L, g, d, flip, [&](int i) -> double & { return wt[i]; }, FUSED && staged);
        staged = true;
        // ---- the pending kick
        if (S.i == HM_START) {
            const bool bad = nbad > 0.0 || !isfinite(lpt);       // a start point the chain cannot leave: reported by pfmi_hmc_wait
            for (int i = tid; i < d; i += HM_NT) wg[i] = bad ? 0.0 : wt[i];
            S.lp = bad ? -DBL_MAX : lpt;
            S.dead = bad ? 1 : 0;
            open = true;
        } else if (S.i < nleap) {
            for (int i = tid; i < d; i += HM_NT) v[i] = fma(eps, hm_scaled<METRIC>(sc, i, wt[i]), v[i]);
            if (nbad > 0.0 || !isfinite(lpt)) S.bad = 1;
            ++S.i;
            drift = true;
        } else {
            // ---- the trajectory's end: last half kick, H1, the decision, row t
            double e = 0.0;
            for (int i = tid; i < d; i += HM_NT) {
                const double vi = fma(0.5 * eps, hm_scaled<METRIC>(sc, i, wt[i]), v[i]);
                e = fma(vi, vi, e);
                if constexpr (CHEES) v[i] = vi;          // v' of the update (row i is this thread's own in every pass)
            }
            e = pf_block_sum1_pp<NVM>(e, L.red, flip);
            const double H1 = -lpt + 0.5 * e, dH = H1 - S.H0;
            const bool div = S.bad || nbad > 0.0 || !isfinite(lpt) || !isfinite(H1) || dH > 1000.0;
            const double a = div ? 0.0 : fmin(1.0, exp(-dH));
            const double u = (double)(pf_rand_u64(seed, (uint64_t)S.t, PF_RNG_STREAM_HMC_ACCEPT) >> 11) * 0x1p-53;
            const bool acc = u < a;
            const int64_t row = S.t - A.t0;
            const bool warm = ADAPT && row < 0;
            double *dr = A.draws + ((size_t)k * A.T + (warm ? 0 : row)) * d;
            for (int i = tid; i < d; i += HM_NT) {
                double xi = x[i];
                if constexpr (CHEES) if (warm) { A.ux[uo + i] = xi; A.uxp[uo + i] = X[i]; }
                if (acc) { xi = X[i]; x[i] = xi; wg[i] = wt[i]; }
                if (!warm) dr[i] = xi;
            }
            if (acc) S.lp = lpt;
            if (tid == 0 && !warm) {
                const size_t r = (size_t)k * A.T + row;
                A.rlp[r] = S.lp; A.racc[r] = a; A.rde[r] = isfinite(dH) ? dH : DBL_MAX; A.rdiv[r] = div ? 1 : 0;
            }
            ++S.t; S.bad = 0;
            if constexpr (CHEES) {
                ended = true; warm_end = warm;
                if (warm) {
                    if (tid == 0) {
                        PfWarmRow *tr = reinterpret_cast<PfWarmRow *>(A.ad + K) + (size_t)k * A.t0 + (S.t - 1);
                        tr->eps = eps; tr->acc = a; tr->div = div ? 1 : 0; tr->nleap = nleap;
                        A.ua[k] = a;
                    }
                    // u' = L v': the drift's pass with a base of 0 and e = 1
                    hm_apply_L<KPAD, RES, HM_NT, NVM>(F, L, A.uv + uo, 1.0, 0.0, staged, d, flip, [&](int i) -> const double & { return v[i]; },
                                                      [&](int) { return 0.0; }, [&](double) {});
                }
            } else if constexpr (ADAPT) {
                if (warm) {
                    __shared__ double sNext;
                    bool wnd = false;                    // METRIC: the transition ended a metric window
                    if constexpr (METRIC)
                        wnd = hm_metric_end<KPAD, RES, NVM>(F, L, A.M, A.ad, k, d, S.t - 1, A.x0 + kd, flip, [&](int i) { return x[i]; });
                    if (tid == 0) {
                        sNext = hm_warm_end(A.ad, A.eps, K, k, S.t, A.t0, eps, a, div ? 1 : 0, nleap);
                        if constexpr (METRIC) if (wnd) pf_adapt_restart(A.ad[k], sNext);
                    }
                    __syncthreads();
                    eps = sNext;
                }
            }
            if (S.t < A.t_end && !(CHEES && warm)) open = true; else S.i = HM_OPEN;
        }
    }
    double vv0 = 0.0;
    if (open) {
        // ---- the next trajectory: fresh momentum (draw index t of the chain's seed), first half kick
        const uint32_t n = (uint32_t)S.t;
        for (int i = tid; i < d; i += HM_NT) {
            const double z = hm_normal(seed, n, i);
            vv0 = fma(z, z, vv0);
            v[i] = fma(0.5 * eps, hm_scaled<METRIC>(sc, i, wg[i]), z);
        }
        S.i = 1;
        drift = true;
    }
    if (drift) {
        const double *base = open ? x : X;
        if constexpr (METRIC) {
            hm_apply_L<KPAD, RES, HM_NT, NVM>(F, L, X, eps, vv0, staged, d, flip, [&](int i) { return sc[i] * v[i]; }, [&](int i) { return base[i]; },
                                              [&](double vv) { if (open) S.H0 = -S.lp + 0.5 * vv; });
        } else {
            hm_apply_L<KPAD, RES, HM_NT, NVM>(F, L, X, eps, vv0, staged, d, flip, [&](int i) -> const double & { return v[i]; }, [&](int i) { return base[i]; },
                                              [&](double vv) { if (open) S.H0 = -S.lp + 0.5 * vv; });
        }
        if constexpr (FUSED) staged = true;
    }
    if (A.record && (FUSED ? round : A.round) >= 0) {
        double *pv = A.pv + ((size_t)(FUSED ? round : A.round) * K + k) * d;
        for (int i = tid; i < d; i += HM_NT) pv[i] = v[i];
    }
    if constexpr (FUSED) { C = {S, eps, round + 1, flip, staged}; return; }
    __syncthreads();                                     // every thread has read S before thread 0 writes
    if (tid == 0) A.st[k] = S;
    if constexpr (CHEES) {
        if (k == 0 && tid == 0 && !A.reopen) {
            if (ended) {
                A.nl[S.t - 1 - A.tcall] = nleap;
                if (clamped) A.C->status |= PF_CHEES_CLAMPED;
                if (warm_end) { A.C->pending = 1; A.C->t_upd = S.t - 1; }
            }
            if (S.i == HM_OPEN && S.t >= A.t_end) A.C->fin_round = A.pround;
        }
    }
}

// one launch of the step kernels: one round on the chain's state in HBM
template <int KPAD, bool RES, int MODE, class Args>
__device__ __forceinline__ void hm_step_body(const Args &A) {
    HmCarry none;                                        // (not read, not written)
    hm_round<KPAD, RES, MODE, HM_TG_NONE>(A, none);
}

#ifndef PF_CHAIN_METRIC_TU             // (hmc_metric_kernel.hip takes the body and hm_args from this file and defines its own kernels)
template <int KPAD, bool RES>
__global__ __launch_bounds__(HM_NT) void pf_hmc_step_kernel(HmArgs A) { hm_step_body<KPAD, RES, HM_PLAIN>(A); }

template <int KPAD, bool RES>
__global__ __launch_bounds__(HM_NT) void pf_hmc_warm_kernel(HmArgs A) { hm_step_body<KPAD, RES, HM_WARM>(A); }
#endif

// ---------------------------------------------------------------------------------------------------
static HmArgs hm_args(pfmi_ctx *c, int64_t round) {
    const HmcState &H = c->hmc;
    HmArgs A;
    A.d = c->d; A.K = H.K; A.nleap = H.nleap; A.record = H.record ? 1 : 0;
    A.t0 = H.t0; A.t_end = H.t0 + H.T; A.T = H.T; A.round = round;
    A.pts = c->hm_pts.as<int32_t>(); A.seeds = c->hm_seeds.as<uint64_t>(); A.eps = c->hm_eps.as<double>(); A.x0 = c->hm_x0.as<double>();
    A.X = c->hm_X.as<double>(); A.out = c->hm_out.as<double>();
    A.x = c->hm_x.as<double>(); A.wg = c->hm_wg.as<double>(); A.wt = c->hm_wt.as<double>(); A.v = c->hm_v.as<double>();
    A.st = c->hm_st.as<HmChain>();
    A.draws = c->hm_draws.as<double>(); A.rlp = c->hm_lp.as<double>(); A.racc = c->hm_acc.as<double>(); A.rde = c->hm_de.as<double>();
    A.rdiv = c->hm_div.as<int32_t>();
    A.pX = c->hm_pX.as<double>(); A.pout = c->hm_pout.as<double>(); A.pv = c->hm_pv.as<double>();
    A.vh = c->vh.as<double>(); A.tmat = c->tmat.as<double>(); A.vchol = c->vchol.as<double>(); A.sqa = c->sqrt_alpha.as<double>();
    A.ad = c->hm_adapt.as<PfAdapt>();
    return A;
}

#ifndef PF_CHAIN_METRIC_TU
size_t pf_hmc_chain_bytes() { return sizeof(HmChain); }

int32_t pf_launch_hmc_init(pfmi_ctx *c, hipStream_t s) {
    hipLaunchKernelGGL(pf_hmc_init_kernel, dim3(c->hmc.K), dim3(HM_NT), 0, s, hm_args(c, 0));
    PF_HIP(hipGetLastError());
    return PFMI_OK;
}

struct HmFamily {
    static constexpr bool has_warm = true;
    template <int KPAD, bool RES, bool ADAPT>
    static auto kernel() { return ADAPT ? &pf_hmc_warm_kernel<KPAD, RES> : &pf_hmc_step_kernel<KPAD, RES>; }
};

// the dying chains' start flags: dead[k] != 0 when chain k's start point had a non-finite log density or gradient
int32_t pf_hmc_dead_flags(pfmi_ctx *c, std::vector<int32_t> &dead) {
    const int K = c->hmc.K;
    std::vector<HmChain> st((size_t)K);
    PF_HIP(hipMemcpyAsync(st.data(), c->hm_st.p, sizeof(HmChain) * K, hipMemcpyDeviceToHost, c->stream));
    PF_HIP(hipStreamSynchronize(c->stream));
    dead.resize((size_t)K);
    for (int k = 0; k < K; ++k) dead[(size_t)k] = st[(size_t)k].dead;
    return PFMI_OK;
}

int32_t pf_launch_hmc_step(pfmi_ctx *c, int64_t round, hipStream_t s) { return hm_launch_step<HmFamily>(c, "hmc", hm_args(c, round), s); }
#endif
