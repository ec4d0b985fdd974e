// nuts_kernel.hip -- the No-U-Turn sampler for DEVICE_CALLBACK targets that carry a value-and-gradient closure, with the Woodbury factor of
// one fitted point as each chain's metric (the reference hands Pathfinder's metric to a NUTS sampler: docs/src/examples/initializing-hmc.md,
// ext/PathfinderAdvancedHMCExt.jl, ext/PathfinderDynamicHMCExt.jl).  Multinomial NUTS (Betancourt 2017) with the ITERATIVE tree builder:
// checkpoints instead of recursion (Phan, Pradhan & Jankowiak 2019, "Composable effects for flexible and accelerated probabilistic
// programming in NumPyro"; Lao & Dillon 2019, "Unrolled implementation of No-U-Turn Sampler").
//
// What a step shares with static HMC is hmc_rows.h: the R pass (hm_apply_R), the thread count, the LDS budget, the launch helper and the end
// of a warm-up transition.  The L pass is static HMC's statement for statement but stays written out here (see the rule for the base
// addresses in nt_round).  pf_nuts_fused_kernel (nuts_fused_kernel.hip) enters the same round once per trip of its loop.
//
// As in hmc_kernel.hip the run is cut into ROUNDS: one call of the closure on all K columns of X, then one launch of pf_nuts_step_kernel (one
// workgroup per chain), which consumes the evaluation -- exactly ONE leapfrog step of every running chain -- and writes the next trial
// point.  The round count is not known up front, so the rounds are scheduled as the closure L-BFGS's are (lbfgs_closure_kernel.hip): a few
// in flight, the last workgroup of a launch publishes (round << 32 | chains still running) to a page-locked word, the host pumps.
//
// Whitened variables (v = R p, Sigma = L R, R = L'): a kick is v += e R grad logp, a drift x += e L v, the kinetic energy |v|^2 / 2, and the
// generalised U-turn criterion rho' Sigma p = (R rho) . (R p) is a plain dot product of whitened momenta: the tree logic needs no operator.
//
// The tree of transition t.  v0 = the normals of draw t, H0 = -lp + |v0|^2 / 2; the tree is the single leaf (x, v0) with log-weight 0.
// Doubling j = 0, 1, ... draws a direction and grows a SUB-TREE of 2^j leaves from the tree's end in that direction, one leaf per round:
//   leaf n (0-based):  v_leaf = v_half + dir (e/2) R g;  H = -lp~ + |v_leaf|^2 / 2;  log-weight lw = H0 - H;  rho_s += v_leaf
//     divergent (non-finite lp~, g~ or H, or H - H0 > 1000): the sub-tree is discarded, the transition ends
//     the leaf replaces the sub-tree's candidate iff u_leaf < exp(lw - logaddexp(logW_s, lw));  logW_s <- logaddexp(logW_s, lw)
//     checkpoints, imax = popcount(n >> 1):  even n stores (v_leaf, rho_s) at index imax;  odd n checks indices imax down to
//     imax - (trailing one-bits of n) + 1:  rho_sub = rho_s - rho_ck[i] + v_ck[i] against v_ck[i] and v_leaf -- a turn when either dot
//     product is <= 0: the sub-tree is discarded, the transition ends
//   after leaf 2^j - 1: the sub-tree's candidate replaces the tree's iff u_tree < exp(logW_s - logW) (biased progressive sampling);
//     logW <- logaddexp(logW, logW_s), rho += rho_s, the end in direction dir becomes the leaf; the transition ends when rho . v- <= 0 or
//     rho . v+ <= 0, or when j + 1 == max_depth.
// The tree's candidate becomes the chain's state and row t.  A chain that ends a transition opens the next one in the same launch; a chain
// that has made its transitions idles (its workgroup returns at once, its column of X stays its state).
//
// Random numbers of transition t under the chain's seed: the momentum is draw t of the normals; direction and tree uniform of doubling j use
// counter 16 t + j of their streams, the leaf uniform counter 1024 t + (leaves made before it in this transition): max_depth <= 10.
//
// Every control-flow scalar comes out of a fixed-order block reduction, so all threads of a chain take the same branch; the only atomics are
// the two progress counters.  A chain's output depends on nothing but its own inputs.
#include "pfmi_common.h"
#include "hmc_rows.h"
#include "hmc_target.h"
#include <float.h>
#include <type_traits>

#define NT_MAXD 10                     // deepest tree: 2^10 - 1 leaves per transition
#define NT_NDOT 24                     // |v|^2, two dot products per checkpoint, two of the full tree, padded to a multiple of 4

enum { NT_START = 0, NT_LEAF = 1, NT_IDLE = 2 };

struct NtChain {                       // per-chain scalar state (HBM); read by every thread, written back by thread 0
    double lp, H0;                     // the state's log density; the energy at the root of the transition's tree
    double lpc, Hc, lps, Hs;           // log density and energy of the tree's / the growing sub-tree's candidate
    double logW, logWs, sacc;          // log total weight of the tree / sub-tree; sum of the leaves' acceptance statistics
    int64_t t, fin_round;              // transitions made so far; the round in which the chain went idle
    int32_t phase, j, n, dir, nleaf, dead;
};

struct NtArgs {
    int d, K, max_depth, nslot, record, reopen;  // nslot: slots of a chain's block (NT_VECS + twice the depth the chains were made with)
    int64_t t0, t_end, T;              // this call records transitions t0 .. t_end - 1 as rows 0 .. T - 1
    int64_t round, prow;               // number of this launch (progress word); row of the recorded path
    const int32_t *pts;
    const uint64_t *seeds;
    double *eps;                       // [K]; a warm-up launch that ends a transition writes the chain's next step size
    const double *x0;
    double *X;                         // closure input: d x K column-major
    const double *out;                 // closure output: logp [K], then grad [K][d]
    double *blk;                       // [K][NT_VECS + 2 max_depth][d]: the chain's vectors (the slots below), then its checkpoints
    NtChain *st;
    PfAdapt *ad;                       // adaptive runs: [K] adaptation states, then the warm-up traces PfWarmRow [K][t0] (read by thread 0 only)
    double *draws, *rlp, *racc, *rde;  // records [K][T][d], [K][T] (shared with static HMC)
    int32_t *rdiv, *rdepth, *rnleap;   // [K][T]
    double *pX, *pout, *pv;            // PFMI_NUTS_RECORD_PATH
    pfmi_nuts_event *pev;              // [rounds][K]
    int32_t *ctr;                      // [2]: chains still running after this launch, tickets
    int64_t *h_status;                 // page-locked progress word
    const double *vh, *tmat, *vchol, *sqa;
};
// Slots of a chain's block: the state x and wg = R grad logp(x), wt = R grad at the trial point, the working momentum v; both ends of the
// trajectory (index 0: the backward end, 1: the forward end); the two candidates; the momentum sums; then max_depth checkpoints of v_leaf and
// max_depth of rho_s.  ONE base address per chain and slot offsets in the index: the scalar registers hold the factor's and the records'
// addresses, not sixteen more.
enum { NT_X = 0, NT_WG = 1, NT_WT = 2, NT_V = 3, NT_XE = 4, NT_VE = 6, NT_WE = 8, NT_XC = 10, NT_WC = 11, NT_XS = 12, NT_WS = 13, NT_RHO = 14,
       NT_RHOS = 15, NT_VECS = 16 };

__device__ __forceinline__ double nt_uniform(uint64_t seed, uint64_t ctr, uint32_t stream) {
    return (double)(pf_rand_u64(seed, ctr, stream) >> 11) * 0x1p-53;
}
__device__ __forceinline__ int nt_direction(uint64_t seed, int64_t t, int j) {
    return (pf_rand_u64(seed, (uint64_t)(16 * t + j), PF_RNG_STREAM_NUTS_DIR) >> 63) ? 1 : -1;
}
__device__ __forceinline__ double nt_logaddexp(double a, double b) {
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    return fmax(a, b) + log1p(exp(-fabs(a - b)));
}

#ifndef PF_CHAIN_METRIC_TU
__global__ __launch_bounds__(HM_NT) void pf_nuts_init_kernel(NtArgs A) {
    const int k = blockIdx.x, d = A.d;
    hm_copy_start(A.x0 + (size_t)k * d, A.X + (size_t)k * d, A.blk + (size_t)k * A.nslot * d + (size_t)NT_X * d, d);
    if (threadIdx.x == 0) {
        NtChain S = {};
        S.phase = NT_START;
        A.st[k] = S;
    }
}
#endif

// ADAPT (pf_nuts_warm_kernel): transitions t < t0 are the warm-up.  They write no row but a PfWarmRow, and thread 0 applies pf_adapt_update
// between recording transition t and opening transition t + 1, whose first half kick and drift already use the new step size.
//
// MODE NT_METRIC (pf_nuts_metric_kernel, nuts_metric_kernel.hip): the chain carries a per-coordinate scale c (HmMetric, hmc_rows.h): a kick is
// v += e c . (R g), a drift x += e L (c . v) -- every stored R g and v stays what it is without a scale -- and a warm-up transition inside a
// metric window ends with hm_metric_end.  Plain runs (which may record their path) and adaptive runs share it.
enum { NT_PLAIN = 0, NT_WARM = 1, NT_METRIC = 2 };

// progress of a launch, by thread 0 of every workgroup: the last one publishes (A.round << 32 | chains still running)
template <class Args>
__device__ __forceinline__ void nt_publish(const Args &A, bool running, int K) {
    if (threadIdx.x == 0) {
        if (running) __hip_atomic_fetch_add(A.ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const int ticket = __hip_atomic_fetch_add(A.ctr + 1, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == K - 1) {
            const int active = __hip_atomic_load(A.ctr, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            A.ctr[0] = 0; A.ctr[1] = 0;
            __hip_atomic_store(A.h_status, (int64_t)((A.round << 32) | (int64_t)active), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ONE ROUND (nt_round) is what a launch of the step kernels does.  TG == HM_TG_NONE (the step kernels): the round loads the chain's scalars,
// consumes the closure's output, stores the state and takes the launch's ticket.  TG a built-in target (pf_nuts_fused_kernel,
// nuts_fused_kernel.hip: MODE NT_WARM, which there may record its path): the kernel enters the round once per TRIP of its loop; the round
// evaluates the target itself where a step kernel reads the closure's output (hm_target_eval, hmc_target.h; the opening trip of a CONTINUE
// evaluates nothing), and the CALLER loads the scalars before the first trip, stores S after the last and takes the ticket.  What a trip
// carries to the next is NtCarry: S, the step size (a warm-up transition's end changes it), the seed and fit point, `trip` (evaluations the
// call has made: the row of the recorded path, and + 1 the round number of the closure route), the ping-pong side `flip` of the reduction
// buffers, `staged` (the factor rows are in LDS: staged ONCE per launch) and `reopen` (this trip is the opening one of a CONTINUE).
struct NtCarry { NtChain S; double eps; uint64_t seed; int64_t trip; int pt, flip; bool staged, reopen; };
template <int KPAD, bool RES, int MODE, int TG, class Args>
__device__ __forceinline__ void nt_round(const Args &A_, NtCarry &C) {
    constexpr bool ADAPT = MODE != NT_PLAIN, METRIC = MODE == NT_METRIC, FUSED = TG != HM_TG_NONE;
    // The arguments are read where they are used, through the kernel-argument segment itself (A_ is the kernel's first and only entry): as a
    // by-value parameter all 80 dwords are loaded on entry and stay in scalar registers until their one use.
#if defined(__HIP_DEVICE_COMPILE__)
    const Args &A = *(const Args *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    const Args &A = A_;
#endif
    // an adaptive run records no path (its flags are 0): the warm kernel carries none of that code and none of its addresses
    auto rec = [&]() -> int {
        if constexpr (MODE == NT_WARM && !FUSED) return 0;
        else return A.record;
    };
    constexpr int NVM = KPAD + 4;                        // KPAD sums + one rider (pf_block_sum_mv takes multiples of 4)
    constexpr int NOPS = NVM > NT_NDOT ? NVM : NT_NDOT;  // FUSED: or the evaluation's reduction, if that is wider
    constexpr int NRED = FUSED && HmTargetShape<TG>::NV > NOPS ? HmTargetShape<TG>::NV : NOPS;
    // (HmLds of hmc_rows.h with the vectors first: with the reduction buffers first pf_nuts_warm_kernel<12, true> moves a seventh scalar
    // register into a lane)
    struct NtLds {
        alignas(16) double sTv[KPAD], sZ[KPAD], sHead[KPAD];
        alignas(16) double red[2 * HM_NW * NRED];
    };
    struct NtTargetLds : NtLds {                         // FUSED: G's copy behind them (hm_target_stage)
        alignas(16) double sG[HmTargetShape<TG>::NG];
    };
    __shared__ std::conditional_t<FUSED, NtTargetLds, NtLds> L;
    const int k = blockIdx.x, tid = threadIdx.x, d = A.d, K = A.K;
    int flip = 0;
    // the chain's scalars, its step size, seed and fit point go through LDS: the values (and the factor's addresses, which depend on the
    // point) live in vector registers; the uniform addresses of the passes fill the scalar file
    __shared__ NtChain sS;
    __shared__ double sEps;
    __shared__ uint64_t sSeed;
    __shared__ int sPt;
    NtChain S;
    if constexpr (FUSED) { flip = C.flip; S = C.S; }
    else {
        if (tid == 0) { sS = A.st[k]; sEps = A.eps[k]; sSeed = A.seeds[k]; sPt = A.pts[k]; }
        __syncthreads();
        S = sS;
    }
    const bool idle_in = S.phase == NT_IDLE;
    // the opening launch (trip) of a CONTINUE; the row of the recorded path; the number of the round -- each read where it is used
    auto reopen = [&]() -> bool { if constexpr (FUSED) return C.reopen; else return A.reopen != 0; };
    auto prow = [&]() -> int64_t { if constexpr (FUSED) return C.trip; else return A.prow; };
    auto round = [&]() -> int64_t { if constexpr (FUSED) return C.trip + 1; else return A.round; };
    if (!(idle_in && !reopen())) {
        int p;
        if constexpr (FUSED) p = C.pt; else p = sPt;
        const size_t kd = (size_t)k * d;
        // The rule for the base addresses: in the warm kernel, and only there, the argument addresses that live through the whole launch pass
        // through an empty asm, which makes each an opaque value in scalar registers.  Left as the result of the merged eight-dword argument
        // load they are a tuple the register allocator splits around the update and REMATERIALISES, and the spill slot it leaves behind
        // (never read, never written) makes every wave reserve scratch; an opaque value is moved into a lane of a vector register instead.
        // The plain kernel keeps its loads as they are and has no such slot as long as the L pass below is written out: through
        // hm_apply_L no rule tried held both its registers and its time (profiles/chain_kernels.md).
        auto karg = [&](auto *const &f) {
            using P = std::remove_cv_t<std::remove_reference_t<decltype(f)>>;
            if constexpr (ADAPT) {
                uint64_t u = (uint64_t)f;
                asm volatile("" : "+s"(u));
                return (P)u;
            } else return f;
        };
        const double *gVh = karg(A.vh) + (size_t)p * d * KPAD, *T = karg(A.tmat) + (size_t)p * KPAD * KPAD, *Vc = karg(A.vchol) + (size_t)p * KPAD * KPAD;
        const double *sqa = karg(A.sqa) + (size_t)p * d;
        double *X = A.X + kd;
        double *B = A.blk + (size_t)k * A.nslot * d;
        const int ckv = NT_VECS, ckr = NT_VECS + (A.nslot - NT_VECS) / 2;        // first checkpoint slots
#define V_(slot, i) B[(size_t)(slot) * d + (i)]
        double eps;
        uint64_t seed;
        if constexpr (FUSED) { eps = C.eps; seed = C.seed; } else { eps = sEps; seed = sSeed; }
        const HmFactor F = {gVh, T, Vc, sqa};
        // METRIC: the chain's scale; c_i w of a kick and c_i v_i of a drift (row i is the calling thread's own; without METRIC the plain operand)
        // (macros on the constant METRIC and not hm_scaled of hmc_rows.h: through the function the step and warm kernels with staged rows
        // allocate their registers differently -- three step kernels then reserve scratch -- although it returns its operand)
        const double *sc = nullptr;
        if constexpr (METRIC) sc = A.M.scale + kd;
#define KSC_(i, w) (METRIC ? sc[i] * (w) : (w))
#define VSC_(i) (METRIC ? sc[i] * V_(NT_V, i) : V_(NT_V, i))
        HM_STAGED_ROWS;                                      // (the L pass below reads the rows the R pass staged)
        auto vrow = [&](int i) -> const double * {
            if constexpr (RES) return sVh + (size_t)i * KPAD;
            else return gVh + (size_t)i * KPAD;
        };
        bool staged = false;                                 // an R pass came before the L pass (hmc_rows.h)
        if constexpr (FUSED) staged = C.staged;
        if constexpr (TG > 0) if (!staged) hm_target_stage<TG>(A.tg, L);     // G, once per launch: the first trip's first barrier publishes it
        bool open = idle_in, drift = false;
        int wend = 0;                                        // ADAPT: this launch ended a warm-up transition (2: a divergent one)
        int bslot = -1;                                      // the drift's base: a slot, or (-1) the trial point itself
        int ndir = S.dir;                                    // direction of the leapfrog step this launch starts
        if (!idle_in) {
            double lpt;
            if constexpr (FUSED) lpt = hm_target_eval<TG, NRED>(A.tg, L, X, A.gout + K + kd, d, flip);
            else lpt = A.out[k];
            const double *g = A.out + K + kd;
            const size_t pr = ((size_t)prow() * K + k);
            if (rec()) {                                  // what the closure saw and what it answered, before X is rewritten
                double *pX = A.pX + pr * d, *pout = A.pout + (size_t)prow() * ((size_t)K * (d + 1));
                for (int i = tid; i < d; i += HM_NT) { pX[i] = X[i]; pout[K + kd + i] = g[i]; }
                if (tid == 0) pout[k] = lpt;
            }
            const double nbad = hm_apply_R<KPAD, RES, HM_NT, NRED>(F, L, g, d, flip, [&](int i) -> double & { return V_(NT_WT, i); },     // (reduction 1)
                                                                      FUSED && staged);
            staged = true;
            const bool badg = nbad > 0.0 || !isfinite(lpt);
            if (S.phase == NT_START) {
                for (int i = tid; i < d; i += HM_NT) V_(NT_WG, i) = badg ? 0.0 : V_(NT_WT, i);
                S.lp = badg ? -DBL_MAX : lpt;
                S.dead = badg ? 1 : 0;
                open = true;
                if (rec()) {
                    double *pv = A.pv + pr * d;
                    for (int i = tid; i < d; i += HM_NT) pv[i] = 0.0;
                    if (tid == 0) {
                        pfmi_nuts_event E = {};
                        E.t = -1; E.j = -1; E.n = -1; E.flags = badg ? PFMI_NUTS_EV_DIVERGENT : 0;
                        A.pev[pr] = E;
                    }
                }
            } else {
                // ---- the leaf: last half kick, rho_s, the checkpoints, every dot product of the decisions      (reduction 2)
                const int j = S.j, n = S.n, dir = S.dir;
                const int imax = __popc((unsigned)n >> 1), nchk = (n & 1) ? __ffs(~n) - 1 : 0;       // trailing one-bits of n
                const bool last = n == (1 << j) - 1, store = (n & 1) == 0;
                const double hk = (dir > 0 ? 0.5 : -0.5) * eps;
                const int vo = NT_VE + (dir > 0 ? 0 : 1);                 // the momentum at the tree's other end
                double *pv = rec() ? A.pv + pr * d : nullptr;
                double w[NT_NDOT];
#pragma unroll
                for (int q = 0; q < NT_NDOT; ++q) w[q] = 0.0;
                for (int i = tid; i < d; i += HM_NT) {
                    const double vl = fma(hk, KSC_(i, V_(NT_WT, i)), V_(NT_V, i)), rs = V_(NT_RHOS, i) + vl;
                    V_(NT_V, i) = vl; V_(NT_RHOS, i) = rs;
                    if (pv) pv[i] = vl;
                    w[0] = fma(vl, vl, w[0]);
                    if (last) {
                        const double rn = V_(NT_RHO, i) + rs;
                        w[21] = fma(rn, vl, w[21]);
                        w[22] = fma(rn, V_(vo, i), w[22]);
                    }
                    if (store) { V_(ckv + imax, i) = vl; V_(ckr + imax, i) = rs; }
                }
                // (one pass per checkpoint, over the rows the thread has just written: the accumulators keep static indices and only one
                // checkpoint's addresses are live at a time)
#pragma unroll
                for (int c = 0; c < NT_MAXD; ++c)
                    if (c < nchk) {
                        const int sv = ckv + imax - c, sr = ckr + imax - c;
                        double a0 = 0.0, a1 = 0.0;
                        for (int i = tid; i < d; i += HM_NT) {
                            const double vc = V_(sv, i), rsub = (V_(NT_RHOS, i) - V_(sr, i)) + vc;
                            a0 = fma(rsub, vc, a0);
                            a1 = fma(rsub, V_(NT_V, i), a1);
                        }
                        w[1 + 2 * c] = a0; w[2 + 2 * c] = a1;
                    }
                pf_block_sum_mv<NT_NDOT, NRED>(w, L.red, flip);
                // ---- decide (every thread, on the same values)
                const double Hl = -lpt + 0.5 * w[0], dH = Hl - S.H0, lw = -dH;
                const bool div = badg || !isfinite(Hl) || dH > 1000.0;
                bool turn = false, sel = false, complete = false, tsel = false, fturn = false, mstop = false;
                S.sacc += div ? 0.0 : fmin(1.0, exp(lw));
                const int leaf = S.nleaf++;
                if (!div) {
                    const double lws = nt_logaddexp(S.logWs, lw);
                    sel = nt_uniform(seed, (uint64_t)(1024 * S.t + leaf), PF_RNG_STREAM_NUTS_LEAF) < exp(lw - lws);
                    S.logWs = lws;
                    if (sel) { S.lps = lpt; S.Hs = Hl; }
#pragma unroll
                    for (int c = 0; c < NT_MAXD; ++c)
                        if (c < nchk) turn = turn || !(w[1 + 2 * c] > 0.0) || !(w[2 + 2 * c] > 0.0);
                    if (!turn && last) {
                        complete = true;
                        tsel = nt_uniform(seed, (uint64_t)(16 * S.t + j), PF_RNG_STREAM_NUTS_TREE) < exp(S.logWs - S.logW);
                        S.logW = nt_logaddexp(S.logW, S.logWs);
                        if (tsel) { S.lpc = S.lps; S.Hc = S.Hs; }
                        fturn = !(w[21] > 0.0) || !(w[22] > 0.0);
                        mstop = j + 1 >= A.max_depth;
                    }
                }
                const bool end = div || turn || (complete && (fturn || mstop));
                if (rec() && tid == 0) {
                    pfmi_nuts_event E;
                    E.t = (int32_t)S.t; E.j = j; E.n = n; E.dir = dir; E.leaf = leaf;
                    E.flags = (div ? PFMI_NUTS_EV_DIVERGENT : 0) | (turn ? PFMI_NUTS_EV_SUBTREE_TURN : 0) | (sel ? PFMI_NUTS_EV_LEAF_TAKEN : 0) |
                              (complete ? PFMI_NUTS_EV_SUBTREE_DONE : 0) | (tsel ? PFMI_NUTS_EV_TREE_TAKEN : 0) | (fturn ? PFMI_NUTS_EV_TREE_TURN : 0) |
                              (mstop ? PFMI_NUTS_EV_MAX_DEPTH : 0) | (end ? PFMI_NUTS_EV_END : 0);
                    E.H_leaf = Hl; E.logW_s = S.logWs; E.logW = S.logW; E.H0 = S.H0;
                    A.pev[pr] = E;
                }
                // ---- update the states
                const int64_t row = S.t - A.t0;
                bool warm = false;                               // (a scalar: S comes through LDS, so row < 0 alone is a lane mask)
                if constexpr (ADAPT) warm = __builtin_amdgcn_readfirstlane(row < 0 ? 1 : 0) != 0;
                double *dr = karg(A.draws) + ((size_t)k * A.T + (warm ? 0 : row)) * d;
                const int en = dir > 0 ? 1 : 0;
                for (int i = tid; i < d; i += HM_NT) {
                    double xsi = V_(NT_XS, i), wsi = V_(NT_WS, i);
                    if (sel) { xsi = X[i]; wsi = V_(NT_WT, i); V_(NT_XS, i) = xsi; V_(NT_WS, i) = wsi; }
                    double xci = V_(NT_XC, i), wci = V_(NT_WC, i);
                    if (complete) {
                        V_(NT_RHO, i) = V_(NT_RHO, i) + V_(NT_RHOS, i);
                        V_(NT_XE + en, i) = X[i]; V_(NT_VE + en, i) = V_(NT_V, i); V_(NT_WE + en, i) = V_(NT_WT, i);
                        if (tsel) { xci = xsi; wci = wsi; V_(NT_XC, i) = xci; V_(NT_WC, i) = wci; }
                    }
                    if (end) { V_(NT_X, i) = xci; V_(NT_WG, i) = wci; if (!warm) dr[i] = xci; }
                }
                if (end) {
                    S.lp = S.lpc;
                    if (warm) wend = div ? 2 : 1;
                    if (tid == 0 && !warm) {
                        const size_t r = (size_t)k * A.T + row;
                        const double de = S.Hc - S.H0;
                        A.rlp[r] = S.lp; A.racc[r] = S.sacc / (double)S.nleaf; A.rde[r] = isfinite(de) ? de : DBL_MAX; A.rdiv[r] = div ? 1 : 0;
                        A.rdepth[r] = j + 1; A.rnleap[r] = S.nleaf;
                    }
                    ++S.t;
                    if (S.t < A.t_end) open = true;
                    else {
                        for (int i = tid; i < d; i += HM_NT) X[i] = V_(NT_X, i);      // an idle chain's column stays a valid point
                        S.phase = NT_IDLE; S.fin_round = round();
                    }
                } else if (complete) {
                    // ---- the next doubling: from the tree's end in the new direction
                    S.j = j + 1; S.n = 0; S.logWs = -INFINITY;
                    ndir = nt_direction(seed, S.t, S.j);
                    S.dir = ndir;
                    const int e = ndir > 0 ? 1 : 0;
                    const double hk2 = (ndir > 0 ? 0.5 : -0.5) * eps;
                    for (int i = tid; i < d; i += HM_NT) { V_(NT_RHOS, i) = 0.0; V_(NT_V, i) = fma(hk2, KSC_(i, V_(NT_WE + e, i)), V_(NT_VE + e, i)); }
                    bslot = NT_XE + e;
                    drift = true;
                } else {
                    // ---- the next leaf of the sub-tree
                    S.n = n + 1;
                    for (int i = tid; i < d; i += HM_NT) V_(NT_V, i) = fma(hk, KSC_(i, V_(NT_WT, i)), V_(NT_V, i));
                    drift = true;
                }
            }
        }
        if constexpr (ADAPT) {
            // ---- the warm-up transition S.t - 1 has ended: its trace, the update, the step size of the transition that opens below
            // (here and not in the branch above: fewer uniform values are live beside the constants of sqrt and exp)
            if (wend) {
                bool wnd = false;                        // METRIC: the transition ended a metric window
                if constexpr (METRIC)
                    wnd = hm_metric_end<KPAD, RES, NRED>(F, L, A.M, A.ad, k, d, S.t - 1, A.x0 + kd, flip, [&](int i) { return V_(NT_X, i); });
                if (tid == 0) {
                    sEps = hm_warm_end(A.ad, A.eps, K, k, S.t, A.t0, eps, S.sacc / (double)S.nleaf, wend - 1, S.nleaf);
                    if constexpr (METRIC) if (wnd) pf_adapt_restart(A.ad[k], sEps);
                }
                __syncthreads();
                eps = sEps;
            }
        }
        double vv0 = 0.0;
        if (open) {
            // ---- the next transition: fresh momentum (draw t of the chain's seed), the one-leaf tree, the first direction and half kick
            const uint32_t nd = (uint32_t)S.t;
            ndir = nt_direction(seed, S.t, 0);
            const double hk = (ndir > 0 ? 0.5 : -0.5) * eps;
            for (int i = tid; i < d; i += HM_NT) {
                const double z = hm_normal(seed, nd, i), xi = V_(NT_X, i), wi = V_(NT_WG, i);
                vv0 = fma(z, z, vv0);
                V_(NT_XE, i) = xi; V_(NT_XE + 1, i) = xi; V_(NT_VE, i) = z; V_(NT_VE + 1, i) = z; V_(NT_WE, i) = wi; V_(NT_WE + 1, i) = wi;
                V_(NT_XC, i) = xi; V_(NT_WC, i) = wi; V_(NT_RHO, i) = z; V_(NT_RHOS, i) = 0.0;
                V_(NT_V, i) = fma(hk, KSC_(i, wi), z);
            }
            S.phase = NT_LEAF; S.j = 0; S.n = 0; S.dir = ndir; S.nleaf = 0; S.sacc = 0.0;
            S.logW = 0.0; S.logWs = -INFINITY; S.lpc = S.lp;
            bslot = NT_X;
            drift = true;
        }
        if (drift) {
            // ---- X <- base + dir e L v: z = [V'v_head; v_tail], w = Vh'z, tv = T w, y = s . (z - Vh tv)          (reduction 3)
            // (hm_apply_L of hmc_rows.h, written out: see the rule for the base addresses above)
            const double se = ndir > 0 ? eps : -eps;
            __syncthreads();                                 // the head product above has read sHead
            if (tid < KPAD) L.sHead[tid] = tid < d ? VSC_(tid) : 0.0;
            __syncthreads();
            if (tid < KPAD) {
                double s = 0.0;
#pragma unroll
                for (int b = 0; b < KPAD; ++b) if (b <= tid) s = fma(Vc[b * KPAD + tid], L.sHead[b], s);
                L.sZ[tid] = s;
            }
            __syncthreads();
            double w[NVM];
#pragma unroll
            for (int q = 0; q < NVM; ++q) w[q] = 0.0;
            if (RES && !staged) {                            // (the opening launch of PFMI_NUTS_CONTINUE: no R-apply came before)
                for (int i = tid; i < d; i += HM_NT)
                    hm_row_axpy<KPAD, NVM, true>(gVh + (size_t)i * KPAD, sVh + (size_t)i * KPAD, i < KPAD ? L.sZ[i] : VSC_(i), w);
            } else {
                for (int i = tid; i < d; i += HM_NT) hm_row_axpy<KPAD, NVM, false>(vrow(i), nullptr, i < KPAD ? L.sZ[i] : VSC_(i), w);
            }
            w[KPAD] = vv0;
            pf_block_sum_mv<NVM, NRED>(w, L.red, flip);
            if (open) { S.H0 = -S.lp + 0.5 * w[KPAD]; S.Hc = S.H0; }
            if (tid < KPAD) {
                double s = 0.0;
#pragma unroll
                for (int b = 0; b < KPAD; ++b) if (b >= tid) s = fma(T[tid * KPAD + b], w[b], s);
                L.sTv[tid] = s;
            }
            __syncthreads();
            for (int i = tid; i < d; i += HM_NT) {
                const double y = hm_row_sub<KPAD>(vrow(i), L.sTv, i < KPAD ? L.sZ[i] : VSC_(i));
                X[i] = fma(se, sqa[i] * y, bslot < 0 ? X[i] : V_(bslot, i));
            }
            if constexpr (FUSED) staged = true;
        }
        if constexpr (FUSED) { C = {S, eps, seed, idle_in ? prow() : round(), p, flip, staged, false}; return; }
        __syncthreads();                                     // every thread has read S before thread 0 writes
        if (tid == 0) A.st[k] = S;
#undef V_
#undef KSC_
#undef VSC_
    }
    // ---- progress of the round: the last workgroup publishes the number of chains still running
    if constexpr (!FUSED) nt_publish(A, S.phase != NT_IDLE, K);
}

// one launch of the step kernels: one round on the chain's state in HBM
template <int KPAD, bool RES, int MODE, class Args>
__device__ __forceinline__ void nt_step_body(const Args &A_) {
    NtCarry none;                                        // (not read, not written)
    nt_round<KPAD, RES, MODE, HM_TG_NONE>(A_, none);
}

#ifndef PF_CHAIN_METRIC_TU             // (nuts_metric_kernel.hip takes the body and nt_args from this file and defines its own kernels)
template <int KPAD, bool RES>
__global__ __launch_bounds__(HM_NT) void pf_nuts_step_kernel(NtArgs A_) { nt_step_body<KPAD, RES, NT_PLAIN>(A_); }

template <int KPAD, bool RES>
__global__ __launch_bounds__(HM_NT) void pf_nuts_warm_kernel(NtArgs A_) { nt_step_body<KPAD, RES, NT_WARM>(A_); }
#endif

// ---------------------------------------------------------------------------------------------------
static NtArgs nt_args(pfmi_ctx *c, int64_t round, int64_t prow, bool reopen) {
    const HmcState &H = c->hmc;
    NtArgs A;
    A.d = c->d; A.K = H.K; A.max_depth = H.max_depth; A.nslot = pf_nuts_vec_slots(H.md_alloc); A.record = H.record ? 1 : 0; A.reopen = reopen ? 1 : 0;
    A.t0 = H.t0; A.t_end = H.t0 + H.T; A.T = H.T; A.round = round; A.prow = prow;
    A.pts = c->hm_pts.as<int32_t>(); A.seeds = c->hm_seeds.as<uint64_t>(); A.eps = c->hm_eps.as<double>(); A.x0 = c->hm_x0.as<double>();
    A.X = c->hm_X.as<double>(); A.out = c->hm_out.as<double>();
    A.blk = c->nt_vec.as<double>();
    A.st = c->nt_st.as<NtChain>();
    A.draws = c->hm_draws.as<double>(); A.rlp = c->hm_lp.as<double>(); A.racc = c->hm_acc.as<double>(); A.rde = c->hm_de.as<double>();
    A.rdiv = c->hm_div.as<int32_t>(); A.rdepth = c->nt_depth.as<int32_t>(); A.rnleap = c->nt_nleap.as<int32_t>();
    A.pX = c->hm_pX.as<double>(); A.pout = c->hm_pout.as<double>(); A.pv = c->hm_pv.as<double>(); A.pev = c->nt_pev.as<pfmi_nuts_event>();
    A.ctr = c->nt_ctr.as<int32_t>(); A.h_status = c->nt_status;
    A.vh = c->vh.as<double>(); A.tmat = c->tmat.as<double>(); A.vchol = c->vchol.as<double>(); A.sqa = c->sqrt_alpha.as<double>();
    A.ad = c->hm_adapt.as<PfAdapt>();
    return A;
}

#ifndef PF_CHAIN_METRIC_TU
size_t pf_nuts_chain_bytes() { return sizeof(NtChain); }
int pf_nuts_vec_slots(int max_depth) { return NT_VECS + 2 * max_depth; }

int32_t pf_launch_nuts_init(pfmi_ctx *c, hipStream_t s) {
    hipLaunchKernelGGL(pf_nuts_init_kernel, dim3(c->hmc.K), dim3(HM_NT), 0, s, nt_args(c, 0, 0, false));
    PF_HIP(hipGetLastError());
    return PFMI_OK;
}

struct NtFamily {
    static constexpr bool has_warm = true;
    template <int KPAD, bool RES, bool ADAPT>
    static auto kernel() { return ADAPT ? &pf_nuts_warm_kernel<KPAD, RES> : &pf_nuts_step_kernel<KPAD, RES>; }
};

// the chains' start flags and the last round in which a chain was still running
int32_t pf_nuts_chain_flags(pfmi_ctx *c, std::vector<int32_t> &dead, int64_t *last_round) {
    const int K = c->hmc.K;
    std::vector<NtChain> st((size_t)K);
    PF_HIP(hipMemcpyAsync(st.data(), c->nt_st.p, sizeof(NtChain) * K, hipMemcpyDeviceToHost, c->stream));
    PF_HIP(hipStreamSynchronize(c->stream));
    dead.resize((size_t)K);
    int64_t lr = 0;
    for (int k = 0; k < K; ++k) {
        dead[(size_t)k] = st[(size_t)k].dead;
        if (st[(size_t)k].fin_round > lr) lr = st[(size_t)k].fin_round;
    }
    *last_round = lr;
    return PFMI_OK;
}

// round: the number the launch publishes with its progress word; prow: its row of the recorded path; reopen: the opening launch of
// PFMI_NUTS_CONTINUE (no closure output is read, every idle chain opens its next transition)
int32_t pf_launch_nuts_step(pfmi_ctx *c, int64_t round, int64_t prow, bool reopen, hipStream_t s) {
    return hm_launch_step<NtFamily>(c, "nuts", nt_args(c, round, prow, reopen), s);
}
#endif
