// nuts_fused_kernel.hip -- NUTS on the BUILT-IN targets (Gaussian family, funnel): whole runs of a chain in one launch.
//
// nuts_kernel.hip cuts a run into rounds because the log density is the user's closure, which no kernel can call: every leapfrog step of
// every chain is two launches, each launch stages the factor rows again, and every chain's workgroup is launched until the slowest chain
// is done.  A built-in target's value and gradient are one block reduction plus row-local work (hm_target_eval, hmc_target.h) and the tree
// logic needs no other chain: so one workgroup of HM_NT threads per chain LOOPS over the trips of its launch --
//     trip:  evaluate the target at the trial point X (unless the trip only opens a transition: the first one of a CONTINUE),
//            then one round of the step (nt_round with a target, nuts_kernel.hip: the round of pf_nuts_warm_kernel, entered once per trip)
// -- with the chain's factor rows staged in LDS ONCE per launch (RES), G of a low-rank Gaussian in LDS beside them, and the scalar state
// (NtChain, the step size, the seed) in registers between the trips.  The chain's vectors stay in its block of nt_vec, X and the
// evaluation's output in the arrays the step kernels use: every thread reads back only rows it wrote, they are L2-resident, and a launch
// can so re-enter from what the launch before left -- in mid-tree too.  That is how a call is cut: no launch makes more than
// HM_FUSED_ROUNDS trips (hmc_rows.h; test hook PFMI_NUTS_FUSED_ROUNDS), and with a cap of 1 the launches are the rounds schedule of
// nuts_kernel.hip, bit for bit the same chain.
//
// A workgroup ends its launch after `cap` trips or as soon as its chain has made its transitions: a chain builds its trees at its own
// pace.  It then stores NtChain (fin_round: the trips the chain has made in this call, final once it is idle), and takes the launch's
// ticket; the last workgroup publishes (launch << 32 | chains still running) to the page-locked progress word (nt_publish).  There is no
// grid-wide barrier, no spin and no hand-over between workgroups: a chain's output depends on its own inputs alone.
//
// Warm-up (pfmi_nuts_fused_enqueue with nwarmup >= 1) is the NT_WARM mode at run time: a transition below t0 ends with hm_warm_end by
// thread 0; a plain run has none.  Random numbers: those of pfmi_nuts_enqueue, stream for stream and counter for counter.
// Instantiations: 7 column paddings x {res, stream} x {funnel, Gaussian rank padding 0, 8, 16} = 56.
#define PF_CHAIN_METRIC_TU             // (the round and nt_args of nuts_kernel.hip, not its kernels)
#include "nuts_kernel.hip"

struct NtFusedArgs : NtArgs {
    HmTarget tg;
    double *gout;                      // == out: the evaluation writes what the round reads
    int cap;                           // most evaluations of this launch; `round` is the launch's number, `reopen` its first trip's
};

// The loop of a launch, its carry, ticket and nt_publish: the body of a kernel <KPAD, RES, TG> whose first and only parameter is ARGS A_.
// MODE is NT_WARM here and NT_METRIC in nuts_fused_metric_kernel.hip (ARGS: NtFusedArgs, there with HmMetric M behind it).  A macro and
// not a function: the fused kernel is then the code it has always been (nuts_kernel.hip is sensitive to how its callers are written).
#if defined(__HIP_DEVICE_COMPILE__)
#define NT_FUSED_ARGS(ARGS) const ARGS &A = *(const ARGS *)__builtin_amdgcn_kernarg_segment_ptr();     /* (nt_round says why) */
#else
#define NT_FUSED_ARGS(ARGS) const ARGS &A = A_;
#endif
#define NT_FUSED_LOOP(ARGS, MODE)                                                                                         \
    NT_FUSED_ARGS(ARGS)                                                                                                   \
    const int k = blockIdx.x, tid = threadIdx.x;                                                                          \
    /* the chain's scalars go through LDS, as in the step kernels: the values live in vector registers */                 \
    __shared__ NtChain sS0;                                                                                               \
    __shared__ double sEps0;                                                                                              \
    __shared__ uint64_t sSeed0;                                                                                           \
    __shared__ int sPt0;                                                                                                  \
    if (tid == 0) { sS0 = A.st[k]; sEps0 = A.eps[k]; sSeed0 = A.seeds[k]; sPt0 = A.pts[k]; }                              \
    __syncthreads();                                                                                                      \
    NtCarry C;                                                                                                            \
    C.S = sS0; C.eps = sEps0; C.seed = sSeed0; C.pt = sPt0;                                                               \
    C.flip = 0; C.staged = false;                                                                                         \
    C.reopen = A.reopen != 0;                                                                                             \
    C.trip = C.reopen ? 0 : C.S.fin_round;               /* a CONTINUE counts its own evaluations */                      \
    const int64_t trip_end = C.trip + A.cap;                                                                              \
    const bool entered = C.reopen || C.S.phase != NT_IDLE;                                                                \
    _Pragma("unroll 1")                                                                                                   \
    while (C.reopen || (C.S.phase != NT_IDLE && C.trip < trip_end)) nt_round<KPAD, RES, MODE, TG>(A_, C);                 \
    if (entered) {                                                                                                        \
        __syncthreads();                                 /* every thread has read sS0 before thread 0 writes */           \
        if (tid == 0) { C.S.fin_round = C.trip; A.st[k] = C.S; }                                                          \
    }                                                                                                                     \
    nt_publish(A, C.S.phase != NT_IDLE, A.K);

// One launch of a fused family (Family::kernel<KPAD, RES, TG>() is its kernel, Family::plan its plan name; Args: NtFusedArgs or a struct
// that extends it): up to `cap` evaluations per chain, counted under "<plan>:<KPAD>:<res|stream>:<f|g0|g8|g16>"
template <class Family, class Args>
static int32_t nt_launch_fused(pfmi_ctx *c, Args &A, int64_t launch, int cap, bool reopen, hipStream_t s) {
    const TargetDev &T = c->target;
    static_cast<NtArgs &>(A) = nt_args(c, launch, 0, reopen);
    A.tg = {T.mean.as<double>(), T.a.as<double>(), T.wd.as<double>(), T.g.as<double>(), T.offset};
    A.gout = c->hm_out.as<double>();
    A.cap = cap;
    const int tgs = T.kind == PFMI_TARGET_FUNNEL ? HM_TG_FUNNEL : T.rpad;
    PF_CHECK((T.kind == PFMI_TARGET_FUNNEL || T.kind == PFMI_TARGET_GAUSS) && (tgs == HM_TG_FUNNEL || tgs == 0 || tgs == 8 || tgs == 16), PFMI_ERR_UNSUPPORTED,
             "%s: target kind %d with rank padding %d has no fused kernel", Family::plan, T.kind, T.rpad);
    const bool res = pf_hmc_resident(A.d, c->kpad);
    auto go = [&](auto KP, auto RES, auto TG) -> int32_t {
        auto *kern = Family::template kernel<KP(), RES(), TG()>();
        if (RES()) PF_TRY(pf_raise_lds_limit(c, reinterpret_cast<const void *>(kern), HM_LDS_RES));
        char name[48], tn[8];
        if (TG() == HM_TG_FUNNEL) snprintf(tn, sizeof tn, "f"); else snprintf(tn, sizeof tn, "g%d", (int)TG());
        snprintf(name, sizeof name, "%s:%d:%s:%s", Family::plan, (int)KP(), RES() ? "res" : "stream", tn);
        ++c->hmc_plans[name];
        hipLaunchKernelGGL(kern, dim3(A.K), dim3(HM_NT), RES() ? (size_t)A.d * KP() * sizeof(double) : 0, s, A);
        return PFMI_OK;
    };
    int32_t rc = PFMI_OK;
    const bool ok = pf_dispatch_kpad<4, 8, 12, 16, 20, 32, 64>(c->kpad, [&](auto KP) {
        auto tgt = [&](auto RES) -> int32_t {
            switch (tgs) {
                case HM_TG_FUNNEL: return go(KP, RES, std::integral_constant<int, HM_TG_FUNNEL>{});
                case 0: return go(KP, RES, std::integral_constant<int, 0>{});
                case 8: return go(KP, RES, std::integral_constant<int, 8>{});
                default: return go(KP, RES, std::integral_constant<int, 16>{});
            }
        };
        rc = res ? tgt(std::true_type{}) : tgt(std::false_type{});
    });
    PF_CHECK(ok, PFMI_ERR_UNSUPPORTED, "unsupported kpad %d", c->kpad);
    PF_TRY(rc);
    PF_HIP(hipGetLastError());
    return PFMI_OK;
}

#ifndef PF_FUSED_METRIC_TU             // (nuts_fused_metric_kernel.hip takes the loop, NtFusedArgs and the launch from this file and defines its own kernel)
template <int KPAD, bool RES, int TG>
__global__ __launch_bounds__(HM_NT) void pf_nuts_fused_kernel(NtFusedArgs A_) {
    NT_FUSED_LOOP(NtFusedArgs, NT_WARM)
}

struct NtFusedFamily {
    static constexpr const char *plan = "nuts_fused";
    template <int KPAD, bool RES, int TG>
    static auto kernel() { return &pf_nuts_fused_kernel<KPAD, RES, TG>; }
};

int32_t pf_launch_nuts_fused(pfmi_ctx *c, int64_t launch, int cap, bool reopen, hipStream_t s) {
    NtFusedArgs A;
    return nt_launch_fused<NtFusedFamily>(c, A, launch, cap, reopen, s);
}
#endif
