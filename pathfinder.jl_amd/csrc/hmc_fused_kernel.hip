// hmc_fused_kernel.hip -- static HMC on the BUILT-IN targets (Gaussian family, funnel): whole runs of a chain in one launch.
//
// hmc_kernel.hip cuts a run into rounds because the log density is the user's closure, which no kernel can call.  A built-in target's value
// and gradient are one block reduction plus row-local work (hm_target_eval, hmc_target.h), and the chains never talk to each other: so one
// workgroup of HM_NT threads per chain LOOPS over the rounds of its launch --
//     trip:  evaluate the target at the trial point X (unless the trip only opens a trajectory: the first one of a CONTINUE),
//            then one round of the step (hm_round with a target, hmc_kernel.hip: the round of pf_hmc_warm_kernel, entered once per trip)
// -- with the chain's factor rows staged in LDS ONCE per launch (RES), G of a low-rank Gaussian in LDS beside them, and the scalar state
// (HmChain, the step size) in registers between the trips.  The chain's vectors stay in the HBM arrays the step kernels use (x, wg, wt, v,
// X and the evaluation's output): every thread reads back only rows it wrote, they are L2-resident, and a launch can so re-enter from what
// the launch before left -- in mid-trajectory too.  That is how a call is cut: no launch makes more than HM_FUSED_ROUNDS trips (hmc_rows.h;
// test hook PFMI_HMC_FUSED_ROUNDS), and with a cap of 1 the launches are the rounds schedule of hmc_kernel.hip, bit for bit the same chain.
// There is no grid-wide barrier, no spin and no hand-over between workgroups: a chain's output depends on its own inputs alone.
//
// Warm-up (pfmi_hmc_fused_enqueue with nwarmup >= 1) is the HM_WARM mode at run time: a transition below t0 ends with hm_warm_end by thread
// 0; a plain run has none.  Instantiations: 7 column paddings x {res, stream} x {funnel, Gaussian rank padding 0, 8, 16} = 56.
#define PF_CHAIN_METRIC_TU             // (the step body and hm_args of hmc_kernel.hip, not its kernels)
#include "hmc_kernel.hip"

struct HmFusedArgs : HmArgs {
    HmTarget tg;
    double *gout;                      // == out: the evaluation writes what the round reads
    int ntrips;                        // trips of this launch; `round` is the first one's (-1: the opening trip of a CONTINUE)
};

// The loop of a launch, the body of a kernel <KPAD, RES, TG> whose parameter is A: MODE is HM_WARM here and HM_METRIC in
// hmc_fused_metric_kernel.hip (A: HmFusedArgs, there with HmMetric M behind it).  A macro and not a function: the fused kernel is then the
// code it has always been -- through a forceinline function every instantiation of it moved about 20 more scalar registers into lanes.
#define HM_FUSED_LOOP(MODE)                                                                                               \
    const int k = blockIdx.x;                                                                                             \
    HmCarry C = {A.st[k], A.eps[k], A.round, 0, false};                                                                   \
    _Pragma("unroll 1")                                                                                                   \
    for (int trip = 0; trip < A.ntrips; ++trip) hm_round<KPAD, RES, MODE, TG>(A, C);                                      \
    __syncthreads();                                     /* every thread has read S before thread 0 writes */             \
    if (threadIdx.x == 0) A.st[k] = C.S;

// One launch of a fused family (Family::kernel<KPAD, RES, TG>() is its kernel, Family::plan its plan name; Args: HmFusedArgs or a struct
// that extends it): trips [round, round + ntrips) of the call, counted under "<plan>:<KPAD>:<res|stream>:<f|g0|g8|g16>"
template <class Family, class Args>
static int32_t hm_launch_fused(pfmi_ctx *c, Args &A, int64_t round, int ntrips, hipStream_t s) {
    const TargetDev &T = c->target;
    static_cast<HmArgs &>(A) = hm_args(c, round);
    A.tg = {T.mean.as<double>(), T.a.as<double>(), T.wd.as<double>(), T.g.as<double>(), T.offset};
    A.gout = c->hm_out.as<double>();
    A.ntrips = ntrips;
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

#ifndef PF_FUSED_METRIC_TU             // (hmc_fused_metric_kernel.hip takes the loop, HmFusedArgs and the launch from this file and defines its own kernel)
template <int KPAD, bool RES, int TG>
__global__ __launch_bounds__(HM_NT) void pf_hmc_fused_kernel(HmFusedArgs A) {
    HM_FUSED_LOOP(HM_WARM)
}

struct HmFusedFamily {
    static constexpr const char *plan = "hmc_fused";
    template <int KPAD, bool RES, int TG>
    static auto kernel() { return &pf_hmc_fused_kernel<KPAD, RES, TG>; }
};

int32_t pf_launch_hmc_fused(pfmi_ctx *c, int64_t round, int ntrips, hipStream_t s) {
    HmFusedArgs A;
    return hm_launch_fused<HmFusedFamily>(c, A, round, ntrips, s);
}
#endif
