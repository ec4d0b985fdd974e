// hmc_fused_metric_kernel.hip -- static HMC on the BUILT-IN targets with a per-chain, per-coordinate scale on the fit's factor (adapt.h: the
// metric windows; include/pfmi.h: pfmi_chain_scale_set, pfmi_hmc_fused_metric_enqueue): pf_hmc_fused_metric_kernel is the loop of
// hmc_fused_kernel.hip (HM_FUSED_LOOP) around the round of hmc_kernel.hip in its HM_METRIC mode, in a translation unit of its own so that
// its 56 instantiations compile beside the fused kernels, not after them.  One kernel serves a plain run of chains that carry a scale and
// an adaptive run with metric windows.
//
// SCALE WRITTEN AND READ IN ONE LAUNCH.  In the step kernels a launch boundary lies between the end of a window, which writes M.scale
// (hm_metric_end, hmc_rows.h), and the next kick, which reads it.  Here both happen inside one launch, with no barrier or fence between
// them that is there for their sake.  That is safe ONLY because row i of the scale, of the Welford state (mean, M2), of the traces and of
// every chain vector is read and written by thread i % HM_NT alone (head row i of a Woodbury pass: by thread i), in program order: a
// thread always sees its own earlier stores.  So the scale pointer carries no __restrict__, no non-temporal and no read-only qualifier --
// any of them would let the compiler hoist the load of c_i over the window's store -- and no pass may ever read a row of the scale that
// another thread owns.  (tests/test_gpu_fused_metric.py runs an adaptive run at a launch cap of 1, where every boundary is back, against
// the default cap: the bits must not differ.)
//
// Nothing new between workgroups: no grid barrier, no spin, no hand-over; the launch cap HM_FUSED_ROUNDS and its test hook apply as they are.
#define PF_FUSED_METRIC_TU             // (the loop, HmFusedArgs and the launch of hmc_fused_kernel.hip, not its kernel)
#include "hmc_fused_kernel.hip"

struct HmFusedMetricArgs : HmFusedArgs {
    HmMetric M;
};

template <int KPAD, bool RES, int TG>
__global__ __launch_bounds__(HM_NT) void pf_hmc_fused_metric_kernel(HmFusedMetricArgs A) {
    HM_FUSED_LOOP(HM_METRIC)
}

struct HmFusedMetricFamily {
    static constexpr const char *plan = "hmc_fused_metric";
    template <int KPAD, bool RES, int TG>
    static auto kernel() { return &pf_hmc_fused_metric_kernel<KPAD, RES, TG>; }
};

int32_t pf_launch_hmc_fused_metric(pfmi_ctx *c, int64_t round, int ntrips, hipStream_t s) {
    HmFusedMetricArgs A;
    A.M = pf_chain_metric_args(c);
    return hm_launch_fused<HmFusedMetricFamily>(c, A, round, ntrips, s);
}
