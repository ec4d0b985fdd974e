// hmc_metric_kernel.hip -- static HMC on the fitted Woodbury factor with a per-chain, per-coordinate scale (adapt.h: the metric windows;
// include/pfmi.h: pfmi_chain_scale_set, pfmi_hmc_adapt_metric_enqueue): pf_hmc_metric_kernel is the step body of hmc_kernel.hip in its third
// mode, in a translation unit of its own so that its 14 instantiations compile beside the step and warm kernels, not after them.  One
// kernel serves a plain run of chains that carry a scale and an adaptive run with metric windows.
#define PF_CHAIN_METRIC_TU
#include "hmc_kernel.hip"

struct HmMetricArgs : HmArgs {
    HmMetric M;
};

template <int KPAD, bool RES>
__global__ __launch_bounds__(HM_NT) void pf_hmc_metric_kernel(HmMetricArgs A) { hm_step_body<KPAD, RES, HM_METRIC>(A); }

struct HmMetricFamily {
    static constexpr bool has_warm = false;
    template <int KPAD, bool RES, bool ADAPT>
    static auto kernel() { return &pf_hmc_metric_kernel<KPAD, RES>; }
};

int32_t pf_launch_hmc_metric_step(pfmi_ctx *c, int64_t round, hipStream_t s) {
    HmMetricArgs A;
    static_cast<HmArgs &>(A) = hm_args(c, round);
    A.M = pf_chain_metric_args(c);
    return hm_launch_step<HmMetricFamily>(c, "hmc_metric", A, s);
}
