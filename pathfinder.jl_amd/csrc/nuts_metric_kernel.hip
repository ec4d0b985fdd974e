// nuts_metric_kernel.hip -- NUTS on the fitted Woodbury factor with a per-chain, per-coordinate scale (adapt.h: the metric windows;
// include/pfmi.h: pfmi_chain_scale_set, pfmi_nuts_adapt_metric_enqueue): pf_nuts_metric_kernel is the step body of nuts_kernel.hip in its
// third mode, in a translation unit of its own (hmc_metric_kernel.hip says why).  One kernel serves a plain run of chains that carry a
// scale, RECORD_PATH included, and an adaptive run with metric windows.
#define PF_CHAIN_METRIC_TU
#include "nuts_kernel.hip"

struct NtMetricArgs : NtArgs {
    HmMetric M;
};

template <int KPAD, bool RES>
__global__ __launch_bounds__(HM_NT) void pf_nuts_metric_kernel(NtMetricArgs A_) { nt_step_body<KPAD, RES, NT_METRIC>(A_); }

struct NtMetricFamily {
    static constexpr bool has_warm = false;
    template <int KPAD, bool RES, bool ADAPT>
    static auto kernel() { return &pf_nuts_metric_kernel<KPAD, RES>; }
};

int32_t pf_launch_nuts_metric_step(pfmi_ctx *c, int64_t round, int64_t prow, bool reopen, hipStream_t s) {
    NtMetricArgs A;
    static_cast<NtArgs &>(A) = nt_args(c, round, prow, reopen);
    A.M = pf_chain_metric_args(c);
    return hm_launch_step<NtMetricFamily>(c, "nuts_metric", A, s);
}
