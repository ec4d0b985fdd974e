// nuts_fused_metric_kernel.hip -- NUTS on the BUILT-IN targets with a per-chain, per-coordinate scale on the fit's factor (adapt.h: the
// metric windows; include/pfmi.h: pfmi_chain_scale_set, pfmi_nuts_fused_metric_enqueue): pf_nuts_fused_metric_kernel is the loop, carry,
// ticket and nt_publish of nuts_fused_kernel.hip (NT_FUSED_LOOP) around the round of nuts_kernel.hip in its NT_METRIC mode, in a
// translation unit of its own (hmc_fused_metric_kernel.hip says why).  One kernel serves a plain run of chains that carry a scale,
// RECORD_PATH included, and an adaptive run with metric windows.  Its arguments are NtFusedArgs with HmMetric M behind them, read through
// the kernel-argument segment as the round reads them.
//
// SCALE WRITTEN AND READ IN ONE LAUNCH.  In the step kernels a launch boundary lies between the end of a window, which writes M.scale
// (hm_metric_end, hmc_rows.h), and the next kick, which reads it.  Here both happen inside one launch.  That is safe ONLY because row i of
// the scale, of the Welford state (mean, M2), of the traces and of every vector of the chain's block is read and written by thread
// i % HM_NT alone (head row i of a Woodbury pass: by thread i), in program order: a thread always sees its own earlier stores.  So the
// scale pointer carries no __restrict__, no non-temporal and no read-only qualifier, and no pass may ever read a row of the scale that
// another thread owns.  (tests/test_gpu_fused_metric.py runs an adaptive run at a launch cap of 1, where every boundary is back, against
// the default cap: the bits must not differ.)
//
// Nothing new between workgroups: no grid barrier, no spin, no hand-over; the launch cap HM_FUSED_ROUNDS and its test hook apply as they are.
#define PF_FUSED_METRIC_TU             // (the loop, NtFusedArgs and the launch of nuts_fused_kernel.hip, not its kernel)
#include "nuts_fused_kernel.hip"

struct NtFusedMetricArgs : NtFusedArgs {
    HmMetric M;
};

template <int KPAD, bool RES, int TG>
__global__ __launch_bounds__(HM_NT) void pf_nuts_fused_metric_kernel(NtFusedMetricArgs A_) {
    NT_FUSED_LOOP(NtFusedMetricArgs, NT_METRIC)
}

struct NtFusedMetricFamily {
    static constexpr const char *plan = "nuts_fused_metric";
    template <int KPAD, bool RES, int TG>
    static auto kernel() { return &pf_nuts_fused_metric_kernel<KPAD, RES, TG>; }
};

int32_t pf_launch_nuts_fused_metric(pfmi_ctx *c, int64_t launch, int cap, bool reopen, hipStream_t s) {
    NtFusedMetricArgs A;
    A.M = pf_chain_metric_args(c);
    return nt_launch_fused<NtFusedMetricFamily>(c, A, launch, cap, reopen, s);
}
