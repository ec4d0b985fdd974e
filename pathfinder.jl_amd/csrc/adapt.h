// adapt.h -- the step-size adaptation of the device warm-up (include/pfmi.h: pfmi_hmc_adapt_enqueue, pfmi_nuts_adapt_enqueue), stated ONCE
// for the host and the device: thread 0 of a chain's workgroup runs pf_adapt_update and pf_adapt_pick between recording warm-up transition t and opening
// transition t + 1 (hmc_kernel.hip, nuts_kernel.hip); pfmi_host_dual_averaging (api_adapt.hip) is the host build of the same source.
//
// Nesterov dual averaging (Hoffman & Gelman 2014, Algorithm 5 and section 3.2.1: gamma = 0.05, t0 = 10, kappa = 0.75 -- the constants of
// pfmi/hmc.py), per chain and per transition.  a_t: the acceptance statistic of warm-up transition t (0-based), m = t + 1, delta the target,
// mu = log(10 eps_0):
//     Hbar <- (1 - 1/(m + t0)) Hbar + (delta - a_t)/(m + t0)        Hbar_0 = 0
//     le    = mu - (sqrt(m)/gamma) Hbar
//     w     = m^(-3/4) = 1 / (sqrt(m) sqrt(sqrt(m)))                (no pow)
//     leb  <- w le + (1 - w) leb                                     leb_0 = 0
// exp(le) steps transition t + 1 while it is a warm-up transition; every later transition uses exp(leb) of the last update.  A step size
// that is zero or not finite is never taken: the chain keeps the one it has and PFMI_ADAPT_KEPT_STEP is set (pf_adapt_pick).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_ADAPT_HD __host__ __device__
#else
#define PF_ADAPT_HD
#endif

#define PF_DA_GAMMA 0.05
#define PF_DA_T0 10.0
#define PF_ADAPT_KEPT_STEP 1           // PFMI_ADAPT_KEPT_STEP

struct PfAdapt {                       // per-chain adaptation state (HBM, beside the chain scalars); read and written by thread 0 only
    double hbar, leb, mu, delta;
    int32_t m, flags;
};

struct PfWarmRow {                     // what warm-up transition t leaves instead of a row: the step size it used, a_t, divergent, leapfrog steps
    double eps, acc;
    int32_t div, nleap;
};

// the state before the first update (host: mu takes the host's log)
inline PfAdapt pf_adapt_init(double eps0, double delta) {
    PfAdapt S;
    S.hbar = 0.0; S.leb = 0.0; S.mu = log(10.0 * eps0); S.delta = delta; S.m = 0; S.flags = 0;
    return S;
}

// one update on the statistic a; returns le (S.leb holds leb): the caller takes the exponential of the one it steps with
PF_ADAPT_HD inline double pf_adapt_update(PfAdapt &S, double a) {
    const double m = (double)++S.m, q = m + PF_DA_T0;
    S.hbar = (1.0 - 1.0 / q) * S.hbar + (S.delta - a) / q;
    const double sm = sqrt(m);
    const double le = S.mu - (sm / PF_DA_GAMMA) * S.hbar;
    const double w = 1.0 / (sm * sqrt(sm));
    S.leb = w * le + (1.0 - w) * S.leb;
    return le;
}

// the step size a chain takes when an update proposes exp(log_cand) and it has `prev`
PF_ADAPT_HD inline double pf_adapt_pick(PfAdapt &S, double log_cand, double prev) {
    const double cand = exp(log_cand);
    if (cand > 0.0 && cand <= 1.79769313486231570815e308) return cand;
    S.flags |= PF_ADAPT_KEPT_STEP;
    return prev;
}
