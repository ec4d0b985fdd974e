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
//
// The metric windows (pfmi_hmc_adapt_metric_enqueue, pfmi_nuts_adapt_metric_enqueue), also stated ONCE here.  Chain k's metric is
// Sigma_k = L diag(c_k)^2 L' with L the factor of its fit point and c_k a per-coordinate scale: a kick is v += e c . (R g), a drift
// x += e L (c . v), nothing else of a transition changes, c = 1 is the fitted metric.  W warm-up transitions (pf_adapt_windows):
//     W < 20:  no window (PFMI_ADAPT_NO_METRIC_WINDOW): the step-size warm-up above.
//     else     init = 75, term = 50, base = 25;  if init + base + term > W:  init = floor(0.15 W), term = floor(0.10 W),
//              base = W - init - term.  end = W - term.  Windows are consecutive from init: one of nominal size s that starts at e ends
//              at e + s, or at `end` if e + s + 2 s - 1 >= end (the next window would not fit); the next nominal size is 2 s.
// (Stan's windowed adaptation, except that the first window takes the stretch test of the others.)  After every transition of a window,
// accepted or not, the chain forms u = L \ (x - x0) (PFMI_OP_WHITEN with the FIT's factor: hm_whiten, hmc_rows.h) and every coordinate
// takes one Welford update (pf_welford_update).  At the end of a window of n transitions (pf_metric_var)
//     D_i = (n / (n + 5)) M2_i / (n - 1) + 5 / (n + 5),     c_i = sqrt(D_i)
// -- shrinkage towards 1, the fitted metric.  If any D_i is not finite or not positive the chain keeps its scale
// (PFMI_ADAPT_KEPT_METRIC).  Then the Welford state is cleared and the dual averaging restarts from the step size eps the ordinary update
// of that transition proposes: m = 0, Hbar = leb = 0, mu = log(10 eps) (pf_adapt_restart).
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
#define PF_ADAPT_NO_METRIC_WINDOW 2    // PFMI_ADAPT_NO_METRIC_WINDOW
#define PF_ADAPT_KEPT_METRIC 4         // PFMI_ADAPT_KEPT_METRIC
#define PF_ADAPT_MAX_WINDOWS 32        // PFMI_ADAPT_MAX_WINDOWS: W < 2^31 gives fewer (the nominal sizes double from >= 15)
#define PF_ADAPT_MIN_WINDOWED 20       // the shortest warm-up with a metric window
#define PF_METRIC_SHRINK 5.0

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

// ---- the metric windows
// The windows of W warm-up transitions: returns their number (0: W < 20), ends[j] the exclusive end of window j (at most
// PF_ADAPT_MAX_WINDOWS entries are written), *init the first window's start, *term the transitions after the last window.
inline int pf_adapt_windows(int64_t W, int64_t *init, int64_t *term, int64_t *ends) {
    if (W < PF_ADAPT_MIN_WINDOWED) { *init = W; *term = 0; return 0; }
    int64_t i0 = 75, tm = 50, base = 25;
    if (i0 + base + tm > W) { i0 = 15 * W / 100; tm = 10 * W / 100; base = W - i0 - tm; }
    const int64_t end = W - tm;
    int n = 0;
    for (int64_t e = i0, s = base; e < end; s *= 2) {
        e = (e + s + 2 * s - 1 >= end) ? end : e + s;
        if (n < PF_ADAPT_MAX_WINDOWS) ends[n] = e;
        ++n;
    }
    *init = i0; *term = tm;
    return n;
}

// Welford's update of one coordinate on the n-th value u of a window (n = 1, 2, ...): four roundings
PF_ADAPT_HD inline void pf_welford_update(double n, double u, double &mean, double &m2) {
    const double dl = u - mean;
    mean += dl / n;
    m2 = fma(dl, u - mean, m2);
}

// the regularised variance of a window of n >= 2 values: D = (n / (n + 5)) M2 / (n - 1) + 5 / (n + 5); the scale is sqrt(D)
PF_ADAPT_HD inline double pf_metric_var(double n, double m2) {
    const double q = n + PF_METRIC_SHRINK;
    return fma(n / q, m2 / (n - 1.0), PF_METRIC_SHRINK / q);
}
PF_ADAPT_HD inline bool pf_metric_var_ok(double D) { return D > 0.0 && D <= 1.79769313486231570815e308; }

// the restart of the dual averaging at a window's end, from the step size the ordinary update has just proposed
PF_ADAPT_HD inline void pf_adapt_restart(PfAdapt &S, double eps) {
    S.hbar = 0.0; S.leb = 0.0; S.mu = log(10.0 * eps); S.m = 0;
}
