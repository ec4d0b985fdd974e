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
//
// ChEES-HMC (pfmi_chees_enqueue; Hoffman, Radul & Sountsov 2021), also stated ONCE here.  All K chains share one step size eps and one
// trajectory length tau; transition t (0-based, over warm-up and sampling, carried across CONTINUE) is static HMC's with
//     h_t = the base-2 radical inverse of t + 1 (pf_chees_halton: 1/2, 1/4, 3/4, 1/8, ...)
//     n   = ceil((h_t tau) / eps),   L_t = min(max(n, 1), Lmax);   n > Lmax sets PFMI_CHEES_CLAMPED          (pf_chees_leapfrog)
// leapfrog steps of size eps.  After warm-up transition t < W, from every chain's state x_k before it, trial point x'_k at its end,
// acceptance a_k (0 when divergent) and x-space end velocity u'_k = L_k v'_k -- chains with a_k = 0 are LEFT OUT of every sum over chains,
// which all run in chain order:
//     A = sum_k a_k;   xbar_i = (sum_k x_k,i) / K;   xbar'_i = (sum_k a_k x'_k,i) / A            (pf_chees_means: one fma per term)
//     p_k = sum_i (x_k,i - xbar_i)^2;  q_k = sum_i (x'_k,i - xbar'_i)^2;  r_k = sum_i (x'_k,i - xbar'_i) u'_k,i    (pf_chees_terms per i)
//     g  = ((h_t tau) sum_k a_k ((q_k - p_k) r_k)) / A;      hm = 0 if any a_k = 0, else K / sum_k (1 / a_k)
//     le = pf_adapt_update(da, hm), m = da.m;  eps+ = pf_adapt_pick(da, le, eps)
//     A > 0 and g finite:  s <- 0.95 s + 0.05 g^2,  b <- 0.95 b (b_0 = 1),  lt = log tau + 0.025 g / (sqrt(s / (1 - b)) + 1e-8)
//     else                 lt = log tau and PFMI_CHEES_KEPT_TRAJ
//     w = 1 / (sqrt(m) sqrt(sqrt(m)));  ltb <- w lt + (1 - w) ltb (ltb_0 = 0);  tau+ = min(max(exp(lt), eps+), Lmax eps+)
// (a tau+ that is not positive and finite keeps tau and sets PFMI_CHEES_KEPT_TRAJ).  After t = W - 1 sampling uses
// eps = pick(exp(leb)) and tau = min(max(exp(ltb), eps), Lmax eps); the jitter h_t stays.  (pf_chees_scalars)
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

// ---- ChEES-HMC
#define PF_CHEES_CLAMPED 8             // PFMI_CHEES_CLAMPED
#define PF_CHEES_KEPT_TRAJ 16          // PFMI_CHEES_KEPT_TRAJ
#define PF_CHEES_MAX_LEAPFROG 1024

struct PfChees {                       // the one shared state of a ChEES run (HBM); written by one thread per launch
    double eps, tau, s, b, ltb;
    PfAdapt da;
    int64_t t_upd, fin_round;          // the warm-up transition whose update is pending; the round in which the chains went idle
    int32_t Lmax, status, pending, pad_;
};

// the base-2 radical inverse of t + 1: its 32 bits reversed, times 2^-32
PF_ADAPT_HD inline double pf_chees_halton(int64_t t) {
    uint32_t n = (uint32_t)(t + 1);
    n = (n >> 16) | (n << 16);
    n = ((n & 0xff00ff00u) >> 8) | ((n & 0x00ff00ffu) << 8);
    n = ((n & 0xf0f0f0f0u) >> 4) | ((n & 0x0f0f0f0fu) << 4);
    n = ((n & 0xccccccccu) >> 2) | ((n & 0x33333333u) << 2);
    n = ((n & 0xaaaaaaaau) >> 1) | ((n & 0x55555555u) << 1);
    return (double)n * 0x1p-32;
}

// L_t; *clamped: n > Lmax.  (An n that is not a number steps once.)
PF_ADAPT_HD inline int32_t pf_chees_leapfrog(int64_t t, double tau, double eps, int32_t Lmax, bool *clamped) {
    const double n = ceil((pf_chees_halton(t) * tau) / eps);
    *clamped = n > (double)Lmax;
    if (!(n >= 1.0)) return 1;
    return *clamped ? Lmax : (int32_t)n;
}

// A (returned), xbar_i and xbar'_i of coordinate i: x, xp [K][d], a [K]
PF_ADAPT_HD inline double pf_chees_means(int K, int d, int i, const double *x, const double *xp, const double *a, double *xb, double *xbp) {
    double A = 0.0, sx = 0.0, sp = 0.0;
    for (int k = 0; k < K; ++k) {
        sx += x[(size_t)k * d + i];
        if (a[k] != 0.0) { A += a[k]; sp = fma(a[k], xp[(size_t)k * d + i], sp); }
    }
    *xb = sx / (double)K; *xbp = sp / A;
    return A;
}

// coordinate i's terms of p_k, q_k and r_k, added to the caller's partial sums
PF_ADAPT_HD inline void pf_chees_terms(double x, double xp, double u, double xb, double xbp, bool left_out, double &p, double &q, double &r) {
    const double dx = x - xb;
    p = fma(dx, dx, p);
    if (left_out) return;
    const double dp = xp - xbp;
    q = fma(dp, dp, q);
    r = fma(dp, u, r);
}

// The scalar part of the update after a warm-up transition with jitter h (`last`: after the last one), on a [K] and
// pqr = {p [K], q [K], r [K]}: the new state; *g_out, *hm_out the gradient and the harmonic mean it used.
PF_ADAPT_HD inline void pf_chees_scalars(PfChees &C, int K, const double *a, const double *pqr, double h, bool last, double *g_out, double *hm_out) {
    const double Lm = (double)C.Lmax;
    double A = 0.0, S = 0.0, inv = 0.0;
    bool zero = false;
    for (int k = 0; k < K; ++k) {
        if (a[k] == 0.0) { zero = true; continue; }
        A += a[k];
        inv += 1.0 / a[k];
        S += a[k] * ((pqr[K + k] - pqr[k]) * pqr[2 * K + k]);
    }
    const double g = ((h * C.tau) * S) / A, hm = zero ? 0.0 : (double)K / inv;
    const double le = pf_adapt_update(C.da, hm), sm = sqrt((double)C.da.m);
    const double en = pf_adapt_pick(C.da, last ? C.da.leb : le, C.eps);
    double lt = log(C.tau);
    if (A > 0.0 && fabs(g) <= 1.79769313486231570815e308) {
        C.s = 0.95 * C.s + 0.05 * (g * g);
        C.b = 0.95 * C.b;
        lt += 0.025 * g / (sqrt(C.s / (1.0 - C.b)) + 1e-8);
    } else C.status |= PF_CHEES_KEPT_TRAJ;
    const double w = 1.0 / (sm * sqrt(sm));
    C.ltb = w * lt + (1.0 - w) * C.ltb;
    const double te = exp(last ? C.ltb : lt);
    if (te > 0.0 && te <= 1.79769313486231570815e308) C.tau = fmin(fmax(te, en), Lm * en); else C.status |= PF_CHEES_KEPT_TRAJ;
    C.eps = en;
    *g_out = g; *hm_out = hm;
}
