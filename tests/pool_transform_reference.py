"""Reference side of the pool-transform / moment-matching tests (tests/test_pool_transform_cpu.py, tests/test_gpu_pool_transform.py).
Plain NumPy, no GPU.  Not collected by pytest.

  exact_move      the correctly rounded a x + b, element by element, through fractions.Fraction: the product and the sum are exact
                  rationals and Fraction -> float rounds once, to nearest even -- what one fused multiply-add returns.  (Long double
                  would not do: its 64-bit significand rounds a x + b once to 64 bits and a second time to 53.)
  ref_logp        logp of the three built-in targets at given columns in long double, with a bound c eps T per column for any
                  double evaluation of the same formula in ANY summation order (derivations at gauss_logp_ld / funnel_logp_ld)
  mm_loop         the moment-matching loop of pfmi.moment_match restated on a host pool: same steps, same order of trials, same
                  acceptance rule, the oracle's PSIS
  scenario        the loop's test scenario on the CPU oracle alone (its fits, its generator, its PSIS)
"""
from fractions import Fraction

import numpy as np

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON   # noqa: F401  (one long-double skip convention for the suite)

LD = np.longdouble
EPS = 2.0 ** -53            # unit roundoff of binary64


# ---- the move, exactly -----------------------------------------------------------------------------------------------------------------
def exact_move(scale, shift, X0):
    """fl(scale_i * X0[i, s] + shift_i) with ONE rounding, for a (d, S) array"""
    X0 = np.asarray(X0, dtype=np.float64)
    d = X0.shape[0]
    out = np.empty(X0.shape, dtype=np.float64)
    flat0, flat = X0.reshape(d, -1), out.reshape(d, -1)
    for i in range(d):
        a, b = Fraction(float(scale[i])), Fraction(float(shift[i]))
        flat[i] = [float(a * Fraction(x) + b) for x in flat0[i].tolist()]
    return out


def sum_log_scale(scale):
    """sum_i log scale_i added in index order in double: the host sum pfmi_pool_transform states (libm's log, as the library's)"""
    import math
    s = 0.0
    for a in np.asarray(scale, dtype=np.float64).tolist():
        s += math.log(a)
    return s


def moved_ratios(lp1, lq0, scale, wrong_sign=False):
    """(lq', lr') of the moved pool from logp at the moved columns and the as-built proposal density: lq' = lq0 - sum log scale,
    lr' = lp' - lq', each one double operation -- what the GPU tests demand of the device to the last bit.  wrong_sign: log|det A|
    added instead of subtracted (the deliberately wrong variant).  The error is a CONSTANT over the pool, so PSIS -- which is
    invariant under a shift of the log ratios -- and with it every decision of the loop cannot see it; only a comparison of the
    ratios themselves can."""
    sla = sum_log_scale(scale)
    lq1 = (lq0 + sla) if wrong_sign else (lq0 - sla)
    return lq1, lp1 - lq1


# ---- logp of the built-in targets in long double ---------------------------------------------------------------------------------------
RPAD_MAX = 16


def gauss_c(d):
    """The constant of the Gaussian family's bound.  With u = EPS and first-order terms only, for a double evaluation in any order:
      e_i = x_i - mean_i                 one rounding
      q   = sum_i a_i e_i e_i            a term carries 2 u (e squared) + 2 u (two products), a sum of d terms at most (d - 1) u:
                                         |dq| <= (d + 3) u sum_i |a_i| e_i^2
      tr_j = sum_i Wd_ij e_i             |dtr_j| <= (d + 1) u A_j,  A_j = sum_i |Wd_ij e_i|  (>= |tr_j|)
      g_j = sum_{l <= j} G_jl tr_l       over at most RPAD_MAX terms: |dg_j| <= (d + RPAD_MAX + 2) u B_j,  B_j = sum_l |G_jl| A_l  (>= |g_j|)
      corr = sum_j g_j^2                 |dcorr| <= (2 (d + RPAD_MAX + 2) + RPAD_MAX + 1) u sum_j B_j^2
      logp = offset - (q - corr) / 2     two more roundings: u |q - corr| / 2 + u |logp|
    so |dlogp| <= c u T with T = (sum_i |a_i| e_i^2 + sum_j B_j^2) / 2 + |offset| + |logp| and c = 2 d + 3 RPAD_MAX + 8 (the largest
    of the factors above, + 3 for the last two roundings and the neglected second-order terms)."""
    return 2 * d + 3 * RPAD_MAX + 8


def funnel_c(d):
    """The constant of the funnel's bound.  logp = -(t3^2 + (d - 1) tau + q exp(-tau)) / 2, tau = x_1, t3 = tau / 3, q = sum_{i >= 2} x_i^2:
      q                 a term carries u, the sum at most (d - 2) u:  |dq| <= (d - 1) u q
      exp(-tau)         the device's exp is within 2 u (its documented 1 ulp), the product one more: q exp(-tau) carries (d + 2) u
      t3^2              3 u;  (d - 1) tau: u;  two additions and the halving: 2 u on the partial sums
    so |dlogp| <= c u T with T = (t3^2 + |(d - 1) tau| + q exp(-tau)) / 2 + |logp| and c = d + 8."""
    return d + 8


def gauss_logp_ld(tg, X):
    """(logp, bound) of a Gaussian-family target (mean, a, Wd (d, r), G (r, r), offset) at the columns of X, in long double"""
    X = np.asarray(X, dtype=LD)
    d = X.shape[0]
    e = X - np.asarray(tg.mean, dtype=LD)[:, None]
    qt = np.asarray(tg.a, dtype=LD)[:, None] * e * e
    q = qt.sum(axis=0)
    corr = np.zeros(X.shape[1], dtype=LD)
    B2 = np.zeros(X.shape[1], dtype=LD)
    if tg.r:
        Wd, G = np.asarray(tg.Wd, dtype=LD), np.tril(np.asarray(tg.G, dtype=LD))
        tr = Wd.T @ e                                              # (r, S)
        A = np.abs(Wd).T @ np.abs(e)
        g = G @ tr
        corr = (g * g).sum(axis=0)
        B = np.abs(G) @ A
        B2 = (B * B).sum(axis=0)
    lp = LD(tg.offset) - (q - corr) / 2
    T = (np.abs(qt).sum(axis=0) + B2) / 2 + abs(LD(tg.offset)) + np.abs(lp)
    return lp, gauss_c(d) * EPS * T


def funnel_logp_ld(d, X):
    X = np.asarray(X, dtype=LD)
    tau = X[0]
    t3 = tau / 3
    q = (X[1:] * X[1:]).sum(axis=0)
    qe = q * np.exp(-tau)
    lp = -(t3 * t3 + (d - 1) * tau + qe) / 2
    T = (t3 * t3 + np.abs((d - 1) * tau) + qe) / 2 + np.abs(lp)
    return lp, funnel_c(d) * EPS * T


def ref_logp(tg, X):
    """(logp, bound) of a built-in pfmi target at the columns of X"""
    return funnel_logp_ld(tg.d, X) if tg.kind == 1 else gauss_logp_ld(tg, X)


# two correct double implementations (different summation orders) and the deliberately wrong ones
def gauss_logp_f64(tg, X, order="forward", wrong=None):
    X = np.asarray(X, dtype=np.float64)
    d, S = X.shape
    idx = range(d) if order == "forward" else range(d - 1, -1, -1)
    r = tg.r
    q, tr = np.zeros(S), np.zeros((max(r, 1), S))
    for i in idx:
        e = X[i] - tg.mean[i]
        q = q + tg.a[i] * e * e
        for j in range(r):
            tr[j] = tr[j] + tg.Wd[i, j] * e
    corr = np.zeros(S)
    for j in range(r):
        g = np.zeros(S)
        for l in range(j + 1):
            g = g + tg.G[j, l] * tr[l]
        corr = corr + g * g
    if wrong == "lowrank_sign":
        corr = -corr
    off = 0.0 if wrong == "no_offset" else tg.offset
    return off - 0.5 * (q - corr)


def funnel_logp_f64(d, X, order="forward"):
    X = np.asarray(X, dtype=np.float64)
    q = np.zeros(X.shape[1])
    for i in (range(1, d) if order == "forward" else range(d - 1, 0, -1)):
        q = q + X[i] * X[i]
    t3 = X[0] / 3.0
    return (t3 * t3 + (d - 1) * X[0] + q * np.exp(-X[0])) / -2.0


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
STEPS = ("T1", "T2")


def _moments(X, w):
    W = w.sum()
    m = (X @ w) / W
    Z = X - m[:, None]
    return m, ((Z * Z) @ w) / W - ((Z @ w) / W) ** 2


def step_map(step, m0, v0, m, v):
    if step == "T1":
        a = np.ones_like(m)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.sqrt(v / v0)
    return a, m - a * m0


def mm_loop(X0, lq0, logp, psis, *, k_threshold=0.7, max_iters=30, wrong_sign=False):
    """pfmi.moment_match on a host pool.  X0 (d, S): the pool as built; lq0 (S): the log density every column is divided by (the
    run's own proposal, or the mixture); logp(X) -> (S,); psis(lr) -> (log weights, weights, k-hat, tail length) (the oracle's).
    Returns dict(scale, shift, history, trials, X, lr, weights, k): history as pfmi's; trials: (step, a, b, scale, shift, m0, v0, m, v)
    of every trial.  wrong_sign: moved_ratios' wrong variant (for the test that shows what can and what cannot catch it)."""
    X0 = np.asarray(X0, dtype=np.float64)
    d = X0.shape[0]
    scale, shift = np.ones(d), np.zeros(d)
    X, lr = X0, logp(X0) - lq0
    _, w, k, _ = psis(lr)
    history, trials = [("start", float(k), True)], []
    ones = np.ones(X0.shape[1])
    for _ in range(max_iters):
        if not k > k_threshold:
            break
        m0, v0 = _moments(X, ones)
        m, v = _moments(X, w)
        accepted = False
        for step in STEPS:
            a, b = step_map(step, m0, v0, m, v)
            sc, sh = a * scale, a * shift + b
            trials.append((step, a, b, sc, sh, m0, v0, m, v))
            if not (np.all(np.isfinite(sc)) and np.all(sc > 0) and np.all(np.isfinite(sh))):
                history.append((step, float("nan"), False))
                continue
            Xn = sc[:, None] * X0 + sh[:, None]
            lrn = moved_ratios(logp(Xn), lq0, sc, wrong_sign=wrong_sign)[1]
            _, wn, kn, _ = psis(lrn)
            if np.isfinite(kn) and kn < k:
                X, lr, w, k, scale, shift, accepted = Xn, lrn, wn, kn, sc, sh, True
                history.append((step, float(kn), True))
                break
            history.append((step, float(kn), False))
        if not accepted:
            break
    return dict(scale=scale, shift=shift, history=history, trials=trials, X=X, lr=lr, weights=w, k=float(k))


# ---- the scenario of the loop tests -------------------------------------------------------------------------------------------------------
SC_D, SC_K, SC_NR, SC_J = 8, 3, 300, 6
SC_K_THRESHOLD = 0.0        # the loop tests run until no trial is accepted: accepted T1 and T2 moves and rejected trials all occur
SC_TRACE_SEED = 11
SC_DRAW_SEEDS = (1000, 1007, 1014)


def scenario_target(pfmi):
    """a diagonal Gaussian with shifted mean and alternating scales: what the pool of t_iso fits is matched to"""
    d = SC_D
    mean = 0.8 + 0.1 * np.arange(d)
    sig = np.where(np.arange(d) % 2 == 0, 0.6, 1.4)
    return pfmi.GaussTarget(mean, sig ** 2)


def scenario_traces(pfmi):
    from helpers import make_traces
    return make_traces(pfmi.t_iso(SC_D), SC_K, SC_TRACE_SEED, history_length=SC_J)


def scenario_oracle_pool(pfmi):
    """(X0 (d, K N_r), lq0) of the scenario from the oracle alone: every trace's last fit, N_r draws of the oracle's generator"""
    from gpu_common import _oracle_factor
    from oracle import pf_oracle as po
    Xs, lqs = [], []
    for k, tr in enumerate(scenario_traces(pfmi)):
        alpha_all, hl, hs, _ = po.lbfgs_history(tr.points, tr.gradients, SC_J)
        l, d = len(tr.points) - 1, tr.points.shape[1]
        F = _oracle_factor(tr, alpha_all, hl, hs, l, d)
        assert F.status == 0
        X, lq = F.rand_and_logpdf(F.fit_mean(tr.points[l], tr.gradients[l]), po.randn_fill(SC_DRAW_SEEDS[k], d, SC_NR))
        Xs.append(X)
        lqs.append(lq)
    return np.concatenate(Xs, axis=1), np.concatenate(lqs)


def scenario_logp(pfmi):
    from helpers import oracle_target
    otg = oracle_target(scenario_target(pfmi))
    return lambda X: otg.logp(np.asfortranarray(X))


def history_gaps(history):
    """|k-hat of a trial - the k-hat it was compared with| for every trial of a history"""
    gaps, k = [], history[0][1]
    for _, kn, acc in history[1:]:
        gaps.append(abs(kn - k))
        if acc:
            k = kn
    return gaps


def scenario_result(pfmi, engs, proposal="component"):
    """The scenario as a MultiPathfinderResult over `engs` (contiguous blocks of runs, as multipathfinder shards them): every engine
    fits its traces of t_iso, then takes the scenario's target -- pfmi_set_target leaves the fits in place -- so the pooled stage
    weights the fits of one target against another.  Only what the pooled stage reads is filled in."""
    from pfmi.api import _blocks
    traces, tg = scenario_traces(pfmi), scenario_target(pfmi)
    runs = []
    for eng, (k0, k1) in zip(engs, _blocks(SC_K, len(engs))):
        eng.set_target(pfmi.t_iso(SC_D))
        eng.set_traces([t.points for t in traces[k0:k1]], [t.gradients for t in traces[k0:k1]])
        eng.fit_batch(SC_J)
        eng.set_target(tg)
        for k in range(k0, k1):
            dist = pfmi.MvNormal(None, None, eng, int(eng.offsets[k - k0 + 1]) - 1, -1, eng.fit_token())
            runs.append(pfmi.PathfinderResult(None, None, None, dist, None, draw_seed=SC_DRAW_SEEDS[k], ndraws_per_run=SC_NR))
    placeholder = pfmi.PSISResult(None, None, float("nan"), 0)          # (importance weighting is on; the stage recomputes it)
    return pfmi.MultiPathfinderResult(tg, pfmi.HostRNG(5), tg.logp, pfmi.MixtureModel([r.fit_distribution for r in runs]),
                                      np.zeros((SC_D, 50)), np.zeros(50, dtype=np.int64), runs, placeholder, engs[0], SC_NR, list(engs),
                                      proposal)
