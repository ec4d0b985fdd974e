"""Reference of pfmi_chain_diagnostics (include/pfmi.h) in plain numpy + scipy.special.ndtri: rank-normalised split R-hat, bulk and tail
ESS, mean, sd and MCSE of the mean after Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021).

`diagnostics(x, extended=False)` accumulates every mean, variance and autocovariance in float64, `extended=True` in np.longdouble; the
ranks, the median, the quantiles and the normal quantile are the same float64 numbers in both (they are not accumulations).  A chain
(or a coordinate) whose values are all equal has that value as its mean, not the rounded sum / n, so that the W = 0 rule is exact under
any summation order.  Besides the
seven outputs it returns, per coordinate and over the four ESS series, the two figures of Geyer's rule that a different summation order
could disturb: "margin", the smallest |P_j| for j <= J -- the sign test that ends the sum is a discontinuity, so a coordinate with a tiny
margin is left out of ESS comparisons -- and "min_gap", the smallest gap |P'_{j-1} - P_j| of the running minimum.  The minimum is
continuous in both arguments: whichever one a tie picks, P' moves by no more than the rounding of P, so a small gap excludes nothing.
(It cannot: the tail indicators of 64-draw chains have a handful of ones, their P_j repeat exactly, and up to 14 % of such coordinates
have a gap of 0 or one ulp; test_chain_diag_reference_cpu.py counts them.)

Also here: the seeded inputs the CPU and the GPU tests share, and the deviation table between the two precisions that bounds the GPU
parity (tests/test_gpu_chain_diag.py)."""
import functools

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

KEYS = ("mean", "sd", "mcse_mean", "ess_mean", "ess_bulk", "ess_tail", "rhat")
FLOOR = 2.0 ** -44                     # floor of every parity bound
BOUND_FACTOR = 8.0                     # bound = 8 x the float64 vs long-double deviation of this reference
MARGIN_MIN = 1e-9                      # decision margins below this are left out of ESS comparisons
MARGIN_CAP = 0.02                      # ... and may be at most this share of the coordinates
TILE = 2048                            # CD_TILE of csrc/chain_diag_kernels.hip: S' values of one counting tile in LDS


def split(x):
    """x (K, T) -> the M = 2 K split chains (M, n): chain k's first and last n = T // 2 draws (odd T: the middle draw is in neither)"""
    K, T = x.shape
    n = T // 2
    y = np.empty((2 * K, n), dtype=x.dtype)
    y[0::2] = x[:, :n]
    y[1::2] = x[:, T - n:]
    return y


def ranks(v):
    """fractional ranks, ties given their average rank: #less + (#equal + 1) / 2"""
    s = np.sort(v, axis=None)
    f = np.ravel(v)
    return (0.5 * (np.searchsorted(s, f, side="left") + np.searchsorted(s, f, side="right") + 1)).reshape(v.shape)


def znorm(v):
    return ndtri((ranks(v) - 0.375) / (v.size + 0.25))


def series_stats(y, ft, want_ess=True):
    """(ess, rhat, margin, min_gap) of the split series y (M, n) with sums in the float type ft"""
    M, n = y.shape
    Sp = M * n
    y = y.astype(ft)
    ybar = np.where(np.all(y == y[:, :1], axis=1), y[:, 0], y.sum(axis=1) / ft(n))     # a constant chain: its value, exactly
    c = y - ybar[:, None]

    def gbar(t):                                                   # mean_m gamma_m(t)
        return ((c[:, :n - t] * c[:, t:]).sum(axis=1) / ft(n)).sum() / ft(M)

    W = ft(n) / ft(n - 1) * gbar(0)
    if not W > 0:
        return np.nan, np.nan, np.inf, np.inf
    mm = ybar.sum() / ft(M)
    varp = ft(n - 1) / ft(n) * W + ((ybar - mm) ** 2).sum() / ft(M - 1)
    rhat = float(np.sqrt(varp / W))
    if not want_ess:
        return np.nan, rhat, np.inf, np.inf

    def rho(t):
        return ft(1) if t == 0 else ft(1) - (W - gbar(t)) / varp

    NP = (n - 1) // 2                                              # pairs with 2 j + 1 <= n - 2
    total, prev, margin, gap, tail = ft(0), None, np.inf, np.inf, ft(0)
    for j in range(NP):
        r0 = rho(2 * j)
        P = r0 + rho(2 * j + 1)
        margin = min(margin, abs(float(P)))
        if not P > 0:
            tail = max(r0, ft(0))
            break
        if prev is not None:
            gap = min(gap, abs(float(prev - P)))
        prev = P if prev is None else min(prev, P)
        total += prev
    tau = ft(-1) + ft(2) * total + tail
    tau = max(tau, ft(1) / np.log10(ft(Sp)))
    return float(ft(Sp) / tau), rhat, margin, gap


def coordinate(x, extended=False):
    """the seven outputs and the decision margin of one coordinate x (K, T)"""
    ft = np.longdouble if extended else np.float64
    x = np.asarray(x, dtype=np.float64)
    K, T = x.shape
    if not np.all(np.isfinite(x)):
        return dict({k: np.nan for k in KEYS}, margin=np.inf, min_gap=np.inf)
    xl = x.astype(ft)
    mean = xl[0, 0] if np.all(xl == xl[0, 0]) else xl.sum() / ft(K * T)                   # all draws equal: that value, exactly
    sd = np.sqrt(((xl - mean) ** 2).sum() / ft(K * T - 1))
    y = split(x)
    z = znorm(y)
    zf = znorm(np.abs(y - np.median(y)))
    e_mean, _, m0, g0 = series_stats(y, ft)
    e_bulk, r1, m1, g1 = series_stats(z, ft)
    _, r2, _, _ = series_stats(zf, ft, want_ess=False)
    e05, _, m2, g2 = series_stats((y <= np.quantile(y, 0.05)).astype(np.float64), ft)
    e95, _, m3, g3 = series_stats((y <= np.quantile(y, 0.95)).astype(np.float64), ft)
    nanmin = np.nan if (e05 != e05 or e95 != e95) else min(e05, e95)
    nanmax = np.nan if (r1 != r1 or r2 != r2) else max(r1, r2)
    return {"mean": float(mean), "sd": float(sd), "mcse_mean": float(sd / np.sqrt(ft(e_mean))), "ess_mean": e_mean, "ess_bulk": e_bulk,
            "ess_tail": nanmin, "rhat": nanmax, "margin": min(m0, m1, m2, m3), "min_gap": min(g0, g1, g2, g3)}


def diagnostics(draws, extended=False):
    """draws (d, T, K) -> dict of KEYS, "margin" and "min_gap", (d,) arrays"""
    draws = np.asarray(draws, dtype=np.float64)
    rows = [coordinate(draws[i].T, extended) for i in range(draws.shape[0])]
    return {k: np.array([r[k] for r in rows]) for k in KEYS + ("margin", "min_gap")}


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
def ar1(rng, d, T, K, phi):
    """(d, T, K) stationary AR(1) chains with unit innovation variance scaled to unit marginal variance"""
    e = rng.standard_normal((d, T, K))
    x = np.empty((d, T, K))
    x[:, 0] = e[:, 0]
    s = np.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + s * e[:, t]
    return x


def tie_heavy(rng, d, T, K):
    """every state repeated 1 to 5 times (what rejected HMC transitions leave behind)"""
    x = np.empty((d, T, K))
    for i in range(d):
        for k in range(K):
            vals = rng.standard_normal(T)
            reps = rng.integers(1, 6, size=T)
            x[i, :, k] = np.repeat(vals, reps)[:T]
    return x


def make_input(kind, d, T, K, seed):
    """ar: AR(1), phi cycling over 0, 0.5, 0.9 by coordinate, location and scale varying; ties: tie_heavy; shift: chain 0 moved by 1 sd"""
    rng = np.random.default_rng(seed)
    if kind == "ar":
        x = np.concatenate([ar1(rng, 1, T, K, (0.0, 0.5, 0.9)[i % 3]) for i in range(d)])
        return x * (1.0 + 0.5 * np.arange(d))[:, None, None] + 3.0 * np.cos(np.arange(d))[:, None, None]
    if kind == "ties":
        return tie_heavy(rng, d, T, K)
    if kind == "shift":
        x = ar1(rng, d, T, K, 0.3)
        x[:, :, 0] += 1.0
        return x
    raise ValueError(kind)


# The parity cases of the GPU test, (kind, d, T, K): the whole grid of inputs, d, K and T, and S' = 2 K (T // 2) on either side of TILE.
# A coordinate's outputs do not depend on the other coordinates, so the cases of one (kind, T, K) are the first d coordinates of ONE input
# of DMAX coordinates and share its reference.
KINDS, DS, KS, TS = ("ar", "ties", "shift"), (1, 3, 64, 65, 130), (1, 2, 5), (8, 9, 64, 257)
DMAX = max(DS)
GRID = [(kind, d, T, K) for kind in KINDS for K in KS for T in TS for d in DS]
BOUNDARY = [("ties", 2, TILE, 1), ("ties", 2, TILE + 2, 1)]          # S' = TILE: one counting tile; TILE + 2: two
CASES = GRID + BOUNDARY


def case_name(case):
    return "%s-d%d-T%d-K%d" % case


@functools.lru_cache(maxsize=None)
def base_data(kind, T, K):
    """(draws (dmax, T, K), float64 reference, long-double reference) of one (kind, T, K); computed once per process, read-only"""
    dmax = DMAX if T <= max(TS) else 2
    x = make_input(kind, dmax, T, K, seed=1000 + 100 * KINDS.index(kind) + 10 * K + T)
    x.setflags(write=False)
    return x, diagnostics(x), diagnostics(x, extended=True)


def case_data(case):
    """(draws (d, T, K), float64 reference, long-double reference, float64 vs long-double deviation per quantity) of one case"""
    kind, d, T, K = case
    x, r64, rld = base_data(kind, T, K)
    r64, rld = {k: v[:d] for k, v in r64.items()}, {k: v[:d] for k, v in rld.items()}
    return x[:d], r64, rld, {k: deviation(r64[k], rld[k]) for k in KEYS}


def deviation(a, b):
    """max |a - b| / (1 + |b|) over the entries finite in b (NaN placement is compared separately)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = np.isfinite(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / (1.0 + np.abs(b[ok])))) if ok.any() else 0.0


def bound(dev):
    return max(BOUND_FACTOR * dev, FLOOR)


def scipy_ranks(v):
    return rankdata(np.ravel(v), method="average").reshape(np.shape(v))
