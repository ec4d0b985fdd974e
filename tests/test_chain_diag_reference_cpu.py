"""Admits tests/chain_diag_reference.py, the numpy restatement of pfmi_chain_diagnostics (include/pfmi.h) that the GPU parity test
(tests/test_gpu_chain_diag.py) compares with: known behaviour on iid, AR(1), shifted, over-dispersed and tie-heavy chains, the split for
odd and minimal T, the constant and NaN rules, and -- on the very inputs of the GPU test -- the float64 vs long-double deviation per
quantity (the GPU bound is 8 x that figure, floor 2^-44) and the absence of coordinates with a decision margin below 1e-9."""
import numpy as np
import pytest

import chain_diag_reference as R


def _one(x, extended=False):
    """x (K, T) -> outputs of the one coordinate"""
    return R.coordinate(np.asarray(x, dtype=np.float64), extended)


def test_iid_normals_have_full_ess_and_rhat_one():
    """100 coordinates of 4 x 500 iid normals: the ESS estimators are unbiased for S' with a relative spread of about 2 / sqrt(J) ... taken
    from the replicates themselves: every coordinate within 5 standard deviations of the replicate mean, the mean within 5 % of S'"""
    x = np.random.default_rng(1).standard_normal((100, 500, 4))
    out = R.diagnostics(x)
    Sp = 2000
    for k in ("ess_mean", "ess_bulk", "ess_tail"):
        m, s = out[k].mean(), out[k].std(ddof=1)
        assert abs(m / Sp - 1.0) < (0.05 if k != "ess_tail" else 0.15), (k, m)     # the tail ESS is the minimum of two estimates: biased low
        assert np.all(np.abs(out[k] - m) < 5 * s), k
    assert np.all(out["rhat"] < 1.01) and np.all(out["rhat"] >= np.sqrt(1.0 - 1.0 / 250))     # var+ >= (n - 1) / n W
    assert np.allclose(out["mcse_mean"], out["sd"] / np.sqrt(out["ess_mean"]), rtol=1e-14)
    assert np.allclose(out["mean"], x.reshape(100, -1).mean(1), atol=1e-14) and np.allclose(out["sd"], x.reshape(100, -1).std(1, ddof=1), rtol=1e-13)


@pytest.mark.parametrize("phi", [0.5, 0.9])
def test_ar1_ess_ratio(phi):
    """ess_mean / S' of AR(1) chains against (1 - phi) / (1 + phi): the band is 5 standard errors of the mean of 200 seeded replicates,
    plus the estimator's known truncation bias of order tau / n"""
    T, K, reps = 1000, 4, 200
    x = R.ar1(np.random.default_rng(7), reps, T, K, phi)
    ratio = R.diagnostics(x)["ess_mean"] / (2 * K * (T // 2))
    want = (1 - phi) / (1 + phi)
    se = ratio.std(ddof=1) / np.sqrt(reps)
    tau = (1 + phi) / (1 - phi)
    assert abs(ratio.mean() - want) < 5 * se + want * 2 * tau / (T // 2), (ratio.mean(), want, se)


def test_shifted_chain_raises_rhat():
    x = np.random.default_rng(3).standard_normal((4, 200))
    assert _one(x)["rhat"] < 1.01
    x[0] += 1.0
    assert _one(x)["rhat"] > 1.1


def test_only_the_folded_rhat_sees_a_wider_chain():
    """one chain with 10 x the variance and the same location: Rhat(z(x)) stays near 1, Rhat(z(fold(x))) does not"""
    x = np.random.default_rng(4).standard_normal((4, 400))
    x[0] *= np.sqrt(10.0)
    y = R.split(x)
    bulk = R.series_stats(R.znorm(y), np.float64, want_ess=False)[1]
    fold = R.series_stats(R.znorm(np.abs(y - np.median(y))), np.float64, want_ess=False)[1]
    assert bulk < 1.01 and fold > 1.05, (bulk, fold)
    assert _one(x)["rhat"] == fold


def test_tie_heavy_ranks_are_average_ranks():
    x = R.tie_heavy(np.random.default_rng(5), 1, 300, 3)[0].T
    y = R.split(x)
    assert len(np.unique(y)) < 0.6 * y.size                        # ties are the normal case here
    assert np.array_equal(R.ranks(y), R.scipy_ranks(y))
    out = _one(x)
    assert all(np.isfinite(out[k]) for k in R.KEYS)


def test_split_of_odd_and_minimal_t():
    x = np.arange(18.0).reshape(2, 9)
    y = R.split(x)
    assert y.shape == (4, 4) and np.array_equal(y[0], [0, 1, 2, 3]) and np.array_equal(y[1], [5, 6, 7, 8]) and np.array_equal(y[3], [14, 15, 16, 17])
    a = np.random.default_rng(6).standard_normal((2, 9))
    b = a.copy()
    b[:, 4] += 100.0                                               # the middle draw moves mean and sd only
    oa, ob = _one(a), _one(b)
    assert oa["mean"] != ob["mean"] and oa["sd"] != ob["sd"]
    for k in ("ess_mean", "ess_bulk", "ess_tail", "rhat"):
        assert oa[k] == ob[k], k
    o8 = _one(np.random.default_rng(8).standard_normal((1, 8)))     # T = 8, K = 1: n = 4, one Geyer pair
    assert all(np.isfinite(o8[k]) for k in R.KEYS) and o8["ess_mean"] <= 8 * np.log10(8) + 1e-12


def test_constant_and_nan_rules():
    c = _one(np.full((2, 20), 0.1))                                # 40 x 0.1 is not an exact sum: the mean is the value all the same
    assert c["mean"] == 0.1 and c["sd"] == 0.0
    for k in ("mcse_mean", "ess_mean", "ess_bulk", "ess_tail", "rhat"):
        assert np.isnan(c[k]), k
    x = np.random.default_rng(9).standard_normal((2, 20))
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 7] = bad
        o = _one(y)
        assert all(np.isnan(o[k]) for k in R.KEYS), bad
    # chains that are constant at different values: W = 0, NaN and not infinity
    d = _one(np.repeat([[0.1], [0.7]], 20, axis=1))
    assert np.isnan(d["rhat"]) and np.isnan(d["ess_bulk"]) and d["sd"] > 0


def test_extended_precision_agrees_on_benign_input():
    x = R.make_input("ar", 6, 200, 4, seed=11)
    a, b = R.diagnostics(x), R.diagnostics(x, extended=True)
    for k in R.KEYS:
        assert R.deviation(a[k], b[k]) < 1e-12, k
    assert np.array_equal(a["margin"] < R.MARGIN_MIN, b["margin"] < R.MARGIN_MIN)


@pytest.mark.parametrize("kind,T,K", sorted({(c[0], c[2], c[3]) for c in R.CASES}))
def test_gpu_inputs_deviation_and_margins(kind, T, K):
    """the inputs of the GPU parity test: the float64 vs long-double deviation per quantity (printed: the GPU bound is 8 x this figure,
    floor 2^-44), equal NaN placement, and no decision margin below 1e-9 in either precision.  The margin is the sign test |P_j|, the one
    discontinuity of Geyer's rule.  The gap of the running minimum is counted and printed, not asserted: it is 0 or one ulp for up to
    14 % of the coordinates at T = 64 (tail indicators with a handful of ones repeat their P_j exactly), and the minimum is continuous,
    so those coordinates stay in the comparison -- the two precisions agree on them to the same 1e-10 as on all others."""
    x, r64, rld = R.base_data(kind, T, K)
    dev = {k: R.deviation(r64[k], rld[k]) for k in R.KEYS}
    print("CHAIN_DIAG_F64_VS_LD", kind, T, K, {k: "%.2e" % v for k, v in dev.items()}, "min margin %.2e" % rld["margin"].min(),
          "share with a gap below 1e-9: %.3f" % np.mean(rld["min_gap"] < R.MARGIN_MIN))
    for k in R.KEYS:
        assert np.array_equal(np.isnan(r64[k]), np.isnan(rld[k])), k
        assert dev[k] < 1e-10, (k, dev[k])                          # the two precisions take the same branches
    assert np.all(r64["margin"] >= R.MARGIN_MIN) and np.all(rld["margin"] >= R.MARGIN_MIN), (r64["margin"].min(), rld["margin"].min())
