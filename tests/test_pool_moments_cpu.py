"""CPU side of the pooled importance summaries (pfmi_pool_moments, importance_summary): the longdouble reference the GPU tests
compare against, the host's in-order combination over runs, and the ABI declarations."""
import ctypes
import os
import re

import numpy as np

from pool_moments_reference import pool_moments, run_moments, summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_agrees_with_numpy_average_and_cov():
    rng = np.random.default_rng(3)
    d, N = 7, 200
    X = rng.normal(size=(d, N)) * rng.uniform(0.5, 3.0, size=(d, 1)) + rng.normal(size=(d, 1))
    w = rng.uniform(size=N) ** 3
    r = run_moments(X, w)
    W = r["wsum"][0]
    mean = (r["s1"] / W).astype(np.float64)
    np.testing.assert_allclose(mean, np.average(X, axis=1, weights=w), rtol=1e-13)
    rc = run_moments(X, w, mean)
    var = (rc["s2"] / W - (rc["s1"] / W) ** 2).astype(np.float64)
    np.testing.assert_allclose(var, np.diag(np.cov(X, aweights=w, ddof=0)), rtol=1e-12)
    np.testing.assert_allclose(float(r["wsum"][1]), np.sum(w * w), rtol=1e-14)
    np.testing.assert_allclose(rc["s2w"].astype(np.float64), np.sum((w * (X - mean[:, None])) ** 2, axis=1), rtol=1e-12)
    # uniform weights: the plain mean / variance, and every absolute sum dominates its sum
    u = run_moments(X)
    np.testing.assert_allclose((u["s1"] / N).astype(np.float64), X.mean(axis=1), rtol=1e-13)
    assert u["wsum"][0] == N and u["wsum"][1] == N
    for s, a in (("s1", "A1"), ("s2", "A2"), ("s2w", "A2w")):
        assert np.all(np.abs(r[s]) <= r[a])


def test_reference_zero_weight_skip_and_nan_propagation():
    rng = np.random.default_rng(4)
    X = rng.normal(size=(3, 10))
    w = rng.uniform(size=10)
    clean = run_moments(X, w)
    Xn, wn = X.copy(), w.copy()
    Xn = np.concatenate([Xn, np.full((3, 2), np.nan)], axis=1)
    Xn[1, -1] = np.inf
    wn = np.concatenate([wn, [0.0, 0.0]])
    skipped = run_moments(Xn, wn)
    for key in clean:
        np.testing.assert_array_equal(skipped[key], clean[key])
    wn[-1] = 1e-300                                          # any non-zero weight: the column counts, NaN / inf propagate
    bad = run_moments(Xn, wn)
    assert np.isnan(bad["s1"][0]) and np.isinf(bad["s1"][1]) and np.isnan(bad["s1"][2])
    np.testing.assert_array_equal(bad["wsum"][0], clean["wsum"][0] + np.longdouble(1e-300))
    uni = run_moments(Xn)                                    # without weights nothing is skipped
    assert np.all(np.isnan(uni["s1"].astype(np.float64)))


def test_pool_and_summary_stack_runs():
    rng = np.random.default_rng(5)
    P = np.asfortranarray(rng.normal(size=(4, 6, 3)))
    w = rng.uniform(size=18)
    m = pool_moments(P, w)
    assert m["s1"].shape == (3, 4) and m["wsum"].shape == (3, 2)
    np.testing.assert_array_equal(m["s2"][1], run_moments(P[:, :, 1], w[6:12])["s2"])
    s = summary(P, w)
    flat = P.reshape(4, 18, order="F")
    np.testing.assert_allclose(s["mean"].astype(np.float64), np.average(flat, axis=1, weights=w), rtol=1e-13)
    np.testing.assert_allclose(float(s["run_weights"].sum()), 1.0, rtol=1e-15)
    np.testing.assert_allclose(float(s["ess"]), w.sum() ** 2 / np.sum(w * w), rtol=1e-13)


def test_combine_moments_is_sharding_invariant():
    from pfmi.api import _combine_moments
    rng = np.random.default_rng(6)
    rows = rng.normal(size=(8, 13)) * 10.0 ** rng.integers(-8, 8, size=(8, 1))     # cancellation: the order of the adds matters
    ws = rng.uniform(size=(8, 2))
    whole = _combine_moments([rows])
    seq = np.zeros(13)
    for r in rows:
        seq = seq + r
    np.testing.assert_array_equal(whole, seq)
    for cuts in ((1, 7), (3, 3, 2), (8,)):
        edges = np.concatenate([[0], np.cumsum(cuts)])
        blocks = [rows[a:b] for a, b in zip(edges[:-1], edges[1:])]
        np.testing.assert_array_equal(_combine_moments(blocks), whole)
        np.testing.assert_array_equal(_combine_moments([ws[a:b] for a, b in zip(edges[:-1], edges[1:])]), _combine_moments([ws]))


def _c_to_ctypes(t):
    t = re.sub(r"\bconst\b", "", t).strip()
    if t.endswith("*"):
        base = t[:-1].strip()
        return {"double": ctypes.POINTER(ctypes.c_double), "pfmi_ctx": ctypes.c_void_p}[base]
    return {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[t]


def test_header_declares_pool_moments_and_the_binding_matches():
    import pfmi
    from pfmi import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfmi.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+pfmi_pool_moments\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/pfmi.h does not declare pfmi_pool_moments"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    names = [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in params]
    assert names == ["ctx", "col_offset", "importance", "center", "wsum", "s1", "s2", "s2w"]
    ctypes_of_header = [_c_to_ctypes(re.sub(r"[A-Za-z_0-9]+$", "", p)) for p in params]
    assert "pfmi_pool_moments" in _lib.SYMBOLS
    assert _lib.ARGTYPES["pfmi_pool_moments"] == ctypes_of_header
    lib = pfmi.lib()
    assert list(lib.pfmi_pool_moments.argtypes) == ctypes_of_header and lib.pfmi_pool_moments.restype is ctypes.c_int32
    assert hasattr(pfmi.Engine, "pool_moments") and callable(pfmi.importance_summary)
    assert hasattr(pfmi.MultiPathfinderResult, "summary")
    assert [f for f in pfmi.ImportanceSummary.__dataclass_fields__] == ["mean", "var", "std", "mcse_mean", "ess", "run_weights",
                                                                        "ncandidates", "pareto_shape"]
