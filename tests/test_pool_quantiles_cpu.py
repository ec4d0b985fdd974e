"""CPU side of the pooled importance quantiles (pfmi_pool_cdf, importance_quantiles): the longdouble reference the GPU tests compare
against, the key map and the bracket search on a NumPy stand-in of the primitive, the ABI declarations and the registers of the
kernel's instantiations."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from pool_quantiles_reference import cdf, quantiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def _pool(seed, d, S, zeros=0.1):
    """a pool with heavy-tailed weights (a share of exact zeros), one skewed row and one row full of ties"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(d, S)) * rng.uniform(0.2, 5.0, size=(d, 1)) + rng.normal(size=(d, 1))
    X[0] = np.exp(3.0 * rng.normal(size=S))
    X[d - 1] = rng.integers(-2, 3, size=S).astype(np.float64)
    w = rng.pareto(1.2, size=S) + 1e-3
    w[rng.uniform(size=S) < zeros] = 0.0
    return X, w


def test_reference_with_unit_weights_is_numpy_inverted_cdf():
    for seed, d, S in ((1, 3, 111), (2, 5, 1000), (3, 4, 7)):
        X, _ = _pool(seed, d, S)
        probs = np.concatenate([[0.0, 1.0], PROBS, np.random.default_rng(seed).uniform(size=9)])
        q, margin = quantiles(X, None, probs)
        np.testing.assert_array_equal(q, np.quantile(X, probs, axis=1, method="inverted_cdf"))
        assert np.all(margin[2:] >= 0)


def test_reference_rules():
    X, w = _pool(4, 4, 200)
    q, _ = quantiles(X, w, PROBS)
    # a zero weight skips the column whatever it holds
    Xn = np.concatenate([X, np.full((4, 3), np.nan)], axis=1)
    Xn[1, -1] = -np.inf
    wn = np.concatenate([w, np.zeros(3)])
    np.testing.assert_array_equal(quantiles(Xn, wn, PROBS)[0], q)
    c = cdf(Xn, wn, np.zeros((1, 4)))
    assert not c["nanflag"].any()
    np.testing.assert_array_equal(c["below"], cdf(X, w, np.zeros((1, 4)))["below"])
    # any non-zero weight counts: the row of the NaN is NaN, the others only gain a column
    wn[-2] = 1e-300
    qn, _ = quantiles(Xn, wn, PROBS)
    assert np.all(np.isnan(qn)) and cdf(Xn, wn, np.zeros((1, 4)))["nanflag"].all()
    Xn[:3, -2] = 0.5
    qn, _ = quantiles(Xn, wn, PROBS)
    assert np.all(np.isnan(qn[:, 3])) and np.all(np.isfinite(qn[:, :3]))
    assert np.all(np.isnan(quantiles(X, None if False else np.zeros_like(w), PROBS)[0]))       # W == 0
    # p = 0: the smallest counted value; p = 1: the largest; every answer is an element of the row
    q01, _ = quantiles(X, w, [0.0, 1.0])
    np.testing.assert_array_equal(q01[0], X[:, w != 0].min(axis=1))
    np.testing.assert_array_equal(q01[1], X[:, w != 0].max(axis=1))
    for i in range(4):
        assert np.all(np.isin(q[:, i], X[i]))
    # ties: the weights of equal values are merged
    x = np.array([[1.0, 2.0, 2.0, 2.0, 3.0]])
    ww = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    qt, mt = quantiles(x, ww, [0.2, 0.21, 0.8, 0.81])
    np.testing.assert_array_equal(qt[:, 0], [1.0, 2.0, 2.0, 3.0])
    c = cdf(x, ww, np.array([[2.0], [2.5], [0.0], [np.inf]]))
    np.testing.assert_array_equal(c["wle"][:, 0].astype(np.float64), [4.0, 4.0, 0.0, 5.0])
    np.testing.assert_array_equal(c["below"][:, 0], [2.0, 2.0, -np.inf, 3.0])
    np.testing.assert_array_equal(c["above"][:, 0], [3.0, 3.0, 1.0, np.inf])


def test_key_map_is_monotone_and_invertible():
    from pfmi.api import _f64_key, _f64_unkey
    rng = np.random.default_rng(5)
    tiny = np.nextafter(0.0, 1.0)
    special = np.array([-np.inf, -1.7976931348623157e308, -1.0, -2.2250738585072014e-308, -tiny, -0.0, 0.0, tiny,
                        2.2250738585072014e-308, 1.0, 1.7976931348623157e308, np.inf])
    k = _f64_key(special)
    assert k.dtype == np.uint64 and np.all(k[1:] > k[:-1])
    assert int(k[6]) - int(k[5]) == 1                                 # -0.0 and +0.0 are neighbours
    x = np.concatenate([special, rng.normal(size=1000) * 10.0 ** rng.integers(-300, 300, size=1000),
                        rng.integers(0, 2 ** 63, size=1000).astype(np.uint64).view(np.float64)])
    x = x[~np.isnan(x)]
    back = _f64_unkey(_f64_key(x))
    np.testing.assert_array_equal(back.view(np.uint64), x.view(np.uint64))
    xs = np.unique(x[x != 0])                                         # (np.sort leaves -0.0 and +0.0 in either order)
    assert np.all(np.diff(_f64_key(xs).astype(object)) > 0)
    np.testing.assert_array_equal(_f64_unkey(_f64_key(xs[:-1]) + np.uint64(1))[xs[:-1] > 0], np.nextafter(xs[:-1], np.inf)[xs[:-1] > 0])


def _standin(X, w):
    """the primitive in float64 NumPy over the whole pool"""
    def cdf_pass(T):
        c = cdf(X, w, T)
        return c["wle"].astype(np.float64), c["below"], c["above"], c["nanflag"]
    return cdf_pass


@pytest.mark.parametrize("seed,d,S", [(11, 3, 111), (12, 8, 2000), (13, 5, 64000)])
@pytest.mark.parametrize("B", [6, 16])
def test_bracket_search_equals_the_reference(seed, d, S, B):
    from pfmi.api import _quantile_pass_cap, _quantile_search
    X, w = _pool(seed, d, S)
    for ww in (w, None):
        W = np.float64((w if ww is not None else np.ones(S)).astype(np.longdouble).sum())
        probs = np.array(PROBS[:32 // B] if B > 6 else PROBS)
        ref, margin = quantiles(X, ww, probs, W)
        if ww is not None:                                           # (unit weights: the sums are integers, exact in both)
            assert np.all(margin > 1e-9 * W)                         # the float64 stand-in decides every comparison as the reference
        q, passes = _quantile_search(_standin(X, ww), d, probs * W, B)
        print(f"bracket search d={d} S={S} B={B} weighted={ww is not None}: {passes} passes (cap {_quantile_pass_cap(B)})")
        np.testing.assert_array_equal(q, ref)
        assert passes <= _quantile_pass_cap(B)
    if ww is None:
        np.testing.assert_array_equal(q, np.quantile(X, probs, axis=1, method="inverted_cdf"))


def test_bracket_search_edges_and_clustered_rows():
    """p = 0 and p = 1, a NaN row, and rows whose values differ in their last bits around 1e300, 1e-300 and across zero: value
    splitting makes no progress there, and the key splitting still closes every bracket under the cap"""
    from pfmi.api import _f64_key, _f64_unkey, _quantile_pass_cap, _quantile_search
    rng = np.random.default_rng(21)
    S = 500
    rows = []
    for centre in (1e300, -1e300, 1e-300, -1e-300):
        rows.append(_f64_unkey(_f64_key(np.full(S, centre)) + rng.integers(0, 40, size=S).astype(np.uint64)))
    rows.append(np.concatenate([np.full(S // 2, -1e300), np.full(S - S // 2 - 1, 1e300), [1e-300]]))   # far apart, one point between
    rows.append(np.concatenate([-rng.uniform(size=S // 2) * 1e-310, rng.uniform(size=S - S // 2) * 1e-310]))  # subnormals about 0
    rows.append(np.full(S, 7.0))
    rows.append(rng.normal(size=S))
    X = np.stack(rows)
    w = rng.pareto(1.5, size=S) + 1e-3
    w[::7] = 0.0
    probs = np.array([0.0, 0.025, 0.5, 0.975, 1.0])
    for B in (2, 6):
        for ww in (w, None):
            W = np.float64((ww if ww is not None else np.ones(S)).astype(np.longdouble).sum())
            ref, _ = quantiles(X, ww, probs, W)
            q, passes = _quantile_search(_standin(X, ww), X.shape[0], probs * W, B)
            print(f"clustered rows B={B} weighted={ww is not None}: {passes} passes (cap {_quantile_pass_cap(B)})")
            np.testing.assert_array_equal(q, ref)
            assert passes <= _quantile_pass_cap(B)
    Xn = X.copy()
    Xn[2, 5] = np.nan
    Xn[3, 0] = np.nan                                                  # (weight 0: invisible)
    ref, _ = quantiles(Xn, w, probs)
    q, _ = _quantile_search(_standin(Xn, w), X.shape[0], probs * np.float64(w.astype(np.longdouble).sum()), 6)
    np.testing.assert_array_equal(q, ref)
    assert np.all(np.isnan(q[:, 2])) and np.all(np.isfinite(q[:, 3]))
    q, _ = _quantile_search(_standin(X, np.zeros(S)), X.shape[0], probs * 0.0, 6)
    assert np.all(np.isnan(q))


def _c_to_ctypes(t):
    t = re.sub(r"\bconst\b", "", t).strip()
    if t.endswith("*"):
        base = t[:-1].strip()
        return {"double": ctypes.POINTER(ctypes.c_double), "int32_t": ctypes.POINTER(ctypes.c_int32), "pfmi_ctx": ctypes.c_void_p}[base]
    return {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[t]


def test_header_declares_pool_cdf_and_the_binding_matches():
    import pfmi
    from pfmi import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfmi.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+pfmi_pool_cdf\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/pfmi.h does not declare pfmi_pool_cdf"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    names = [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in params]
    assert names == ["ctx", "col_offset", "importance", "nthr", "thresholds", "wle_in", "wle", "below", "above", "nanflag"]
    ctypes_of_header = [_c_to_ctypes(re.sub(r"[A-Za-z_0-9]+$", "", p)) for p in params]
    assert "pfmi_pool_cdf" in _lib.SYMBOLS
    assert _lib.ARGTYPES["pfmi_pool_cdf"] == ctypes_of_header
    lib = pfmi.lib()
    assert list(lib.pfmi_pool_cdf.argtypes) == ctypes_of_header and lib.pfmi_pool_cdf.restype is ctypes.c_int32
    assert hasattr(pfmi.Engine, "pool_cdf") and hasattr(pfmi.Engine, "pool_draws_dev") and callable(pfmi.importance_quantiles)
    assert "pfmi_pool_draws_dev" in _lib.SYMBOLS and hasattr(lib, "pfmi_pool_draws_dev")
    assert re.search(r"int32_t\s+pfmi_pool_draws_dev\s*\(\s*pfmi_ctx \*ctx, void \*\*dev_ptr, int64_t \*count\)\s*;", txt)
    assert hasattr(pfmi.MultiPathfinderResult, "quantiles")


# VGPRs of the shipped build per instantiation <V, NT, TS> (V rows per lane, NT thresholds per thread, TS threshold groups per
# workgroup); the pin allows 8 registers more.  The doubled workgroup <1, 16, 2> is 8 waves per CU: it needs <= 256.
_VGPRS = {(2, 4, 1): 110, (1, 4, 1): 86, (2, 8, 1): 226, (1, 8, 1): 126, (1, 16, 1): 206, (1, 16, 2): 241}


@pytest.mark.parametrize("inst", sorted(_VGPRS), ids=lambda t: "V%d-NT%d-TS%d" % t)
def test_pool_cdf_kernel_stays_in_registers(inst):
    sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    t = kr.kernel_resources()
    hits = [k for k in t if k.startswith("pf_pool_cdf_kernel<%d, %d, %d>(" % inst)]
    assert len(hits) == 1, hits
    r = t[hits[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] + r.get("agpr_count", 0) <= min(_VGPRS[inst] + 8, 256), r
    assert len([k for k in t if k.startswith("pf_pool_cdf_kernel<")]) == len(_VGPRS)
