"""CPU side of the pooled importance covariance (pfmi_pool_cross, importance_covariance): the longdouble reference the GPU tests compare
against, the carry chaining and the host algebra on a NumPy stand-in of the primitive, the ABI declarations and the registers of the
kernel's instantiations."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from pool_cross_reference import bound, covariance, pool_cross, run_cross

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _pool(seed, d, N_r, K, zeros=0.1):
    """a correlated pool (d, N_r, K) with heavy-tailed weights, a share of them exact zeros"""
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
    P = np.einsum("ij,jnk->ink", L, rng.normal(size=(d, N_r, K))) + rng.normal(size=(d, 1, 1)) * 3.0
    w = rng.pareto(1.2, size=K * N_r) + 1e-3
    w[rng.uniform(size=K * N_r) < zeros] = 0.0
    return np.ascontiguousarray(P), w


@pytest.mark.parametrize("seed,d,N_r,K", [(1, 3, 40, 2), (2, 7, 111, 3), (3, 12, 5, 4)])
def test_reference_is_numpy_weighted_covariance(seed, d, N_r, K):
    P, w = _pool(seed, d, N_r, K)
    P2 = P.reshape(d, N_r * K, order="F")
    for ww in (w, None):
        got = covariance(P, ww)
        aw = ww if ww is not None else np.ones(N_r * K)
        ref = np.cov(P2, aweights=aw, ddof=0)
        np.testing.assert_allclose(got["cov"].astype(np.float64), ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
        np.testing.assert_allclose(got["mean"].astype(np.float64), np.average(P2, axis=1, weights=aw), rtol=1e-12)
    np.testing.assert_allclose(covariance(P, None)["cov"].astype(np.float64), np.cov(P2, ddof=0), rtol=1e-12,
                               atol=1e-12 * np.abs(ref).max())
    # the pool is its runs added on top of the carry, and A bounds |C|
    X = np.random.default_rng(seed).normal(size=(d, d))
    C, A = pool_cross(P, w, P[:, 0, 0], X)
    parts = [run_cross(P[:, :, k], w[k * N_r:(k + 1) * N_r], P[:, 0, 0]) for k in range(K)]
    acc = X.astype(LD)
    for p in parts:                                                # run order, on top of the carry
        acc = acc + p[0]
    np.testing.assert_array_equal(C, acc)
    assert np.all(np.abs(C) <= A * (1 + 1e-15)) and np.all(bound(K * N_r + 1, A) >= 0)


def test_reference_rules():
    P, w = _pool(4, 5, 30, 2)
    d, N_r, K = P.shape
    C, A = pool_cross(P, w)
    # a zero weight skips the column whatever it holds
    Pn, wn = P.copy(), w.copy()
    z = int(np.flatnonzero(w == 0)[0])
    Pn[:, z % N_r, z // N_r] = np.nan
    Pn[1, z % N_r, z // N_r] = np.inf
    Cz, Az = pool_cross(Pn, wn)
    np.testing.assert_array_equal(Cz, C)
    np.testing.assert_array_equal(Az, A)
    # unit weights skip nothing: the non-finite column poisons everything (inf * inf = inf at [1][1]); one NaN in row r poisons
    # exactly row r and column r
    assert not np.any(np.isfinite(pool_cross(Pn, None)[0]))
    r, c = 3, int(np.flatnonzero(w != 0)[2])
    Pr = P.copy()
    Pr[r, c % N_r, c // N_r] = np.nan
    Cr, _ = pool_cross(Pr, w, P[:, 1, 1])
    Cc, _ = pool_cross(P, w, P[:, 1, 1])
    bad = np.zeros((d, d), dtype=bool)
    bad[r, :] = bad[:, r] = True
    assert np.all(np.isnan(Cr[bad])) and np.all(np.isfinite(Cr[~bad]))
    np.testing.assert_array_equal(Cr[~bad], Cc[~bad])
    # any non-zero weight counts
    wn[z] = 1e-300
    assert not np.any(np.isfinite(pool_cross(Pn, wn)[0]))
    # a run whose weights are all zero changes nothing
    w0 = w.copy()
    w0[N_r:] = 0.0
    X = np.arange(25.0).reshape(5, 5)
    np.testing.assert_array_equal(pool_cross(P[:, :, 1:], w0[N_r:], None, X)[0], X.astype(LD))


def _standin(P, w, k0, k1):
    """Engine.pool_cross of an engine that owns runs [k0, k1) of the pool, in float64 NumPy: one chain per entry, the runs in run
    order on top of the carry, only i >= j computed and mirrored"""
    d, N_r, _ = P.shape

    def cross_pass(center, carry):
        C = np.zeros((d, d)) if carry is None else np.array(carry, dtype=np.float64)
        for k in range(k0, k1):
            for n in range(N_r):
                wn = 1.0 if w is None else w[k * N_r + n]
                if w is not None and wn == 0.0:
                    continue
                t = P[:, n, k] - center
                C = C + np.outer(wn * t, t)
        L = np.tril(C)
        return L + np.tril(C, -1).T
    return cross_pass


def _host_sums(P, w, center):
    """what the two moment passes hand importance_covariance, in float64, the runs added in run order"""
    d, N_r, K = P.shape
    P2 = P.reshape(d, N_r * K, order="F")
    ww = np.ones(N_r * K) if w is None else w
    W, s1, s2 = 0.0, np.zeros(d), np.zeros(d)
    for k in range(K):
        sl = slice(k * N_r, (k + 1) * N_r)
        t = P2[:, sl] - (0.0 if center is None else center[:, None])
        W = W + ww[sl].sum()
        s1 = s1 + (ww[sl] * t).sum(axis=1)
        s2 = s2 + (ww[sl] * t * t).sum(axis=1)
    return W, s1, s2


@pytest.mark.parametrize("seed,d,N_r,K", [(5, 4, 30, 4), (6, 9, 17, 6)])
def test_carry_chained_host_logic_is_sharding_invariant(seed, d, N_r, K):
    from pfmi.api import _blocks, _covariance_from_sums, _cross_of_pool
    P, w = _pool(seed, d, N_r, K)
    for ww in (w, None):
        W, s1, _ = _host_sums(P, ww, None)
        mean = s1 / W
        _, c1, c2 = _host_sums(P, ww, mean)
        out = []
        for nen in (1, 2, 3, K):
            passes = [_standin(P, ww, k0, k1) for k0, k1 in _blocks(K, nen)]
            assert len(passes) == nen
            C = _cross_of_pool(passes, mean)
            out.append(_covariance_from_sums(C, c1, W))
        for cov, corr in out[1:]:
            np.testing.assert_array_equal(cov, out[0][0])
            np.testing.assert_array_equal(corr, out[0][1])
        cov, corr = out[0]
        np.testing.assert_array_equal(cov, cov.T)
        np.testing.assert_array_equal(corr, corr.T)
        # against the reference, and the diagonal by importance_summary's formula on the same sums
        ref = covariance(P, ww)
        np.testing.assert_allclose(cov, ref["cov"].astype(np.float64), rtol=1e-11, atol=1e-12 * np.abs(cov).max())
        C = _cross_of_pool([_standin(P, ww, 0, K)], mean)
        np.testing.assert_array_equal(np.diagonal(cov), np.diagonal(C) / W - (c1 / W) ** 2)
        np.testing.assert_allclose(np.diagonal(cov), c2 / W - (c1 / W) ** 2, rtol=1e-11)
        np.testing.assert_array_equal(np.diagonal(corr), np.ones(d))
        assert np.all(np.abs(corr) <= 1 + 1e-12)


def test_correlation_of_a_degenerate_coordinate_is_nan():
    from pfmi.api import _covariance_from_sums
    C = np.array([[2.0, 0.5, 0.0], [0.5, 1.0, 0.0], [0.0, 0.0, 0.0]])
    cov, corr = _covariance_from_sums(C, np.zeros(3), 2.0)
    np.testing.assert_array_equal(cov, C / 2.0)
    assert np.all(np.isnan(corr[2])) and np.all(np.isnan(corr[:, 2]))
    np.testing.assert_array_equal(np.diagonal(corr)[:2], [1.0, 1.0])
    assert corr[0, 1] == corr[1, 0] == 0.25 / np.sqrt(0.5)


def _c_to_ctypes(t):
    t = re.sub(r"\bconst\b", "", t).strip()
    if t.endswith("*"):
        base = t[:-1].strip()
        return {"double": ctypes.POINTER(ctypes.c_double), "int32_t": ctypes.POINTER(ctypes.c_int32), "pfmi_ctx": ctypes.c_void_p}[base]
    return {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[t]


def test_header_declares_pool_cross_and_the_binding_matches():
    import pfmi
    from pfmi import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfmi.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+pfmi_pool_cross\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/pfmi.h does not declare pfmi_pool_cross"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    names = [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in params]
    assert names == ["ctx", "col_offset", "importance", "center", "c_in", "c_out"]
    ctypes_of_header = [_c_to_ctypes(re.sub(r"[A-Za-z_0-9]+$", "", p)) for p in params]
    assert "pfmi_pool_cross" in _lib.SYMBOLS
    assert _lib.ARGTYPES["pfmi_pool_cross"] == ctypes_of_header
    lib = pfmi.lib()
    assert list(lib.pfmi_pool_cross.argtypes) == ctypes_of_header and lib.pfmi_pool_cross.restype is ctypes.c_int32
    assert hasattr(pfmi.Engine, "pool_cross") and callable(pfmi.importance_covariance)
    assert hasattr(pfmi.MultiPathfinderResult, "covariance") and hasattr(pfmi.MultiPathfinderResult, "correlation")
    assert {"mean", "cov", "corr", "ess", "ncandidates", "pareto_shape"} == set(pfmi.ImportanceCovariance.__dataclass_fields__)


# Register budget of the instantiations <T, V> (T x T tile, V rows per lane in the staging loads), accumulators included (the unified
# file: vgpr_count covers the AGPRs).  A lane holds (T / 32)^2 accumulators of 4 doubles = 8 (T / 32)^2 AGPRs, 32 registers of
# staged loads, and the addresses.  T = 64: three workgroups per CU (512 / 3, in units of 8).  T = 128: one wave per SIMD, the whole file.
_BUDGET = {(64, 1): (168, 32), (64, 2): (168, 32), (128, 1): (512, 128), (128, 2): (512, 128)}


@pytest.mark.parametrize("inst", sorted(_BUDGET), ids=lambda t: "T%d-V%d" % t)
def test_pool_cross_kernel_stays_in_registers(inst):
    sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    t = kr.kernel_resources()
    hits = [k for k in t if k.startswith("pf_pool_cross_kernel<%d, %d>(" % inst)]
    assert len(hits) == 1, hits
    r = t[hits[0]]
    vgprs, agprs = _BUDGET[inst]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, r
    assert r.get("agpr_count", 0) <= agprs and r["vgpr_count"] <= vgprs, r
    assert len([k for k in t if k.startswith("pf_pool_cross_kernel<")]) == len(_BUDGET)
