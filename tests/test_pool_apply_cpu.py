"""CPU side of the pooled low-rank covariance (pfmi_pool_apply, importance_lowrank_covariance): the longdouble reference the GPU tests
compare against, the subspace iteration (pfmi.api._lowrank_from_apply) driven by a NumPy apply on planted-spectrum pools, the carry
chaining on a NumPy stand-in of the primitive, the ABI declarations and the resources of the kernels' instantiations."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from pool_apply_reference import LD, U, bound, bound_scores, pool_apply, pool_scores, propagated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pool(seed, d, N_r, K, zeros=0.1):
    """a correlated pool (d, N_r, K) with heavy-tailed weights, a share of them exact zeros"""
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
    P = np.einsum("ij,jnk->ink", L, rng.normal(size=(d, N_r, K))) + rng.normal(size=(d, 1, 1)) * 3.0
    w = rng.pareto(1.2, size=K * N_r) + 1e-3
    w[rng.uniform(size=K * N_r) < zeros] = 0.0
    return np.ascontiguousarray(P), w


@pytest.mark.parametrize("seed,d,N_r,K,r", [(1, 3, 40, 2, 1), (2, 7, 111, 3, 5), (3, 12, 5, 4, 12)])
def test_reference_is_numpy(seed, d, N_r, K, r):
    P, w = _pool(seed, d, N_r, K)
    P2 = P.reshape(d, N_r * K, order="F")
    rng = np.random.default_rng(seed + 10)
    V, c, y_in = rng.normal(size=(r, d)), rng.normal(size=d), rng.normal(size=(r, d))
    for ww in (w, None):
        for cc in (c, None):
            T = P2 - (0.0 if cc is None else cc[:, None])
            wv = np.ones(N_r * K) if ww is None else ww
            Z, Az = pool_scores(P, ww, cc, V)
            Zn = (V @ T).T
            Zn[wv == 0.0] = 0.0
            np.testing.assert_allclose(Z.astype(np.float64), Zn, rtol=1e-12, atol=1e-12 * np.abs(Zn).max())
            assert np.all(np.abs(Z) <= Az * (1 + 1e-15)) and np.all(bound_scores(d, Az) >= 0)
            assert np.all(Z[wv == 0.0] == 0) and np.all(Az[wv == 0.0] == 0)
            for yy in (None, y_in):
                Y, Ay = pool_apply(P, ww, cc, Z, yy)
                Yn = ((T * wv) @ Zn).T + (0.0 if yy is None else yy)
                np.testing.assert_allclose(Y.astype(np.float64), Yn, rtol=1e-11, atol=1e-12 * np.abs(Yn).max())
                assert np.all(np.abs(Y) <= Ay * (1 + 1e-15)) and np.all(bound(K * N_r + 1, Ay) >= 0)
            # the apply is the cross moments times the directions, and a subset of the coordinates is that subset of the result
            C = (T * wv) @ T.T
            np.testing.assert_allclose(pool_apply(P, ww, cc, Z)[0].astype(np.float64), V @ C, rtol=1e-10, atol=1e-11 * np.abs(V @ C).max())
            rows = np.array([d - 1, 0])
            for full, part in zip(pool_apply(P, ww, cc, Z, y_in), pool_apply(P, ww, cc, Z, y_in, rows=rows)):
                np.testing.assert_array_equal(full[:, rows], part)
            assert propagated(P, ww, cc, Az).shape == (r, d) and np.all(propagated(P, ww, cc, Az) >= 0)
            np.testing.assert_array_equal(propagated(P, ww, cc, Az)[:, rows], propagated(P, ww, cc, Az, rows=rows))


def test_reference_rules():
    P, w = _pool(4, 5, 30, 2)
    d, N_r, K = P.shape
    V = np.random.default_rng(1).normal(size=(3, d))
    V[1, 2] = 0.0
    Z, Az = pool_scores(P, w, None, V)
    Y, Ay = pool_apply(P, w, None, Z)
    # a zero weight skips the column whatever it holds: its scores are exact zeros and it adds nothing
    Pn = P.copy()
    z = int(np.flatnonzero(w == 0)[0])
    Pn[:, z % N_r, z // N_r] = np.nan
    Pn[1, z % N_r, z // N_r] = np.inf
    Zz, Azz = pool_scores(Pn, w, None, V)
    np.testing.assert_array_equal(Zz, Z)
    np.testing.assert_array_equal(Azz, Az)
    assert np.all(Zz[z] == 0)
    for a, b in zip(pool_apply(Pn, w, None, Zz), (Y, Ay)):
        np.testing.assert_array_equal(a, b)
    # unit weights skip nothing: the NaN column has NaN scores (also against the zero of V[1][2]) and poisons all of Y
    Zu, _ = pool_scores(Pn, None, None, V)
    assert np.all(np.isnan(Zu[z])) and np.count_nonzero(np.isnan(Zu)) == 3
    assert np.all(np.isnan(pool_apply(Pn, None, None, Zu)[0]))
    # one NaN in row 2 of a counted column: that column's scores, every direction, and with them every entry of Y
    c = int(np.flatnonzero(w != 0)[2])
    Pr = P.copy()
    Pr[2, c % N_r, c // N_r] = np.nan
    Zr, _ = pool_scores(Pr, w, P[:, 1, 1], V)
    bad = np.zeros(Zr.shape, dtype=bool)
    bad[c] = True
    np.testing.assert_array_equal(np.isnan(Zr), bad)
    assert np.all(np.isnan(pool_apply(Pr, w, P[:, 1, 1], Zr)[0]))
    # any non-zero weight counts
    wn = w.copy()
    wn[z] = 1e-300
    assert np.all(np.isnan(pool_scores(Pn, wn, None, V)[0][z]))
    # a run whose weights are all zero changes nothing
    w0 = w.copy()
    w0[N_r:] = 0.0
    X = np.arange(15.0).reshape(3, 5)
    Z0, _ = pool_scores(P[:, :, 1:], w0[N_r:], None, V)
    assert np.all(Z0 == 0)
    np.testing.assert_array_equal(pool_apply(P[:, :, 1:], w0[N_r:], None, Z0, X)[0], X.astype(LD))


# ---- the subspace iteration on planted spectra ------------------------------------------------------------------------------------
def _planted(seed, d, S):
    """U0 diag(sqrt(400, 200, 100, 50)) G + noise G' + 3 with U0 (d, 4) orthonormal (fewer columns when d < 4), noise uniform(0.5, 1)
    per row; weights Pareto(1.5) + 1e-3"""
    rng = np.random.default_rng(seed)
    k = min(4, d)
    U0 = np.linalg.qr(rng.standard_normal((d, k)))[0]
    lam0 = np.array([400.0, 200.0, 100.0, 50.0])[:k]
    P = U0 @ (np.sqrt(lam0)[:, None] * rng.standard_normal((k, S))) + rng.uniform(0.5, 1.0, size=d)[:, None] * rng.standard_normal((d, S)) + 3.0
    return P, rng.pareto(1.5, size=S) + 1e-3


def _numpy_cov(P, w):
    """(mean, var, apply(Q) -> cov Q without forming cov, the dense cov) in float64"""
    W = w.sum()
    mean = (P * w).sum(axis=1) / W
    T = P - mean[:, None]
    delta = (T * w).sum(axis=1) / W
    var = (T * T * w).sum(axis=1) / W - delta ** 2

    def apply(Q):
        return (T * w) @ (T.T @ Q) / W - delta[:, None] * (delta @ Q)[None, :]
    return mean, var, apply, (T * w) @ T.T / W - np.outer(delta, delta)


def _result(pfmi, mean, var, out):
    lam, Uv, rho, passes, converged = out
    return pfmi.LowRankCovariance(mean, var, lam, Uv, np.maximum(var - (Uv * Uv) @ lam, 0.0), rho, passes, converged, 1.0, 0, float("nan"))


@pytest.mark.parametrize("d,S,rank", [(10, 150, 3), (65, 150, 4), (130, 400, 4)])
def test_planted_spectrum(d, S, rank):
    import pfmi
    from pfmi.api import _lowrank_from_apply
    P, w = _planted(d, d, S)
    mean, var, apply, C = _numpy_cov(P, w)
    out = _lowrank_from_apply(apply, d, rank)
    lr = _result(pfmi, mean, var, out)
    print(f"planted d={d} S={S} rank={rank}: passes={lr.passes} residuals={lr.residuals}")
    assert lr.converged and lr.passes <= 30
    assert lr.eigenvalues.shape == (rank,) and lr.eigenvectors.shape == (d, rank) and lr.residuals.shape == (rank,)
    assert np.all(np.diff(lr.eigenvalues) <= 0)
    np.testing.assert_allclose(lr.eigenvectors.T @ lr.eigenvectors, np.eye(rank), atol=1e-12)
    ev = np.linalg.eigvalsh(C)
    lam1 = ev[-1]
    # the residual inclusion theorem for symmetric matrices: an eigenvalue lies within |C u - lam u| of lam for a unit u
    for j in range(rank):
        assert np.min(np.abs(ev - lr.eigenvalues[j])) <= lr.residuals[j] + 64 * 2.0 ** -53 * d * lam1, j
    assert np.max(lr.residuals) <= 1e-6 * lr.eigenvalues[0]
    if rank + 8 >= d:                                               # b == d: the first pass is exact
        assert lr.passes == 1
        np.testing.assert_allclose(lr.eigenvalues, ev[::-1][:rank], rtol=1e-12)
    assert np.all(lr.diag >= 0)
    assert np.all(lr.diag > 0)                                      # (noise on every row: the remaining diagonal is positive here)
    D = lr.dense()
    np.testing.assert_allclose(D, D.T, rtol=0, atol=1e-13 * lam1)
    rng = np.random.default_rng(5)
    for x in (rng.standard_normal(d), rng.standard_normal((d, 3))):
        np.testing.assert_allclose(lr.mul(x), D @ x, rtol=1e-12, atol=1e-12 * np.abs(D @ x).max())
        back = D @ lr.solve(x)
        assert np.linalg.norm(back - x) <= 1e-10 * np.linalg.norm(x)
    sign, ld = np.linalg.slogdet(D)
    assert sign == 1.0 and abs(lr.logdet - ld) <= 1e-10 * (1 + abs(ld))
    # the same seed, the same bits; another seed, the same eigenvalues to the residuals
    again = _lowrank_from_apply(apply, d, rank)
    for a, b in zip(out, again):
        np.testing.assert_array_equal(a, b)
    other = _lowrank_from_apply(apply, d, rank, seed=1)
    np.testing.assert_allclose(other[0], out[0], atol=2 * 1e-6 * lam1 + 64 * 2.0 ** -53 * d * lam1)


def test_iteration_arguments_and_failures():
    import pfmi
    from pfmi.api import _lowrank_from_apply
    P, w = _planted(1, 10, 150)
    mean, var, apply, C = _numpy_cov(P, w)
    for bad in (0, 11, 33):
        with pytest.raises(ValueError):
            _lowrank_from_apply(apply, 10, bad)
    with pytest.raises(ValueError, match="not finite"):
        _lowrank_from_apply(lambda Q: np.full(Q.shape, np.nan), 10, 2)
    # max_passes is a cap, not an error: the result says it did not converge
    out = _lowrank_from_apply(apply, 10, 2, oversample=0, tol=0.0, max_passes=2)
    assert out[3] == 2 and out[4] is False
    # the block: b = min(d, 32, rank + oversample) columns are handed to the apply
    seen = []
    _lowrank_from_apply(lambda Q: (seen.append(Q.shape), apply(Q))[1], 10, 2, oversample=3, max_passes=1)
    assert seen == [(10, 5)]
    # a diag entry that is not positive: solve and logdet raise, mul and dense do not
    lr = _result(pfmi, mean, var, _lowrank_from_apply(apply, 10, 3))
    lr.diag[4] = 0.0
    with pytest.raises(pfmi.PosDefException):
        lr.solve(np.ones(10))
    with pytest.raises(pfmi.PosDefException):
        lr.logdet
    assert np.all(np.isfinite(lr.mul(np.ones(10)))) and lr.dense().shape == (10, 10)


# ---- sharding invariance: the carry chain ------------------------------------------------------------------------------------------
def _standin(P, w, k0, k1):
    """Engine.pool_apply of an engine that owns runs [k0, k1) of the pool, in float64 NumPy: a run's sum from zero, draw by draw, the
    runs' sums in run order on top of the carry"""
    d, N_r, _ = P.shape

    def apply_pass(center, V, carry):
        Y = np.zeros(V.shape) if carry is None else np.array(carry, dtype=np.float64)
        for k in range(k0, k1):
            run = np.zeros(V.shape)
            for n in range(N_r):
                wn = 1.0 if w is None else w[k * N_r + n]
                if w is not None and wn == 0.0:
                    continue
                t = P[:, n, k] - center
                run = run + np.outer(V @ t, wn * t)
            Y = Y + run
        return Y
    return apply_pass


@pytest.mark.parametrize("seed,d,N_r,K", [(5, 6, 30, 4), (6, 9, 17, 6)])
def test_carry_chained_host_logic_is_sharding_invariant(seed, d, N_r, K):
    from pfmi.api import _apply_of_pool, _blocks, _lowrank_from_apply
    P, w = _pool(seed, d, N_r, K)
    P2 = P.reshape(d, N_r * K, order="F")
    for ww in (w, None):
        wv = np.ones(N_r * K) if ww is None else ww
        W = wv.sum()
        mean = (P2 * wv).sum(axis=1) / W
        delta = ((P2 - mean[:, None]) * wv).sum(axis=1) / W
        out = []
        for nen in (1, 2, 3):
            passes = [_standin(P, ww, k0, k1) for k0, k1 in _blocks(K, nen)]
            assert len(passes) == nen

            def apply(Q):
                Y = _apply_of_pool(passes, mean, np.ascontiguousarray(Q.T)).T
                return Y / W - delta[:, None] * (delta @ Q)[None, :]
            out.append(_lowrank_from_apply(apply, d, 3, oversample=2, max_passes=4))
        for other in out[1:]:
            for a, b in zip(other, out[0]):
                np.testing.assert_array_equal(a, b)
        lam, Uv, rho, npass, _ = out[0]                             # (converged or not: the inclusion theorem holds for any residual)
        assert 1 <= npass <= 4
        ev = np.linalg.eigvalsh(np.cov(P2, aweights=wv, ddof=0))
        for j in range(3):
            assert np.min(np.abs(ev - lam[j])) <= rho[j] + 1e-11 * ev[-1]


# ---- binding -----------------------------------------------------------------------------------------------------------------------
def _c_to_ctypes(t):
    t = re.sub(r"\bconst\b", "", t).strip()
    if t.endswith("*"):
        base = t[:-1].strip()
        return {"double": ctypes.POINTER(ctypes.c_double), "int32_t": ctypes.POINTER(ctypes.c_int32), "pfmi_ctx": ctypes.c_void_p}[base]
    return {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[t]


def test_header_declares_pool_apply_and_the_binding_matches():
    import pfmi
    from pfmi import _lib
    raw = open(os.path.join(ROOT, "include", "pfmi.h")).read()
    assert re.search(r"#define\s+PFMI_POOL_APPLY_MAX_R\s+32\b", raw)
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int32_t\s+pfmi_pool_apply\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/pfmi.h does not declare pfmi_pool_apply"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    names = [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in params]
    assert names == ["ctx", "col_offset", "importance", "center", "r", "v", "y_in", "y_out", "scores"]
    ctypes_of_header = [_c_to_ctypes(re.sub(r"[A-Za-z_0-9]+$", "", p)) for p in params]
    assert "pfmi_pool_apply" in _lib.SYMBOLS
    assert _lib.ARGTYPES["pfmi_pool_apply"] == ctypes_of_header
    lib = pfmi.lib()
    assert list(lib.pfmi_pool_apply.argtypes) == ctypes_of_header and lib.pfmi_pool_apply.restype is ctypes.c_int32
    assert hasattr(pfmi.Engine, "pool_apply") and callable(pfmi.importance_lowrank_covariance)
    assert hasattr(pfmi.MultiPathfinderResult, "lowrank_covariance")
    assert {"mean", "var", "eigenvalues", "eigenvectors", "diag", "residuals", "passes", "converged", "ess", "ncandidates",
            "pareto_shape"} == set(pfmi.LowRankCovariance.__dataclass_fields__)
    for name in ("dense", "mul", "solve", "logdet"):
        assert hasattr(pfmi.LowRankCovariance, name)
    julia = open(os.path.join(ROOT, "pathfinder.jl_amd", "julia", "PathfinderMI355X.jl")).read()
    assert "ccall((:pfmi_pool_apply, libpfmi)" in julia


# ---- kernel resources ----------------------------------------------------------------------------------------------------------------
# <RB, V>: RB accumulator blocks of 16 directions, V rows per lane in the staging loads; and the combine kernel
_INSTANCES = ["pf_pool_scores_kernel<%d, %d>(" % t for t in ((1, 1), (1, 2), (2, 1), (2, 2))] + \
             ["pf_pool_apply_kernel<%d, %d>(" % t for t in ((1, 1), (1, 2), (2, 1), (2, 2))] + ["pf_pool_apply_combine_kernel("]


def test_pool_apply_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    t = kr.kernel_resources()
    found = [k for k in t if k.startswith("pf_pool_apply") or k.startswith("pf_pool_scores")]
    assert len(found) == len(_INSTANCES) == 9, found
    for inst in _INSTANCES:
        hits = [k for k in found if k.startswith(inst)]
        assert len(hits) == 1, (inst, hits)
        r = t[hits[0]]
        print(inst, {k: r.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (inst, r)
        assert r["group_segment_fixed_size"] <= 65536, (inst, r)
