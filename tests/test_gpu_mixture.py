"""The uniform mixture of fits on the device (pfmi_mixture_logpdf / Engine.mixture_logpdf / MixtureModel): the mixture density the
reference's multipathfinder returns as fit_distribution (src/multipath.jl:215-216, Distributions.MixtureModel).

Every component column must be the single-fit logpdf of pfmi_logpdf and of an extended-precision reference built from the fit's
factors; lse must be the log-sum-exp of the columns; the Python MixtureModel must be the list of components with the mixture
surface on top.  Points: draws of each component, another component's mean, and far points 50 standard deviations out along the
top eigenvector of the component's covariance."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.special import logsumexp

import margins as mg
from gpu_common import CASES, _targets
from helpers import ROOT, STANDIN_LIB, fit_seeds, make_traces
from mixture_reference import _chol_ld, _solve_ld, _top_eig, ref_logpdf  # noqa: F401  (the extended-precision reference)

pytestmark = pytest.mark.gpu


# ---- fits and points -----------------------------------------------------------------------------------------------------------------
def _fit(eng, tg, K, hl, seed=7, maxiters=1000):
    traces = make_traces(tg, K, seed, history_length=hl, maxiters=maxiters)
    eng.set_target(tg)
    eng.set_traces([t.points for t in traces], [t.gradients for t in traces])
    eng.fit_batch(hl)
    status, jeff, _, _ = eng.fit_status()
    ok = [p for p in range(eng.P) if status[p] == 0]
    assert ok
    pts = sorted(set(ok[::max(1, len(ok) // 5)][:5] + [ok[-1]]))
    return pts, {p: eng.get_fit(p, int(jeff[p])) for p in pts}


def _points(eng, pts, fits, ndraw=4):
    """draws of each component, the next component's mean, a far point of each component"""
    cols = []
    seeds = fit_seeds(max(pts) + 1, 11)
    for k, p in enumerate(pts):
        cols.append(eng.draws(p, seeds[p], ndraw)[0])
        cols.append(fits[pts[(k + 1) % len(pts)]]["mu"][:, None])
        lam, v = _top_eig(fits[p])
        cols.append((fits[p]["mu"] + 50 * np.sqrt(lam) * v)[:, None])
    return np.asfortranarray(np.concatenate(cols, axis=1))


def _set_kernel(pfmi_mod, mode):
    assert pfmi_mod.lib().pfmi_debug_set(b"PFMI_MIXTURE_KERNEL", mode.encode() if mode else None) == 0


def _check_case(pfmi_mod, eng, name, pts, fits, X):
    lse, comp = eng.mixture_logpdf(pts, X, componentwise=True)
    assert comp.shape == (X.shape[1], len(pts)) and lse.shape == (X.shape[1],)
    for k, p in enumerate(pts):
        single = eng.logpdf(p, X)
        ref = ref_logpdf(fits[p], X)
        assert np.all(np.isfinite(single))
        mg.check(name, "logq@mixture_vs_logpdf", np.abs(comp[:, k] - single) / (1 + np.abs(single)))
        mg.check(name, "logq@mixture_vs_longdouble", np.abs(comp[:, k] - ref) / (1 + np.abs(ref)))
    ref_lse = logsumexp(comp, axis=1)
    mg.check(name, "lse@mixture", np.abs(lse - ref_lse) / np.maximum(np.abs(ref_lse), 1.0), bound=1e-13)
    # the general path: pfmi_logpdf's own algebra per component, the bits of pfmi_logpdf
    _set_kernel(pfmi_mod, "lane")
    try:
        lse_l, comp_l = eng.mixture_logpdf(pts, X, componentwise=True)
    finally:
        _set_kernel(pfmi_mod, None)
    for k, p in enumerate(pts):
        np.testing.assert_array_equal(comp_l[:, k], eng.logpdf(p, X))
    mg.check(name, "logq@mixture_mfma_vs_lane", np.abs(comp - comp_l) / (1 + np.abs(comp_l)))
    return lse, comp


@pytest.mark.parametrize("case", CASES, ids=[f"{t}-K{K}-J{J}" for t, K, J in CASES])
def test_componentwise_equals_per_component_cases(pfmi_mod, eng, case):
    tname, K, hl = case
    tg = _targets(pfmi_mod)[tname]
    pts, fits = _fit(eng, tg, K, hl)
    _check_case(pfmi_mod, eng, f"{tname}-J{hl}", pts, fits, _points(eng, pts, fits))


@pytest.mark.parametrize("hl", [6, 10, 16, 20])
def test_componentwise_every_history_padding(pfmi_mod, eng, hl):
    """kpad 12, 20, 32 (main kernel) and 64 (general path)"""
    tg = pfmi_mod.t_lowrank(80, r=12, seed=4)
    pts, fits = _fit(eng, tg, 3, hl)
    _check_case(pfmi_mod, eng, f"lr80-J{hl}", pts, fits, _points(eng, pts, fits, ndraw=3))


def test_componentwise_factor_read_from_l2(pfmi_mod, eng):
    """d = 1000 at kpad 20: the factor does not fit in LDS beside the kernel's buffers, both passes read it from L2"""
    tg = pfmi_mod.t_lowrank(1000, r=8, seed=5)
    pts, fits = _fit(eng, tg, 2, 10, maxiters=80)
    _check_case(pfmi_mod, eng, "lr1000-J10", pts, fits, _points(eng, pts, fits, ndraw=3))


@pytest.mark.timeout(900)
def test_componentwise_large_d_tsqr_range(pfmi_mod, eng):
    """d = 4096: beyond the main kernel's registers (general path), fits from the TSQR kernel's range"""
    tg = pfmi_mod.t_lowrank(4096, r=8, seed=6)
    pts, fits = _fit(eng, tg, 2, 6, maxiters=60)
    assert len(pts) >= 2
    _check_case(pfmi_mod, eng, "lr4096-J6", pts, fits, _points(eng, pts, fits, ndraw=2))


@pytest.fixture(scope="module")
def lr50(pfmi_mod, eng):
    tg = _targets(pfmi_mod)["lr50"]
    pts, fits = _fit(eng, tg, 3, 6)
    return pts, fits, _points(eng, pts, fits)


def test_single_component_matches_logpdf(pfmi_mod, eng, lr50):
    """K = 1: the general path is pfmi_logpdf bit for bit; the main kernel sums in another order, within 4 ulp at the draws"""
    pts, fits, X = lr50
    for p in pts:
        single = eng.logpdf(p, X)
        lse, comp = eng.mixture_logpdf([p], X, componentwise=True)
        np.testing.assert_array_equal(lse, comp[:, 0])
        draws = np.isin(np.arange(X.shape[1]), np.arange(X.shape[1]).reshape(len(pts), -1)[:, :4].ravel())
        ulp = np.abs(lse - single) / np.spacing(np.abs(single))
        assert np.max(ulp[draws]) <= 4, np.max(ulp[draws])
        mg.check("lr50-J6", "logq@mixture_K1", np.abs(lse - single) / (1 + np.abs(single)))
        _set_kernel(pfmi_mod, "lane")
        try:
            np.testing.assert_array_equal(eng.mixture_logpdf([p], X), single)
        finally:
            _set_kernel(pfmi_mod, None)


def test_repeated_point_and_determinism(pfmi_mod, eng, lr50):
    pts, fits, X = lr50
    p = pts[-1]
    lse, comp = eng.mixture_logpdf([p, p, p], X, componentwise=True)
    assert np.array_equal(comp[:, 0], comp[:, 1]) and np.array_equal(comp[:, 0], comp[:, 2])
    want = comp[:, 0] + np.log(3.0)
    np.testing.assert_allclose(lse, want, rtol=1e-15, atol=1e-15)
    lse2, comp2 = eng.mixture_logpdf([p, p, p], X, componentwise=True)
    assert np.array_equal(lse, lse2) and np.array_equal(comp, comp2)
    l1 = eng.mixture_logpdf(pts, X)
    l2 = eng.mixture_logpdf(pts, X)
    assert np.array_equal(l1, l2)


def test_dev_route_equals_host_bit_for_bit(pfmi_mod, eng, lr50):
    import torch
    pts, fits, X = lr50
    lse, comp = eng.mixture_logpdf(pts, X, componentwise=True)
    Xt = torch.from_numpy(np.ascontiguousarray(X.T)).to(f"cuda:{eng.device}").t()     # (d, N), column-major storage
    lse_d, comp_d = eng.mixture_logpdf(pts, Xt, componentwise=True)
    assert lse_d.is_cuda and comp_d.shape == (X.shape[1], len(pts))
    np.testing.assert_array_equal(lse_d.cpu().numpy(), lse)
    np.testing.assert_array_equal(comp_d.cpu().numpy(), comp)
    np.testing.assert_array_equal(eng.mixture_logpdf(pts, Xt).cpu().numpy(), lse)
    # a row-major (d, N) tensor: Engine.mixture_logpdf makes the column-major copy the entry point reads
    np.testing.assert_array_equal(eng.mixture_logpdf(pts, torch.from_numpy(np.ascontiguousarray(X)).to(f"cuda:{eng.device}")).cpu().numpy(), lse)


def test_failed_fit_gives_nan(pfmi_mod):
    """a fit whose status is not PFMI_FIT_OK: NaN in its column and in lse, the other columns unaffected"""
    eng = pfmi_mod.Engine(0)
    try:
        _failed_fit(pfmi_mod, eng)
    finally:
        eng.close()


def _failed_fit(pfmi_mod, eng):
    # (the hand-built trace of test_gpu_fit.py's non-PD test fits with status OK on the device -- its bad pair is rejected by the
    # curvature check -- so this uses test_gpu_elbo.py's construction: a random walk with negative-curvature pairs accepted)
    d = 40
    rng = np.random.default_rng(0)
    bad_th, bad_gr = np.cumsum(rng.normal(size=(9, d)), 0), rng.normal(size=(9, d))
    tg = pfmi_mod.t_diag(d, seed=3)
    good = make_traces(tg, 1, 3)[0]
    eng.set_target(tg)
    eng.set_traces([bad_th, good.points], [bad_gr, good.gradients])
    eng.fit_batch(5, -1e300)
    status = eng.fit_status()[0]
    bad = [p for p in range(eng.P) if status[p] != 0]
    okp = [p for p in range(eng.P) if status[p] == 0]
    assert bad and okp, status                            # the check below cannot pass vacuously
    X = np.asfortranarray(np.random.default_rng(1).normal(size=(d, 20)))
    for mode in (None, "lane"):
        _set_kernel(pfmi_mod, mode)
        try:
            lse, comp = eng.mixture_logpdf([okp[-1], bad[0]], X, componentwise=True)
        finally:
            _set_kernel(pfmi_mod, None)
        assert np.all(np.isnan(comp[:, 1])) and np.all(np.isnan(lse))
        np.testing.assert_allclose(comp[:, 0], eng.logpdf(okp[-1], X), rtol=1e-12)


def test_errors(pfmi_mod, eng, lr50):
    pts, fits, X = lr50
    with pytest.raises(pfmi_mod.PfmiError) as ei:
        eng.mixture_logpdf([eng.P], X)
    assert ei.value.code == -1
    with pytest.raises(pfmi_mod.PfmiError) as ei:
        eng.mixture_logpdf([-1], X)
    assert ei.value.code == -1
    with pytest.raises(pfmi_mod.PfmiError) as ei:
        eng.mixture_logpdf(pts, np.zeros((eng.d, 0), order="F"))
    assert ei.value.code == -1
    with pytest.raises(pfmi_mod.PfmiError) as ei:
        eng.mixture_logpdf([], X)
    assert ei.value.code == -1
    fresh = pfmi_mod.Engine(0)
    try:
        with pytest.raises(pfmi_mod.PfmiError) as ei:
            fresh.mixture_logpdf([0], X)
        assert ei.value.code == -3
    finally:
        fresh.close()


# ---- public API --------------------------------------------------------------------------------------------------------------------
def test_multipathfinder_fit_distribution_is_a_mixture(pfmi_mod):
    eng = pfmi_mod.Engine(0)
    try:
        _api(pfmi_mod, eng)
    finally:
        eng.close()


def _api(pfmi_mod, eng):
    tg = pfmi_mod.t_lowrank(40, r=6, seed=2)
    res = pfmi_mod.multipathfinder(tg, 200, nruns=8, rng=pfmi_mod.HostRNG(4), engine=eng)
    mix = res.fit_distribution
    assert isinstance(mix, list) and isinstance(mix, pfmi_mod.MixtureModel) and mix.ncomponents == 8
    for k in range(8):
        assert mix.components[k] is res.pathfinder_results[k].fit_distribution
    np.testing.assert_array_equal(mix.probs, np.full(8, 1 / 8))
    np.testing.assert_array_equal(mix.mean(), np.mean(np.stack([c.mu for c in mix]), axis=0))
    X = np.asfortranarray(res.draws[:, :64])
    comp = mix.componentwise_logpdf(X)
    for k in range(8):
        np.testing.assert_array_equal(comp[:, k], eng.mixture_logpdf([mix[k].point], X, componentwise=True)[1][:, 0])
        mg.check("mixture-api", "logq@mixture_component", np.abs(comp[:, k] - mix[k].logpdf(X)) / (1 + np.abs(comp[:, k])))
    lp = mix.logpdf(X)
    np.testing.assert_allclose(lp, logsumexp(comp, axis=1) - np.log(8), rtol=1e-13)
    np.testing.assert_allclose(mix.pdf(X), np.exp(lp), rtol=1e-13)
    assert mix.logpdf(X[:, 3]) == lp[3]
    Xr, ids = mix.rand(pfmi_mod.HostRNG(3), 500)
    assert Xr.shape == (40, 500) and ids.min() >= 1 and ids.max() <= 8
    assert sum(np.count_nonzero(ids == k + 1) for k in range(8)) == 500
    rng = pfmi_mod.HostRNG(3)
    u = rng.rand(500)
    np.testing.assert_array_equal(ids, np.minimum(np.floor(8 * u).astype(np.int64), 7) + 1)
    seeds = rng.rand_u64(8)
    for k in range(8):
        cols = np.flatnonzero(ids == k + 1)
        if len(cols):
            np.testing.assert_array_equal(Xr[:, cols], eng.draws(mix[k].point, seeds[k], len(cols))[0])
    r2 = pfmi_mod.resample(res, 100)
    assert r2.fit_distribution is mix
    eng.set_target(tg)
    tr = make_traces(tg, 1, 9)
    eng.set_traces([t.points for t in tr], [t.gradients for t in tr])
    eng.fit_batch(6)
    with pytest.raises(pfmi_mod.StaleHandleError):
        mix.logpdf(X)
    with pytest.raises(pfmi_mod.StaleHandleError):
        mix.rand(pfmi_mod.HostRNG(1), 5)


_MULTI = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/pathfinder.jl_amd")
import pfmi
tg = pfmi.t_lowrank(60, r=6, seed=3)
one = pfmi.multipathfinder(tg, 200, nruns=8, rng=pfmi.HostRNG(6))
engs = [pfmi.Engine(0), pfmi.Engine(0)]
two = pfmi.multipathfinder(tg, 200, nruns=8, rng=pfmi.HostRNG(6), engines=engs)
assert len({id(c.engine) for c in two.fit_distribution}) == 2
X = np.asfortranarray(one.draws[:, :80])
c1, c2 = one.fit_distribution.componentwise_logpdf(X), two.fit_distribution.componentwise_logpdf(X)
assert np.array_equal(c1, c2), np.max(np.abs(c1 - c2))
l1, l2 = one.fit_distribution.logpdf(X), two.fit_distribution.logpdf(X)
err = np.max(np.abs(l1 - l2) / (1 + np.abs(l1)))
assert err <= 1e-14, err
print("mixture engines ok", err)
"""


@pytest.mark.timeout(600)
def test_mixture_over_two_engines():
    """engines=[Engine(0), Engine(0)] through the RCCL stand-in: the same component columns bit for bit, the mixture within 1e-14"""
    assert os.path.exists(STANDIN_LIB), "tests/rccl_standin/librccl_standin.so missing: run __graft_entry__.build()"
    env = dict(os.environ, PFMI_RCCL_LIB=STANDIN_LIB, PFMI_COMM_ALLOW_SHARED_GPU="1", PFMI_STANDIN_TIMEOUT_S="60")
    env.pop("PFMI_COMM_FORCE_RCCL", None)
    r = subprocess.run([sys.executable, "-c", _MULTI, ROOT], env=env, capture_output=True, text=True, timeout=550)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    assert "mixture engines ok" in r.stdout
