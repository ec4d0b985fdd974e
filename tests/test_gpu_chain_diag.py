"""pfmi_chain_diagnostics on the GPU (csrc/chain_diag_kernels.hip): parity of the uploaded route with the long-double reference
(tests/chain_diag_reference.py, admitted by tests/test_chain_diag_reference_cpu.py) over the grid of inputs, d, K and T and on either
side of the counting kernel's LDS-tile boundary; the resident route after a real HMC run, bit for bit; the public calls; every return
code of the C ABI.

Bounds: every quantity goes through margins.check with 8 x the float64 vs long-double deviation of the reference on the same input
(the figure test_chain_diag_reference_cpu.py prints), floor 2^-44 -- a different summation order is the only licensed difference.
Coordinates whose decision margin (smallest |P_j| of Geyer's sign test) is below 1e-9 are left out of the ESS comparison; they may be at
most 2 % of the coordinates.  NaN placement must be equal."""
import ctypes as C

import numpy as np
import pytest

import chain_diag_reference as R
import margins
from helpers import demo_device_target

pytestmark = pytest.mark.gpu

ESS_KEYS = ("mcse_mean", "ess_mean", "ess_bulk", "ess_tail")
PLANS = ("chain_diag:count:one", "chain_diag:count:tiled")


def _plan_counts(eng):
    return [eng.kernel_time(p)[1] for p in PLANS]


def _is_reference(got, x):
    """got == the long-double reference of x within 8 x the reference's own float64 vs long-double deviation (floor 2^-44)"""
    r64, ref = R.diagnostics(x), R.diagnostics(x, extended=True)
    for k in R.KEYS:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        assert np.array_equal(np.isnan(g), np.isnan(ref[k])), k
        ok = np.isfinite(ref[k]) & ((ref["margin"] >= R.MARGIN_MIN) if k in ESS_KEYS else True)
        assert np.all(margins.rel(g[ok], ref[k][ok]) <= R.bound(R.deviation(r64[k], ref[k]))), k
    return ref


def _parity(eng, case):
    x, _, ref, dev = R.case_data(case)
    kind, d, T, K = case
    got = eng.chain_diagnostics(x)
    small = ref["margin"] < R.MARGIN_MIN
    assert small.mean() <= R.MARGIN_CAP, (case, small.mean())
    for k in R.KEYS:
        assert got[k].shape == (d,)
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (case, k)
        use = np.isfinite(ref[k]) & (~small if k in ESS_KEYS else True)
        b = R.bound(dev[k])
        margins.check("chain_diag/%s-T%d-K%d" % (kind, T, K), k, margins.rel(got[k][use], ref[k][use]), bound=b,
                      why="8 x the float64 vs long-double deviation %.2e of the numpy reference on this input "
                          "(CHAIN_DIAG_F64_VS_LD, test_chain_diag_reference_cpu.py), floor 2^-44" % dev[k], ctx=case)
    return got


@pytest.mark.parametrize("case", R.GRID, ids=R.case_name)
def test_parity_with_the_long_double_reference(eng, case):
    _parity(eng, case)


@pytest.mark.parametrize("case,plan", list(zip(R.BOUNDARY, PLANS)), ids=lambda v: v if isinstance(v, str) else R.case_name(v))
def test_parity_on_either_side_of_the_counting_tile(eng, case, plan):
    """S' = 2048 values fill one LDS tile of the counting kernel exactly; S' = 2050 take a second, padded one"""
    before = _plan_counts(eng)
    _parity(eng, case)
    after = _plan_counts(eng)
    assert [a - b for a, b in zip(after, before)] == [int(p == plan) for p in PLANS], (plan, before, after)


def test_special_values(eng):
    """a non-finite draw: NaN everywhere for that coordinate alone; a constant coordinate: mean and sd, NaN for ESS and R-hat; chains constant at
    different values (W = 0): NaN, not infinity; a constant tail indicator cannot occur with finite non-constant draws"""
    x = np.array(R.make_input("ar", 6, 20, 2, seed=77))
    x[1, 7, 1] = np.nan
    x[2, 0, 0] = np.inf
    x[3] = 0.1                                                     # 40 x 0.1 and 10 x 0.7 are not exact sums
    x[4, :, 0], x[4, :, 1] = 0.1, 0.7
    got = eng.chain_diagnostics(x)
    _is_reference(got, x)
    assert all(np.isnan(got[k][1]) and np.isnan(got[k][2]) for k in R.KEYS)
    assert got["mean"][3] == 0.1 and got["sd"][3] == 0.0 and np.isnan(got["rhat"][3]) and np.isnan(got["ess_bulk"][3]) and np.isnan(got["mcse_mean"][3])
    assert got["sd"][4] > 0 and np.isnan(got["rhat"][4]) and np.isnan(got["ess_tail"][4])
    assert all(np.isfinite(got[k][[0, 5]]).all() for k in R.KEYS)


# ---- the resident route: the `small` set-up of test_gpu_hmc.py, rebuilt here ------------------------------------------------------------
HMC_T, HMC_LF = 40, 3


@pytest.fixture(scope="module")
def hmc_run(pfmi_mod, eng):
    """d = 20, J = 6, two closure-optimised paths, four chains; returns the arguments of the run"""
    tg = pfmi_mod.t_lowrank(20, r=2, seed=2, wscale=0.5)
    eng.set_target(demo_device_target(tg, grad=True))
    x0 = pfmi_mod.HostRNG(5).rand(2 * tg.d).reshape(2, tg.d) * 4.0 - 2.0
    eng.optimize_batch(x0, 6, 40, 1e-8)
    eng.fit_batch(6)
    status, off = eng.fit_status()[0], eng.offsets
    pts = np.array([0, 2, off[1] - 1, off[2] - 1], dtype=np.int64)
    assert np.all(status[pts] == 0)
    start = np.asfortranarray(tg.mean[:, None] + 0.3 * np.random.default_rng(1).standard_normal((20, 4)))
    seeds = np.asarray(pfmi_mod.hostrng.rand_u64(31, np.arange(4, dtype=np.uint64), 9), dtype=np.uint64)
    return pts, start, seeds, np.array([0.2, 0.3, 0.25, 0.35])


def _run(eng, args, T, **kw):
    pts, start, seeds, eps = args
    eng.hmc_enqueue(pts, None if kw.get("cont") else start, seeds, eps, HMC_LF, T, **kw)
    eng.hmc_wait()
    return eng.hmc_get()


def _same_bits(a, b, keys=R.KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_resident_route_is_the_uploaded_route_bit_for_bit(eng, hmc_run):
    rec = _run(eng, hmc_run, HMC_T)
    res = eng.chain_diagnostics()
    host = eng.chain_diagnostics(rec["draws"])
    assert res["rhat"].shape == (20,) and np.all(np.isfinite(res["rhat"])) and np.all(res["ess_bulk"] > 0)
    _same_bits(res, host)
    with_lp = eng.chain_diagnostics(with_lp=True)
    lp = eng.chain_diagnostics(rec["logp"].T[None, :, :])
    for k in R.KEYS:
        assert with_lp[k].shape == (21,) and np.array_equal(with_lp[k][:20], res[k]) and with_lp[k][20] == lp[k][0], k
    _same_bits(eng.chain_diagnostics(with_lp=True), with_lp)              # a second call: equal bits
    _is_reference(res, rec["draws"])                                      # ... and they are the reference's numbers


def test_diagnostics_leave_the_chains_resumable(eng, hmc_run):
    """T = 40 + diagnostics + PFMI_HMC_CONTINUE 10 == T = 50 in one call"""
    whole = _run(eng, hmc_run, HMC_T + 10)
    a = _run(eng, hmc_run, HMC_T)
    eng.chain_diagnostics(with_lp=True)
    again = eng.hmc_get()
    for q in ("draws", "logp", "accept_prob", "energy_error", "divergent"):
        assert np.array_equal(again[q], a[q]), q                          # the records are untouched
    b = _run(eng, hmc_run, 10, cont=True)
    assert np.array_equal(np.concatenate([a["draws"], b["draws"]], axis=1), whole["draws"])
    for q in ("logp", "accept_prob", "energy_error", "divergent"):
        assert np.array_equal(np.concatenate([a[q], b[q]], axis=1), whole[q]), q


def test_public_calls(pfmi_mod):
    import torch
    tg = pfmi_mod.t_diag(10, 1)
    m, a = torch.tensor(tg.mean, device="cuda"), torch.tensor(tg.a, device="cuda")
    tgt = pfmi_mod.TorchDeviceTarget(10, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), host=tg, grad="autograd")
    e, bare = pfmi_mod.Engine(0), pfmi_mod.Engine(0)
    try:
        res = pfmi_mod.multipathfinder(tgt, 6, nruns=3, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        first = pfmi_mod.hmc(res, 40, step_size=0.2, nleapfrog=4, rng=pfmi_mod.HostRNG(8))
        assert first.run == e.hmc_runs > 0 and first.accept_prob.mean() > 0.5      # chains that move (stuck ones are constant: NaN)
        s = first.summary()
        assert isinstance(s, pfmi_mod.ChainSummary) and (s.nchains, s.ndraws) == (6, 40)
        for k in R.KEYS:
            assert getattr(s, k).shape == (10,) and np.all(np.isfinite(getattr(s, k))) and np.isfinite(s.lp[k]), k
        assert set(s.lp) == set(R.KEYS) and isinstance(s.lp["rhat"], float)
        assert "rhat" in str(s) and "chains: 6" in str(s)
        assert isinstance(s.ok(), bool) and s.ok(rhat=np.inf, ess_per_chain=0) and not s.ok(rhat=0.5)
        _is_reference(s, first.draws)
        second = pfmi_mod.hmc(res, 12, nchains=2, step_size=0.2)          # the engine's latest run is now another one
        assert second.run == e.hmc_runs > first.run
        before = e.kernel_time("chain_diag:count:one")[1]
        s2 = first.summary()                                              # ... so this one uploads the result's own copy: two calls
        assert e.kernel_time("chain_diag:count:one")[1] == before + 2
        for k in R.KEYS:
            assert np.array_equal(getattr(s2, k), getattr(s, k)) and s2.lp[k] == s.lp[k], k
        assert second.summary().rhat.shape == (10,)
        out = pfmi_mod.chain_diagnostics(first.draws, engine=bare)        # an engine without target or fit
        for k in R.KEYS:
            assert np.array_equal(out[k], getattr(s, k)), k
    finally:
        e.close()
        bare.close()


def test_return_codes(pfmi_mod):
    """every return code of pfmi_chain_diagnostics through the C ABI; the ctx stays usable afterwards"""
    from pfmi import _lib
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    d, T, K = 12, 8, 2
    tg = pfmi_mod.t_diag(d, seed=3)
    x = np.asfortranarray(np.random.default_rng(2).standard_normal((d, T, K)))
    outs = [np.empty(d + 1) for _ in range(7)]

    def call(e, source=1, draws=x, dd=d, TT=T, KK=K, flags=0, out=True):
        ptrs = [o.ctypes.data_as(dp) if out else None for o in outs]
        return L.pfmi_chain_diagnostics(e.ctx, source, None if draws is None else draws.ctypes.data_as(dp), dd, TT, KK, flags, *ptrs)

    e = pfmi_mod.Engine(0)
    try:
        assert call(e) == 0 and np.all(np.isfinite(outs[6][:d]))
        assert call(e, out=False) == 0                                        # every output NULL
        assert call(e, TT=7) == -1 and b"T >= 8" in L.pfmi_last_error()   # PFMI_ERR_ARG
        for bad in (dict(KK=0), dict(dd=0), dict(flags=2), dict(flags=4), dict(flags=1), dict(source=2), dict(source=-1), dict(draws=None)):
            assert call(e, **bad) == -1, bad
        assert call(e, source=0, draws=None, dd=0, TT=0, KK=0) == -3            # PFMI_ERR_STATE: no run on this ctx
        assert call(e, source=0, draws=None, dd=0, TT=0, KK=0, flags=1) == -3
        # a resident run
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        start = np.asfortranarray(np.repeat(tg.mean[:, None], K, axis=1))
        e.hmc_enqueue([0, 0], start, np.array([1, 2], dtype=np.uint64), 0.1, 2, T)
        e.hmc_wait()
        assert call(e, source=0, draws=None, dd=0, TT=0, KK=0, flags=1) == 0 and np.all(np.isfinite(outs[0]))
        assert call(e, source=0, draws=None) == 0                               # the run's own d, T, K
        assert call(e, source=0) == -1                                          # SRC_HMC with host draws
        for bad in (dict(dd=d + 1), dict(TT=T + 1), dict(KK=K + 1), dict(dd=0), dict(TT=0, KK=0)):
            assert call(e, source=0, draws=None, **bad) == -1, bad
        assert call(e, source=0, draws=None, flags=2) == -1
        e.hmc_enqueue([0, 0], start, np.array([1, 2], dtype=np.uint64), 0.1, 2, 7)   # a run too short to split
        e.hmc_wait()
        assert call(e, source=0, draws=None, dd=0, TT=0, KK=0) == -1
        e.fit_batch(6)                                                          # a new fit forgets the chains
        assert call(e, source=0, draws=None, dd=0, TT=0, KK=0) == -3
        assert call(e) == 0                                                     # the ctx is usable afterwards
        got = e.chain_diagnostics(x)
        assert np.array_equal(got["rhat"], outs[6][:d])
    finally:
        e.close()
