"""Per-run Pareto diagnostics of the pool (pfmi_pool_psis_runs, csrc/psis_kernels.hip: pf_psis_runs_kernel, one workgroup per run).

The reference of every bit-for-bit check is pfmi_psis on the run's slice through the one-workgroup route (PFMI_PSIS_KERNEL=single, a
second Engine): both call one device function, so pareto_k, tail_len, log_weights and weights must be EQUAL.  The two outputs pfmi_psis
does not hand out have checks of their own (pool_psis_runs_reference.py): lse is the constant that was subtracted, sumsq is within
N_r 2^-52 of np.sum(w^2).  Against the CPU oracle the contract margins of SURVEY 8(d) apply unchanged (tests/margins.py); the oracle is
admitted on these very pools by tests/test_pool_psis_runs_cpu.py."""
import numpy as np
import pytest

from oracle import pf_oracle as po
import margins as mg
import pool_psis_runs_reference as rr
import psis_reference as pr
from pool_common import J, _pool, _traces, run_two_engines

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng2(pfmi_mod):
    """the second engine: the one-workgroup pfmi_psis of the references"""
    e = pfmi_mod.Engine(0)
    yield e
    e.close()


def _single(eng2, monkeypatch, lr):
    monkeypatch.setenv("PFMI_PSIS_KERNEL", "single")
    try:
        return eng2.psis(np.ascontiguousarray(lr))
    finally:
        monkeypatch.delenv("PFMI_PSIS_KERNEL", raising=False)


def _bits(a, b, what=None):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64), err_msg=str(what))


def _pool_k(pfmi, eng, name, K, N_r):
    """pool_common._pool for any K: run k is trace k % 3 drawn with seed 1000 + 7 k (K <= 3: the same pool); returns the log ratios"""
    if K <= 3:
        return _pool(pfmi, eng, name, K, N_r)[1]
    tg, traces = _traces(pfmi, name)
    trs = [traces[k % 3] for k in range(K)]
    eng.set_target(tg)
    eng.set_traces([t.points for t in trs], [t.gradients for t in trs])
    eng.fit_batch(J)
    eng.pool_build(N_r, [int(eng.offsets[k + 1]) - 1 for k in range(K)], np.array([1000 + 7 * k for k in range(K)], dtype=np.uint64))
    return eng.pool_get(draws=False)[1]


def _install(eng, lr):
    """overwrite the resident pool's log ratios"""
    ptr, cnt = eng.pool_log_ratios_dev()
    assert cnt == len(lr)
    eng.memcpy_h2d(ptr, np.ascontiguousarray(lr, dtype=np.float64))


def _compare_with_single_route(eng, eng2, monkeypatch, lr, K, N_r, tag, source="component"):
    """pool_psis_runs of the resident pool against pfmi_psis (one workgroup) on each run's slice; returns the call's dict"""
    out = eng.pool_psis_runs(source, want_weights=True)
    again = eng.pool_psis_runs(source, want_weights=True)
    for name in ("pareto_shape", "lse", "sumsq", "log_weights", "weights"):
        _bits(out[name], again[name], (tag, "second call", name))
    np.testing.assert_array_equal(out["tail_length"], again["tail_length"])
    assert out["log_weights"].shape == out["weights"].shape == (K, N_r)
    bare = eng.pool_psis_runs(source)
    assert bare["log_weights"] is None and bare["weights"] is None
    _bits(bare["pareto_shape"], out["pareto_shape"], (tag, "without weights"))
    _bits(bare["sumsq"], out["sumsq"], (tag, "without weights"))
    for k in range(K):
        s = np.ascontiguousarray(lr[k * N_r:(k + 1) * N_r])
        ref = _single(eng2, monkeypatch, s)
        cfg = (tag, "run", k)
        _bits(out["pareto_shape"][k], ref["pareto_shape"], cfg)
        assert out["tail_length"][k] == ref["tail_length"] == pr.tail_length(N_r), cfg
        _bits(out["log_weights"][k], ref["log_weights"], cfg)
        _bits(out["weights"][k], ref["weights"], cfg)
        bad = rr.lse_is_the_constant(s, out["log_weights"][k], out["lse"][k], out["pareto_shape"][k])
        assert len(bad) == 0, (cfg, "fl(lr - lse) != log_weights at", bad[:5], out["lse"][k])
        want = np.sum(ref["weights"] ** 2)
        if np.isnan(ref["weights"]).any():
            assert np.isnan(out["sumsq"][k]), cfg
        else:
            rel = abs(out["sumsq"][k] - want) / want
            print(f"{tag} run {k}: k {out['pareto_shape'][k]:.4f} sumsq rel {rel:.3g} (bound {rr.sumsq_rel_bound(N_r):.3g})")
            assert rel <= rr.sumsq_rel_bound(N_r), (cfg, out["sumsq"][k], want)
    return out


# ---- 1. the bits of the one-workgroup PSIS -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_r", [1, 4, 20, 21, 37, 1000, 1025, 8192])
@pytest.mark.parametrize("K", [1, 3, 5])
def test_bits_of_the_one_workgroup_psis_on_every_run(pfmi_mod, eng, eng2, monkeypatch, K, N_r):
    """N_r = 20: M = 4, no smoothing; 21: M = 5, the first fit; 1025: one past the thread count; 8192: where pfmi_psis on its own would
    take the multi-workgroup route"""
    lr = _pool_k(pfmi_mod, eng, "lr10", K, N_r)
    assert np.all(np.isfinite(lr))
    out = _compare_with_single_route(eng, eng2, monkeypatch, lr, K, N_r, f"psis_runs lr10 K{K} N{N_r}")
    assert np.all(np.isnan(out["pareto_shape"])) == (N_r <= 20)
    _bits(eng.pool_get(draws=False)[1], lr, "the pool's ratios changed")


# ---- 2. prescribed vectors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", range(len(rr.PRESCRIBED_POOLS)))
@pytest.mark.parametrize("N_r", [37, 1000])
def test_prescribed_vectors(pfmi_mod, eng, eng2, monkeypatch, N_r, pool):
    names = rr.PRESCRIBED_POOLS[pool]
    vec = rr.prescribed(N_r)
    lr = np.concatenate([vec[n] for n in names])
    _pool(pfmi_mod, eng, "lr10", 3, N_r)
    _install(eng, lr)
    out = _compare_with_single_route(eng, eng2, monkeypatch, lr, 3, N_r, f"psis_runs prescribed N{N_r} {'+'.join(names)}")
    for k, n in enumerate(names):
        lw, w, kk = out["log_weights"][k], out["weights"][k], out["pareto_shape"][k]
        if n in ("nan_in_tail", "nan_outside_tail", "all_neginf"):
            assert np.all(np.isnan(lw)) and np.all(np.isnan(w)) and np.isnan(kk) and np.isnan(out["sumsq"][k]), n
        elif n == "one_posinf":
            assert np.isnan(kk) and np.sum(np.isnan(w)) == 1 and np.all(w[~np.isnan(w)] == 0.0) and np.isnan(out["sumsq"][k]), n
        elif n in ("all_equal", "constant_tail"):
            assert np.isnan(kk) and abs(w.sum() - 1.0) <= 1e-12, n
            if n == "all_equal":
                assert np.all(w == w[0]), n
        else:
            assert np.isfinite(kk) and abs(w.sum() - 1.0) <= 1e-12, n


# ---- 3. independence of K and of the run's position -------------------------------------------------------------------------------------------
def test_a_run_alone_or_in_the_middle_of_three(pfmi_mod, eng):
    """funnel12, N_r = 37: run 1 pooled alone (K = 1) and as the middle of three has the same ratios, hence the same bits everywhere"""
    N_r = 37
    lr1 = _pool(pfmi_mod, eng, "funnel12", 1, N_r, runs=[1])[1]
    one = eng.pool_psis_runs(want_weights=True)
    lr3 = _pool(pfmi_mod, eng, "funnel12", 3, N_r)[1]
    _bits(lr3[N_r:2 * N_r], lr1, "the run's ratios")
    three = eng.pool_psis_runs(want_weights=True)
    assert np.isfinite(one["pareto_shape"][0])
    for name in ("pareto_shape", "lse", "sumsq", "log_weights", "weights"):
        _bits(three[name][1], one[name][0], name)
    assert three["tail_length"][1] == one["tail_length"][0] == pr.tail_length(N_r)
    # the same run as the LAST of five, behind installed special values in the other four
    _pool_k(pfmi_mod, eng, "funnel12", 5, N_r)
    vec = rr.prescribed(N_r)
    lr5 = np.concatenate([vec["all_neginf"], vec["nan_in_tail"], vec["one_posinf"], vec["light"], lr1])
    _install(eng, lr5)
    five = eng.pool_psis_runs(want_weights=True)
    for name in ("pareto_shape", "lse", "sumsq", "log_weights", "weights"):
        _bits(five[name][4], one[name][0], ("last of five", name))


# ---- 4. the pooled result is untouched --------------------------------------------------------------------------------------------------------
def test_the_pooled_psis_result_is_untouched(pfmi_mod, eng):
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, "funnel12", K, N_r)
    S = K * N_r
    pooled = eng.psis(lr)
    w0, lw0 = eng.psis_weights(S)
    _bits(w0, pooled["weights"])
    mom0 = eng.pool_moments(0, True)
    idx0 = eng.resample_indices(S, 50, seed=3)
    eng.pool_mixture_ratios(want=False)
    for source in ("component", "mixture"):
        out = eng.pool_psis_runs(source, want_weights=True)
        assert not np.array_equal(out["weights"].ravel(), w0)               # (every run normalised on its own: other numbers)
        w1, lw1 = eng.psis_weights(S)
        _bits(w1, w0, source)
        _bits(lw1, lw0, source)
        for a, b in zip(eng.pool_moments(0, True), mom0):
            _bits(a, b, (source, "pool_moments"))
        np.testing.assert_array_equal(eng.resample_indices(S, 50, seed=3), idx0)
    _bits(eng.pool_get(draws=False)[1], lr, "the pool's ratios changed")


# ---- 5. oracle parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_r", [37, 1000])
@pytest.mark.parametrize("name", ["lr10", "funnel12"])
def test_every_run_against_the_cpu_oracle(pfmi_mod, eng, name, N_r):
    K = 3
    lr = _pool(pfmi_mod, eng, name, K, N_r)[1]
    out = eng.pool_psis_runs(want_weights=True)
    for k in range(K):
        cfg = f"psis_runs {name} N{N_r} run{k}"
        lw_o, w_o, k_o, M = po.psis(np.ascontiguousarray(lr[k * N_r:(k + 1) * N_r]))
        assert out["tail_length"][k] == M
        assert np.isnan(out["pareto_shape"][k]) == np.isnan(k_o), (cfg, out["pareto_shape"][k], k_o)
        fin = np.isfinite(lw_o)
        np.testing.assert_array_equal(np.isfinite(out["log_weights"][k]), fin, err_msg=cfg)
        dev_lw = np.max(np.abs(out["log_weights"][k][fin] - lw_o[fin]) / (1 + np.abs(lw_o[fin])))
        dev_k = abs(out["pareto_shape"][k] - k_o) if np.isfinite(k_o) else 0.0
        print(f"{cfg}: psis_logw {dev_lw:.3g} pareto_k {dev_k:.3g} (k {k_o:.4f})")
        mg.check(cfg, "psis_logw", dev_lw)
        mg.check(cfg, "pareto_k", dev_k)


# ---- 6. the mixture source ------------------------------------------------------------------------------------------------------------------------
def test_mixture_source(pfmi_mod, eng, eng2, monkeypatch):
    N_r, K = 37, 3
    lr = _pool(pfmi_mod, eng, "lr10", K, N_r)[1]
    with pytest.raises(pfmi_mod.PfmiError) as ex:                            # no pfmi_pool_mixture_ratios on this pool yet
        eng.pool_psis_runs("mixture")
    assert ex.value.code == -3
    _, lrm = eng.pool_mixture_ratios()
    assert not np.array_equal(lrm, lr)
    _compare_with_single_route(eng, eng2, monkeypatch, lrm, K, N_r, "psis_runs lr10 mixture", source="mixture")
    _compare_with_single_route(eng, eng2, monkeypatch, lr, K, N_r, "psis_runs lr10 component after mixture")
    _pool(pfmi_mod, eng, "lr10", K, N_r)                                     # a new pool: the mixture ratios are gone
    with pytest.raises(pfmi_mod.PfmiError) as ex:
        eng.pool_psis_runs("mixture")
    assert ex.value.code == -3


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------------------------
def test_error_codes(pfmi_mod):
    e = pfmi_mod.Engine(0)
    try:
        tg, traces = _traces(pfmi_mod, "lr10")
        e.set_target(tg)
        e.set_traces([t.points for t in traces[:2]], [t.gradients for t in traces[:2]])
        e.fit_batch(J)
        with pytest.raises(pfmi_mod.PfmiError) as ex:                        # no pool
            e.pool_psis_runs()
        assert ex.value.code == -3
        pts = [int(e.offsets[k + 1]) - 1 for k in range(2)]
        e.pool_build(5, pts, np.array([1, 2], dtype=np.uint64))
        for source in (2, -1):
            with pytest.raises(pfmi_mod.PfmiError) as ex:
                e.pool_psis_runs(source)
            assert ex.value.code == -1
        assert pfmi_mod.lib().pfmi_pool_psis_runs(e.ctx, 0, None, None, None, None, None, None) == 0     # every output NULL
        out = e.pool_psis_runs()
        assert np.all(np.isnan(out["pareto_shape"])) and np.all(out["tail_length"] == 1)
    finally:
        e.close()


# ---- 8. the public route ----------------------------------------------------------------------------------------------------------------------------
def _public(pfmi, **kw):
    return pfmi.multipathfinder(pfmi.t_lowrank(10, r=3, seed=3), 100, nruns=4, ndraws_elbo=50, **kw)


def test_public_route(pfmi_mod, eng, eng2, monkeypatch):
    pfmi = pfmi_mod
    res = _public(pfmi, engine=eng)
    before = (res.psis_result.weights.copy(), res.psis_result.log_weights.copy(), res.psis_result.pareto_shape)
    summ0 = res.summary()
    rd = res.run_diagnostics()
    assert isinstance(rd, pfmi.RunDiagnostics) and rd.ndraws_per_run == 50
    for f in ("pareto_shape", "tail_length", "ess", "log_evidence", "elbo", "success"):
        assert getattr(rd, f).shape == (4,), f
    runs = res.pathfinder_results
    refs = []
    for r in runs:
        _, lp, lq = eng.draws(r.fit_distribution.point, r.draw_seed, 50)
        refs.append(_single(eng2, monkeypatch, lp - lq))
    k_ref = np.array([r["pareto_shape"] for r in refs])
    _bits(rd.pareto_shape, k_ref, "k-hat of the runs' stored draws")
    np.testing.assert_array_equal(rd.tail_length, [r["tail_length"] for r in refs])
    # ess = 1 / sumsq: the sum within N_r 2^-52 of np.sum (any order), plus the roundings of the two reciprocals
    sumsq_ref = np.array([np.sum(r["weights"] ** 2) for r in refs])
    assert np.all(np.abs(1.0 / rd.ess - sumsq_ref) <= 2 * rr.sumsq_rel_bound(50) * sumsq_ref)
    # log_evidence = lse - log N_r with lse the constant the route subtracted: at an entry PSIS left alone log_weights_i = fl(lr_i - lse), so
    # lr_i - log_weights_i - log N_r is log_evidence up to the roundings of these four operations
    for k, r in enumerate(runs):
        _, lp, lq = eng.draws(r.fit_distribution.point, r.draw_seed, 50)
        lr, lw = lp - lq, refs[k]["log_weights"]
        keep = np.setdiff1d(np.arange(50), pr.tail_indices(lr)[0])
        lev = lr[keep] - lw[keep] - np.log(50.0)
        slack = 2.0 ** -52 * (np.abs(lw[keep]) + 2 * np.abs(lr[keep] - lw[keep]) + 2 * np.abs(lev) + np.log(50.0))
        assert np.all(np.abs(lev - rd.log_evidence[k]) <= slack), (k, lev - rd.log_evidence[k], slack)
    ok_h = rr.host_diagnostics(rd.pareto_shape, rd.log_evidence, 1.0 / rd.ess, 50)[2]
    np.testing.assert_array_equal(rd.ok(), ok_h)
    np.testing.assert_array_equal(rd.elbo, [r.elbo_estimates[r.fit_iteration - 1].value if r.fit_iteration >= 1 else np.nan for r in runs])
    np.testing.assert_array_equal(rd.success, [r.success for r in runs])
    # nothing of the pooled result moved
    _bits(res.psis_result.weights, before[0])
    _bits(res.psis_result.log_weights, before[1])
    assert res.psis_result.pareto_shape == before[2]
    summ1 = res.summary()
    for q in ("mean", "var", "mcse_mean", "run_weights"):
        _bits(getattr(summ1, q), getattr(summ0, q), q)
    assert summ1.ess == summ0.ess and summ1.pareto_shape == summ0.pareto_shape
    rd2 = pfmi.importance_run_diagnostics(res)
    _bits(rd2.pareto_shape, rd.pareto_shape)
    _bits(rd2.ess, rd.ess)
    with pytest.raises(ValueError, match="source"):
        res.run_diagnostics(source="pooled")
    # a mixture-proposal result, diagnosed under the mixture weights and under the per-run ones
    mix = _public(pfmi, engine=eng, proposal="mixture")
    rm = mix.run_diagnostics(source="mixture")
    rc = mix.run_diagnostics()
    assert rm.pareto_shape.shape == (4,) and np.all(np.isfinite(rm.pareto_shape)) and np.all(rm.ess > 1.0)
    _bits(rc.pareto_shape, rd.pareto_shape, "the runs are the same: so are their per-run diagnostics")
    assert not np.array_equal(rm.pareto_shape, rc.pareto_shape)
    mixk = mix.psis_result.pareto_shape
    assert mix.summary().pareto_shape == mixk
    # stale: the engine is refitted
    eng.fit_batch(J)
    for stale in (res, mix):
        with pytest.raises(pfmi.StaleHandleError):
            stale.run_diagnostics()


_MULTI = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/pathfinder.jl_amd")
import pfmi
tg = pfmi.t_lowrank(10, r=3, seed=3)
one = pfmi.multipathfinder(tg, 100, nruns=4, ndraws_elbo=50)
engs = [pfmi.Engine(0), pfmi.Engine(0)]
two = pfmi.multipathfinder(tg, 100, nruns=4, ndraws_elbo=50, engines=engs)
assert [id(r.fit_distribution.engine) for r in two.pathfinder_results] == [id(engs[0])] * 2 + [id(engs[1])] * 2
a, b = one.run_diagnostics(), two.run_diagnostics()
for f in ("pareto_shape", "tail_length", "ess", "log_evidence", "elbo", "success"):
    x, y = getattr(a, f), getattr(b, f)
    assert x.shape == (4,) and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (f, x, y)
assert a.ndraws_per_run == b.ndraws_per_run == 50 and np.all(np.isfinite(a.pareto_shape))
w = two.psis_result.weights.copy()
two.run_diagnostics()
assert np.array_equal(two.summary().mean, one.summary().mean)
try:
    two.run_diagnostics(source="mixture")
    raise SystemExit("source='mixture' over two engines did not raise")
except ValueError:
    pass
print("run diagnostics engines ok", a.pareto_shape)
"""


@pytest.mark.timeout(600)
def test_run_diagnostics_over_two_engines_are_bit_identical():
    """engines=[Engine(0), Engine(0)], the runs split 2 + 2 (the pooled stage through the RCCL stand-in): every field of
    run_diagnostics() has the bits of the one-engine result"""
    run_two_engines(_MULTI, "run diagnostics engines ok")
