"""CPU side of the pool transform and of moment matching (pfmi_pool_transform, pfmi.moment_match): the reference of
tests/pool_transform_reference.py against itself -- correct double evaluations of every built-in logp inside the derived bound,
wrong ones far outside --, the pure step function against the restated loop, composition of steps, the scenario of the GPU loop
test on the CPU oracle, and the new names where no device is touched."""
import numpy as np
import pytest

import pool_transform_reference as R
from pfmi import moment_match, moment_match_step           # (the parent commit fails here: the names do not exist)
from pfmi._lib import ARGTYPES, SYMBOLS

needs_ld = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.SKIP_REASON)
SHAPES = (1, 3, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def pfmi_cpu():
    import pfmi
    return pfmi


def _targets(pfmi, d):
    out = {"r0": pfmi.t_diag(d, seed=3), "funnel": pfmi.t_funnel(d)}
    for r in (3, 8, 16):
        if d >= r:
            out[f"r{r}"] = pfmi.t_lowrank(d, r=r, seed=2, wscale=2 / np.sqrt(d))
    return out


def _columns(d, n=40, seed=7):
    return np.random.default_rng(seed + d).normal(size=(d, n)) * 1.5 + 0.3


def _f64(tg, X, order, wrong=None):
    return R.funnel_logp_f64(tg.d, X, order) if tg.kind == 1 else R.gauss_logp_f64(tg, X, order, wrong)


@needs_ld
@pytest.mark.parametrize("d", SHAPES)
def test_two_double_evaluations_stay_inside_the_bound(pfmi_cpu, d):
    X = _columns(d)
    for name, tg in _targets(pfmi_cpu, d).items():
        ref, bound = R.ref_logp(tg, X)
        for order in ("forward", "backward"):
            err = np.abs(_f64(tg, X, order).astype(R.LD) - ref)
            assert np.all(err <= bound), (name, d, order, float(np.max(err / bound)))


@needs_ld
@pytest.mark.parametrize("d", (3, 65, 130))
def test_wrong_evaluations_exceed_the_bound_by_a_wide_factor(pfmi_cpu, d):
    """missing offset, scale applied twice, wrong sign of the low-rank term: each at least 1e6 bounds away in the median column
    (log|det| with the wrong sign: test_wrong_sign_of_logdet_is_caught_by_the_ratios_and_by_nothing_else)"""
    X0 = _columns(d)
    scale = 1.0 + 0.25 * (np.arange(d) % 3)
    shift = 0.1 * np.arange(d) / d - 0.2
    X = R.exact_move(scale, shift, X0)
    for name, tg in _targets(pfmi_cpu, d).items():
        ref, bound = R.ref_logp(tg, X)
        wrongs = {"scale_twice": _f64(tg, scale[:, None] * X, "forward")}
        if tg.kind != 1:
            tgo = pfmi_cpu.GaussTarget(tg.mean, 1.0 / tg.a, None, offset=1.5) if tg.r == 0 else None
            if tgo is not None:                                     # (the named targets have offset 0: the diagonal one gets 1.5)
                refo, boundo = R.ref_logp(tgo, X)
                err = np.abs(R.gauss_logp_f64(tgo, X, "forward", "no_offset").astype(R.LD) - refo)
                assert np.median(err / boundo) > 1e6, (name, d, "no_offset")
            if tg.r:
                wrongs["lowrank_sign"] = _f64(tg, X, "forward", "lowrank_sign")
        for what, got in wrongs.items():
            err = np.abs(got.astype(R.LD) - ref)
            assert np.median(err / bound) > 1e6, (name, d, what, float(np.median(err / bound)))


def test_wrong_sign_of_logdet_is_caught_by_the_ratios_and_by_nothing_else(pfmi_cpu):
    """The wrong-sign variant of the reference's own ratio helper, routed through the loop on the scenario.  It fails the check the GPU
    test makes of the device -- lq' and lr' equal to moved_ratios(...) bit for bit -- in every column of every T2 trial, by
    2 |sum log scale|, 1e6 roundings and more.  And it is invisible to the loop: log|det A| is one constant for the whole pool and
    PSIS is invariant under a shift of the log ratios, so history and map agree with the correct loop's to rounding.  The bit-exact
    comparison of tests/test_gpu_pool_transform.py::test_move_and_ratios_bit_for_bit is therefore the guard against this error;
    no k-hat, weight or decision is."""
    from oracle import pf_oracle as po
    X0, lq0 = R.scenario_oracle_pool(pfmi_cpu)
    logp = R.scenario_logp(pfmi_cpu)
    good = R.mm_loop(X0, lq0, logp, po.psis, k_threshold=R.SC_K_THRESHOLD)
    bad = R.mm_loop(X0, lq0, logp, po.psis, k_threshold=R.SC_K_THRESHOLD, wrong_sign=True)
    seen = 0
    for step, _, _, sc, sh, *_ in good["trials"]:
        lp1 = logp(sc[:, None] * X0 + sh[:, None])
        lq_ok, lr_ok = R.moved_ratios(lp1, lq0, sc)
        lq_bad, lr_bad = R.moved_ratios(lp1, lq0, sc, wrong_sign=True)
        sla = R.sum_log_scale(sc)
        if sla == 0.0:                                              # a pure shift has no Jacobian to get wrong
            np.testing.assert_array_equal(lr_bad, lr_ok)
            continue
        seen += 1
        assert np.all(lq_bad != lq_ok) and np.all(lr_bad != lr_ok)
        assert np.all(np.abs(lr_bad - lr_ok) > 1e6 * R.EPS * (1 + np.abs(lr_ok))), (step, sla)
    assert seen >= 2
    assert [(s, a) for s, _, a in bad["history"]] == [(s, a) for s, _, a in good["history"]]
    assert max(abs(a[1] - b[1]) for a, b in zip(bad["history"], good["history"])) < 1e-9
    np.testing.assert_allclose(bad["scale"], good["scale"], rtol=1e-9)


def test_exact_move_is_the_single_rounding():
    """where a x + b is exactly representable exact_move returns it; where the product's rounding would show, it does not"""
    a, b = np.array([1.0 + 2.0 ** -30]), np.array([-1.0])
    x = np.array([[1.0 + 2.0 ** -30, 3.0, -7.5]])
    got = R.exact_move(a, b, x)
    assert got[0, 0] == 2.0 ** -29 + 2.0 ** -60                     # (plain double: the product rounds the 2^-60 away)
    assert (a[0] * x[0, 0] + b[0]) != got[0, 0]
    np.testing.assert_array_equal(R.exact_move(np.ones(1), np.zeros(1), x), x)
    assert R.sum_log_scale(np.ones(5)) == 0.0


def _sums(X, w):
    W = w.sum()
    s1 = X @ w
    Z = X - (s1 / W)[:, None]
    return W, s1, Z @ w, (Z * Z) @ w


def test_step_function_agrees_with_the_loop_and_composes(pfmi_cpu):
    from oracle import pf_oracle as po
    X0, lq0 = R.scenario_oracle_pool(pfmi_cpu)
    out = R.mm_loop(X0, lq0, R.scenario_logp(pfmi_cpu), po.psis, k_threshold=R.SC_K_THRESHOLD)
    # every trial of the loop from the pure function, given the moment sums of the pool the trial started from
    scale, shift, X = np.ones(R.SC_D), np.zeros(R.SC_D), X0
    _, w, _, _ = po.psis(R.scenario_logp(pfmi_cpu)(X0) - lq0)
    ones = np.ones(X0.shape[1])
    it = iter(out["history"][1:])
    for step, a, b, sc, sh, *_ in out["trials"]:
        ga, gb, gsc, gsh = moment_match_step(step, _sums(X, ones), _sums(X, w), scale, shift)
        for got, ref in ((ga, a), (gb, b), (gsc, sc), (gsh, sh)):
            np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-15)
        # composition: the step applied to the current pool is the cumulative map applied to the pool as built
        np.testing.assert_allclose(ga[:, None] * X + gb[:, None], gsc[:, None] * X0 + gsh[:, None], rtol=0, atol=1e-13)
        if next(it)[2]:
            scale, shift = sc, sh
            X = sc[:, None] * X0 + sh[:, None]
            _, w, _, _ = po.psis(R.scenario_logp(pfmi_cpu)(X) - (lq0 - R.sum_log_scale(sc)))
    np.testing.assert_array_equal(scale, out["scale"])
    # two steps in a row equal the cumulative map: (a2, b2) after (a1, b1) is (a2 a1, a2 b1 + b2)
    a1, b1 = np.array([2.0, 0.5]), np.array([1.0, -1.0])
    dummy = (1.0, np.zeros(2), np.zeros(2), np.ones(2))
    _, _, s2, h2 = moment_match_step("T2", dummy, (1.0, np.array([3.0, 4.0]), np.zeros(2), 4.0 * np.ones(2)), a1, b1)
    np.testing.assert_array_equal(s2, 2.0 * a1)                    # a = sqrt(4 / 1) = 2, b = m - 2 * 0
    np.testing.assert_array_equal(h2, 2.0 * b1 + np.array([3.0, 4.0]))
    with pytest.raises(ValueError):
        moment_match_step("T3", dummy, dummy, a1, b1)


def test_scenario_of_the_gpu_loop_on_the_oracle(pfmi_cpu):
    """starts above 0.7, ends below 0.5, and every decision is at least 1e-6 clear, so that demanding the same decisions of the
    device (whose k-hat is within 1e-8) is fair; at the default threshold the loop stops after its first accepted move"""
    from oracle import pf_oracle as po
    X0, lq0 = R.scenario_oracle_pool(pfmi_cpu)
    out = R.mm_loop(X0, lq0, R.scenario_logp(pfmi_cpu), po.psis, k_threshold=R.SC_K_THRESHOLD)
    h = out["history"]
    assert h[0][0] == "start" and h[0][1] > 0.7 and out["k"] < 0.5
    assert min(R.history_gaps(h)) > 1e-6
    steps = [(s, acc) for s, _, acc in h[1:]]
    assert ("T1", True) in steps and ("T2", True) in steps and ("T1", False) in steps and steps[-2:] == [("T1", False), ("T2", False)]
    ks = [k for _, k, acc in h if acc]
    assert all(b < a for a, b in zip(ks, ks[1:]))
    dflt = R.mm_loop(X0, lq0, R.scenario_logp(pfmi_cpu), po.psis)
    assert [s for s, _, _ in dflt["history"]] == ["start", "T1"] and dflt["k"] <= 0.7


def test_names_and_arguments_without_a_device(pfmi_cpu):
    assert "pfmi_pool_transform" in SYMBOLS and "pfmi_pool_transform_revert" in SYMBOLS
    assert len(ARGTYPES["pfmi_pool_transform"]) == 5 and len(ARGTYPES["pfmi_pool_transform_revert"]) == 1
    assert hasattr(pfmi_cpu.Engine, "pool_transform") and hasattr(pfmi_cpu.Engine, "pool_transform_revert")
    res = pfmi_cpu.MultiPathfinderResult(None, None, None, [], None, None, [], None)
    assert res.pool_transform is None and res.moment_match_history is None
    with pytest.raises(ValueError):                                 # no importance weights, decided before any device is touched
        moment_match(res)
    assert res.moment_match.__func__ is pfmi_cpu.MultiPathfinderResult.moment_match
