"""Pins tests/hmc_reference.py on the CPU: the float64 mirror of the HMC transition against the long-double checker on the grid of
tests/test_gpu_hmc_steps.py (synthetic factors of the fits' shapes: no GPU fit exists here), the checker against six injected faults,
the dual-averaging rule against hand-computed values, and the sampling / energy-order cases of tests/test_gpu_hmc.py on the mirror
with the seeds, step sizes and (identity: a path's first point) metric the GPU tests use.  CPU only."""
import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import hmc_reference as H                                      # noqa: E402
import margins as mg                                           # noqa: E402

FAULTS = ("half_sign", "T_for_Tt", "no_sqrt_alpha", "normals_t1", "uniform_counter", "full_kick_end")


@pytest.fixture(scope="module")
def pfmi_cpu():
    import pfmi
    return pfmi


def _grid_chains(pfmi, case):
    """the case's three chains on the mirror: factors with j_eff = 0, 0 < j_eff < J and j_eff = J"""
    d, J, tn, T = case
    tg = H.grid_target(pfmi, tn, d)
    rng = np.random.default_rng(7 * d + J)
    x0 = (np.zeros(d) if tn == "funnel" else tg.mean) + 0.1 * rng.standard_normal(d)
    eps, seeds = H.grid_eps(d), H.grid_seeds(d, J)
    for k, j in enumerate((0, max(1, J // 2), J)):
        M = H.random_metric(d, j, rng)
        M.s *= 0.5 if tn == "funnel" else 1.0
        yield k, tg, M, x0, int(seeds[k]), float(eps[k]), T


@pytest.mark.parametrize("case", H.GRID, ids=[H.case_id(c) for c in H.GRID])
def test_mirror_passes_the_checker_without_borderline_decisions(pfmi_cpu, case):
    d, J, tn, T = case
    kpad = H.kpad_for(J)
    for k, tg, M, x0, seed, eps, T in _grid_chains(pfmi_cpu, case):
        rec = H.mirror(M, tg.logp_and_grad, x0, seed, eps, H.GRID_LF, T)
        out = H.check(M, rec, seed, eps, H.GRID_LF, kpad, label=(H.case_id(case), k))
        assert out["borderline"] == 0, (case, k)
        assert out["accepted"] + out["rejected"] == T
        for q, m in out["margins"].items():
            mg.record("cpu:" + H.case_id(case), "hmc_" + q, [m], 1.0)


def test_grid_reaches_every_instantiation_and_both_factor_routes():
    kp = {H.kpad_for(J) for _, J, _, _ in H.GRID}
    assert kp == set(H.KPADS)                                   # all seven paddings of pf_dispatch_kpad (hm_launch_step)
    assert {(d, H.kpad_for(J)) for d, J, _, _ in H.GRID} >= {(64, 8), (64, 16), (64, 20), (5, 20)}
    routes = {H.resident(d, H.kpad_for(J)) for d, J, _, _ in H.GRID}
    assert routes == {True, False}
    assert not H.resident(20000, 12) and H.resident(1000, 12) and not H.resident(1000, 64)


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_rejects_injected_fault(pfmi_cpu, fault):
    """each wrong step must be caught on a small case (d = 64, J = 6, a full factor; a step size at which the acceptance probabilities
    spread over (0.4, 1), so that a uniform from the wrong counter changes a decision)"""
    d, J = 64, 6
    tg = H.grid_target(pfmi_cpu, "gauss", d)
    rng = np.random.default_rng(3)
    M = H.random_metric(d, J, rng)
    x0 = tg.mean + 0.3 * rng.standard_normal(d)
    seed, eps = 12345, 0.4
    good = H.mirror(M, tg.logp_and_grad, x0, seed, eps, 3, 12)
    H.check(M, good, seed, eps, 3, H.kpad_for(J))
    bad = H.mirror(M, tg.logp_and_grad, x0, seed, eps, 3, 12, fault=fault)
    with pytest.raises(H.Mismatch):
        H.check(M, bad, seed, eps, 3, H.kpad_for(J))


def test_dual_averaging_update_three_steps_by_hand(pfmi_cpu):
    """eps_0 = 1, target 0.8, acceptances 0.5, 0.9, 0.7 (gamma = 0.05, t0 = 10, kappa = 0.75, mu = log 10):
       Hbar_1 = 0.3 / 11;                 log eps_1 = log 10 - 20 Hbar_1;            log epsbar_1 = log eps_1
       Hbar_2 = 11/12 Hbar_1 - 0.1 / 12;  log eps_2 = log 10 - 20 sqrt 2 Hbar_2;     log epsbar_2 = 2^-.75 log eps_2 + (1 - 2^-.75) log epsbar_1
       Hbar_3 = 12/13 Hbar_2 + 0.1 / 13;  log eps_3 = log 10 - 20 sqrt 3 Hbar_3;     log epsbar_3 = 3^-.75 log eps_3 + (1 - 3^-.75) log epsbar_2"""
    da = pfmi_cpu.hmc
    st = da.dual_averaging_init(1.0)
    want = [(0.3 / 11, 5.795782787848097, 5.795782787848097), (1.0 / 60, 6.24125055778261, 6.056674915231589),
            (0.3 / 13, 4.495950163783623, 5.314494971505881)]
    h1 = 0.3 / 11
    h2 = 11 / 12 * h1 - 0.1 / 12
    h3 = 12 / 13 * h2 + 0.1 / 13
    assert abs(h2 - 1 / 60) < 1e-15 and abs(h3 - 0.3 / 13) < 1e-15
    for a, (hb, e, eb) in zip((0.5, 0.9, 0.7), want):
        st, eps, ebar = da.dual_averaging_update(st, a, 0.8)
        assert abs(float(st[1]) - hb) < 1e-15 and abs(float(eps) - e) < 1e-12 and abs(float(ebar) - eb) < 1e-12
    le1 = np.log(10) - 20 * h1
    le2 = np.log(10) - 20 * np.sqrt(2) * h2
    assert abs(np.log(want[1][2]) - (2 ** -0.75 * le2 + (1 - 2 ** -0.75) * le1)) < 1e-12
    # vectorised over chains, pure (the input state is not modified)
    s0 = da.dual_averaging_init(np.array([1.0, 0.5]))
    s1, e, _ = da.dual_averaging_update(s0, np.array([0.5, 0.5]))
    assert s0[0] == 0 and np.all(s0[1] == 0) and e.shape == (2,) and abs(e[1] / e[0] - 0.5) < 1e-12


# ---- the cases of tests/test_gpu_hmc.py on the mirror -------------------------------------------------------------------------------
def test_energy_order_on_the_mirror(pfmi_cpu):
    tg, M, x0, seeds = H.energy_case(pfmi_cpu)
    mx = []
    for eps, Lf in H.ENERGY_RUNS:
        de = [H.mirror(M, tg.logp_and_grad, x0[:, k], int(seeds[k]), eps, Lf, 1)["energy_error"][0] for k in range(x0.shape[1])]
        mx.append(np.max(np.abs(de)))
    ratio = mx[0] / mx[1]
    print("HMC_ENERGY_ORDER mirror", mx, ratio)
    assert H.ENERGY_RATIO[0] <= ratio <= H.ENERGY_RATIO[1], (mx, ratio)


def _sampling_on_the_mirror(pfmi, refresh):
    tg, M, x0, seeds, Lc = H.sampling_case(pfmi)
    fin = np.stack([H.mirror(M, tg.logp_and_grad, x0, int(s), H.SAMPLING_EPS, H.SAMPLING_LF, H.SAMPLING_T, refresh=refresh)["draws"][-1]
                    for s in seeds], axis=1)
    return H.sampling_stats(tg, Lc, fin)


def test_sampling_on_the_mirror(pfmi_cpu):
    mean, var = _sampling_on_the_mirror(pfmi_cpu, True)
    print("HMC_SAMPLING mirror", np.max(np.abs(mean)), np.min(var), np.max(var))
    assert H.sampling_ok(mean, var), (mean, var)


def test_sampling_fails_without_the_momentum_refresh(pfmi_cpu):
    mean, var = _sampling_on_the_mirror(pfmi_cpu, False)
    assert not H.sampling_ok(mean, var), (mean, var)
