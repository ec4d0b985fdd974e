"""Pins tests/hmc_fused_reference.py on the CPU: the long-double value and gradient of the built-in targets against their host
logp_and_grad and a central difference; hmc_reference's mirror and checker, driven by the built-in targets' host logp_and_grad, on the
grid of tests/test_gpu_hmc_fused_steps.py (synthetic factors of the fits' shapes) with ZERO borderline decisions -- so the 2 % cap of the
GPU test is met by the reference alone; the target check against two injected faults of the new gradient; and the sampling case of
tests/test_gpu_hmc_fused.py on the mirror.  CPU only."""
import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import hmc_fused_reference as F                                # noqa: E402
import hmc_reference as H                                      # noqa: E402
import margins as mg                                           # noqa: E402


@pytest.fixture(scope="module")
def pfmi_cpu():
    import pfmi
    return pfmi


def _targets(pfmi):
    return [pfmi.t_diag(37), pfmi.t_lowrank(37, r=2, seed=2, wscale=0.3), pfmi.t_lowrank(300, r=12, seed=2, wscale=0.1), pfmi.t_funnel(37),
            pfmi.t_funnel(5)]


def test_long_double_target_matches_the_host_target_and_a_central_difference(pfmi_cpu):
    for n, tg in enumerate(_targets(pfmi_cpu)):
        d = tg.d
        x = np.random.default_rng(n).standard_normal(d) * 0.7
        lp, S, g, Sg = F.target_ld(tg, x)
        hl, hg = tg.logp_and_grad(x)
        assert S >= abs(lp) and np.all(Sg >= np.abs(g))
        # the float64 host target is one more implementation of the same sums: within a few C eps S of the long-double one
        C = d + 3 * F.rpad_of(tg) + 16
        assert abs(float(lp) - hl) <= C * F.EPS * float(S), (n, float(lp), hl)
        assert np.all(np.abs(g.astype(np.float64) - hg) <= C * F.EPS * Sg.astype(np.float64)), n
        # central difference in long double: h = 2^-20, truncation O(h^2 |f'''|) -- exact for the quadratic, ~1e-12 relative for the funnel
        h = F.LD(2.0) ** -20
        for i in (0, 1, d // 2, d - 1):
            e = np.zeros(d, dtype=F.LD)
            e[i] = h
            fd = (F.target_ld(tg, np.asarray(x, dtype=F.LD) + e)[0] - F.target_ld(tg, np.asarray(x, dtype=F.LD) - e)[0]) / (2 * h)
            assert abs(float(fd - g[i])) <= 1e-9 * (1 + float(Sg[i])), (n, i, float(fd), float(g[i]))


def _grid_chains(pfmi, case):
    """the case's three chains on the mirror: factors with j_eff = 0, 0 < j_eff < J and j_eff = J"""
    d, J, tn = case
    tg = F.grid_target(pfmi, tn, d)
    rng = np.random.default_rng(7 * d + J)
    x0 = (np.zeros(d) if tn == "funnel" else tg.mean) + 0.1 * rng.standard_normal(d)
    eps, seeds = H.grid_eps(d), H.grid_seeds(d, J)
    for k, j in enumerate((0, max(1, J // 2), J)):
        M = H.random_metric(d, j, rng)
        M.s *= 0.5 if tn == "funnel" else 1.0
        yield k, tg, M, x0, int(seeds[k]), float(eps[k])


@pytest.mark.parametrize("case", F.GRID, ids=[F.case_id(c) for c in F.GRID])
def test_mirror_on_the_built_in_targets_passes_the_checker_without_borderline_decisions(pfmi_cpu, case):
    d, J, tn = case
    kpad = H.kpad_for(J)
    for k, tg, M, x0, seed, eps in _grid_chains(pfmi_cpu, case):
        rec = H.mirror(M, tg.logp_and_grad, x0, seed, eps, F.GRID_LF, F.GRID_T)
        out = H.check(M, rec, seed, eps, F.GRID_LF, kpad, label=(F.case_id(case), k))
        assert out["borderline"] == 0, (case, k)
        assert out["accepted"] + out["rejected"] == F.GRID_T
        # the mirror's evaluations are the host target's (NumPy's sums: at most d terms in a row, not the kernel's reduction map): within
        # the same form of bound with C = d + 3 RPAD + 16; the ratios against the kernel's own C are recorded
        rl, rg = F.target_ratios(tg, rec["X"], rec["lp"], rec["g"])
        mg.record("cpu:" + F.case_id(case), "hmc_fused_lp", [rl], 1.0)
        mg.record("cpu:" + F.case_id(case), "hmc_fused_grad", [rg], 1.0)
        host = F.c_target(d, F.rpad_of(tg)) / (d + 3 * F.rpad_of(tg) + 16.0)
        assert rl * host <= 1.0 and rg * host <= 1.0, (case, k, rl, rg)


def test_grid_reaches_every_padding_target_shape_and_both_factor_routes(pfmi_cpu):
    assert {H.kpad_for(J) for _, J, _ in F.GRID} == set(H.KPADS)
    plans = F.grid_plans(pfmi_cpu)
    assert {p.rsplit(":", 1)[1] for p in plans} == {"f", "g0", "g8", "g16"}
    assert "hmc_fused:12:res:f" in plans and "hmc_fused:12:stream:f" in plans and "hmc_fused:64:stream:g8" in plans
    assert H.resident(1600, 12) and not H.resident(1601, 12) and not H.resident(320, 64)
    assert (5, 20) in {(d, H.kpad_for(J)) for d, J, _ in F.GRID}
    assert F.c_target(257, 16) == 2 + 6 + 4 + 48 + 16 and F.c_target(64, 0) == 1 + 6 + 4 + 16


@pytest.mark.parametrize("fault,tn,d", [("lowrank_sign", "gauss", 64), ("lowrank_sign", "lowrank12", 257), ("funnel_g0", "funnel", 64)])
def test_target_check_rejects_an_injected_fault_in_the_gradient(pfmi_cpu, fault, tn, d):
    """a reference with the sign of the low-rank term flipped, or with g_0 of the funnel short of its e^-tau ss term, is far outside the
    bound of the host target's gradient -- and the value, which the fault leaves alone, stays inside"""
    tg = F.grid_target(pfmi_cpu, tn, d)
    rng = np.random.default_rng(5)
    X = (0.0 if tn == "funnel" else tg.mean) + 0.5 * rng.standard_normal((6, d))
    lp = np.array([tg.logp_and_grad(x)[0] for x in X])
    g = np.array([tg.logp_and_grad(x)[1] for x in X])
    rl, rg = F.target_ratios(tg, X, lp, g)
    assert rl <= 1.0 and rg <= 1.0, (rl, rg)
    bl, bg = F.target_ratios(tg, X, lp, g, fault=fault)
    assert bl <= 1.0 and bg > 1e6, (fault, bl, bg)


def test_sampling_case_on_the_mirror(pfmi_cpu):
    """d = 8, 256 chains, T = 60, Lf = 4 from 3 sd off the mean with the identity metric: the final states' whitened means and variances"""
    tg, M, x0, seeds, Lc = H.sampling_case(pfmi_cpu)
    fin = np.empty((8, H.SAMPLING_K))
    for k in range(H.SAMPLING_K):
        rec = H.mirror(M, tg.logp_and_grad, x0, int(seeds[k]), H.SAMPLING_EPS, H.SAMPLING_LF, H.SAMPLING_T)
        fin[:, k] = rec["draws"][-1]
    mean, var = H.sampling_stats(tg, Lc, fin)
    assert H.sampling_ok(mean, var), (mean, var)
