"""Pins tests/nuts_reference.py on the CPU: the iterative (checkpoint) tree builder against the textbook recursive one, the float64 mirror
against the long-double checker on the grid of tests/test_gpu_nuts_steps.py (synthetic factors of the fits' shapes: no GPU fit exists
here) without a borderline decision, the checker against six injected faults, and the mirror as a sampler.  CPU only."""
import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import hmc_reference as H                                      # noqa: E402
import margins as mg                                           # noqa: E402
import nuts_reference as N                                     # noqa: E402

FAULTS = ("ck_index", "skip_check", "uniform_top", "flip_dir", "weight_sign", "stale_rho")


@pytest.fixture(scope="module")
def pfmi_cpu():
    import pfmi
    return pfmi


class _Gauss:
    """logp = -sum(a x^2) / 2"""

    def __init__(self, a):
        self.a = a

    def logp_and_grad(self, x):
        return -0.5 * float(np.sum(self.a * x * x)), -self.a * x


def test_iterative_builder_equals_the_recursive_one(pfmi_cpu):
    """depth, leaf count and stop reason of one transition, 1200 random cases (dimension, target scales, factor, start, momentum, step size,
    directions), every tree depth 1 .. 7 occurring and every stop reason"""
    rng = np.random.default_rng(2024)
    depths, stops = {}, {}
    for case in range(1200):
        d = int(rng.integers(2, 7))
        tg = _Gauss(np.exp(rng.uniform(-2, 2, d)))
        M = H.random_metric(d, int(rng.integers(0, 3)), rng)
        x = rng.standard_normal(d) * (30.0 if case % 40 == 0 else 1.0)
        eps = float(np.exp(rng.uniform(np.log(0.004), np.log(1.5)))) * (40.0 if case % 40 == 0 else 1.0)
        v0 = rng.standard_normal(d)
        dirs = [1 if b else -1 for b in rng.integers(0, 2, 8)]
        lp, g = tg.logp_and_grad(x)
        rec = N.mirror(M, tg.logp_and_grad, x, 1000 + case, eps, 7, 1, momenta=lambda t: v0, directions=lambda t, j: dirs[j])
        got = (int(rec["tree_depth"][0]), int(rec["n_leapfrog"][0]), rec["stop"][0])
        want = N.recursive(M, tg.logp_and_grad, x, lp, M.R(g), v0, eps, 7, lambda j: dirs[j])
        assert got == want, (case, got, want)
        depths[got[0]] = depths.get(got[0], 0) + 1
        stops[got[2]] = stops.get(got[2], 0) + 1
    print("NUTS_BUILDERS", depths, stops)
    assert set(depths) == set(range(1, 8)), depths
    assert set(stops) == {"divergent", "subtree_turn", "tree_turn", "max_depth"}, stops


def _grid_chains(pfmi, case):
    """the case's three chains on the mirror: factors with j_eff = 0, 0 < j_eff < J and j_eff = J (tests/test_hmc_reference_cpu.py's)"""
    d, J, tn, md, T = case
    tg = H.grid_target(pfmi, tn, d)
    rng = np.random.default_rng(7 * d + J)
    x0 = (np.zeros(d) if tn == "funnel" else tg.mean) + 0.1 * rng.standard_normal(d)
    eps, seeds = H.grid_eps(d), H.grid_seeds(d, J)
    for k, j in enumerate((0, max(1, J // 2), J)):
        M = H.random_metric(d, j, rng)
        M.s *= 0.5 if tn == "funnel" else 1.0
        yield k, tg, M, x0, int(seeds[k]), float(eps[k])


_SEEN = set()


@pytest.mark.parametrize("case", N.GRID, ids=[N.case_id(c) for c in N.GRID])
def test_mirror_passes_the_checker_without_borderline_decisions(pfmi_cpu, case):
    d, J, tn, md, T = case
    kpad = H.kpad_for(J)
    for k, tg, M, x0, seed, eps in _grid_chains(pfmi_cpu, case):
        rec = N.mirror(M, tg.logp_and_grad, x0, seed, eps, md, T)
        out = N.check(M, rec, seed, eps, md, kpad, label=(N.case_id(case), k))
        assert out["borderline"] == 0 and out["decisions"] > 0, (case, k, out)
        _SEEN.update(out["seen"])
        for q, m in out["margins"].items():
            mg.record("cpu:" + N.case_id(case), "nuts_" + q, [m], 1.0)


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_rejects_injected_fault(pfmi_cpu, fault):
    """each wrong step must be caught on a small case (d = 64, J = 6, a full factor, trees of up to 32 leaves)"""
    d, J = 64, 6
    tg = H.grid_target(pfmi_cpu, "gauss", d)
    rng = np.random.default_rng(3)
    M = H.random_metric(d, J, rng)
    x0 = tg.mean + 0.3 * rng.standard_normal(d)
    seed, eps = 12345, 0.15
    good = N.mirror(M, tg.logp_and_grad, x0, seed, eps, 6, 8)
    out = N.check(M, good, seed, eps, 6, H.kpad_for(J))
    assert out["borderline"] == 0
    bad = N.mirror(M, tg.logp_and_grad, x0, seed, eps, 6, 8, fault=fault)
    with pytest.raises(N.Mismatch):
        N.check(M, bad, seed, eps, 6, H.kpad_for(J))


def test_mirror_samples_a_gaussian(pfmi_cpu):
    """256 chains of 12 transitions on a 3-d Gaussian from 3 standard deviations off: means and variances of the final states within
    hmc_reference.sampling_ok's sampling-distribution bounds"""
    a = np.array([0.25, 1.0, 9.0])
    tg = _Gauss(a)
    M = H.identity_metric(3)
    x0 = 3.0 / np.sqrt(a)
    seeds = np.asarray(pfmi_cpu.hostrng.rand_u64(4711, np.arange(256, dtype=np.uint64), 9), dtype=np.uint64)
    recs = [N.mirror(M, tg.logp_and_grad, x0, int(s), 0.25, 6, 12) for s in seeds]
    fin = np.stack([r["draws"][-1] for r in recs], axis=1) * np.sqrt(a)[:, None]
    mean, var = fin.mean(axis=1), fin.var(axis=1, ddof=1)
    depth = np.concatenate([r["tree_depth"] for r in recs])
    print("NUTS_SAMPLING mirror", mean, var, np.bincount(depth))
    assert H.sampling_ok(mean, var, n=256), (mean, var)


def test_grid_reaches_every_instantiation():
    assert {H.kpad_for(c[1]) for c in N.GRID} == set(H.KPADS)   # all seven paddings of pf_dispatch_kpad (hm_launch_step)
    assert {(c[0], H.kpad_for(c[1])) for c in N.GRID} >= {(64, 8), (64, 16), (64, 20), (5, 20)}


def test_grid_reaches_every_kind_of_event(pfmi_cpu):
    """what the coverage test of tests/test_gpu_nuts_steps.py asks of the GPU runs occurs on the mirror's runs of the same grid"""
    for case in N.GRID[:-1]:
        if not _SEEN >= {"divergent", "subtree_turn", "tree_turn", "max_depth", "candidate_replaced", "candidate_kept", "dir+", "dir-"}:
            test_mirror_passes_the_checker_without_borderline_decisions(pfmi_cpu, case)
    print("NUTS_GRID_SEEN", sorted(_SEEN))
    assert _SEEN >= {"divergent", "subtree_turn", "tree_turn", "max_depth", "candidate_replaced", "candidate_kept", "dir+", "dir-"}, _SEEN
