"""The ChEES rule on the CPU (csrc/adapt.h through its host builds pfmi_host_chees_leapfrog and pfmi_host_chees_update): the jitter and the
leapfrog rule exactly; the cross-chain update against the long-double replay of tests/chees_reference.py within its counted bound, for the
host build and for the float64 NumPy mirror (so the GPU is never held to a bound the CPU has not met); five injected faults, each rejected;
and the mirror on hmc_reference.sampling_case with the W, T and Lmax the GPU test uses.  CPU only."""
import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import chees_reference as R                                     # noqa: E402
import hmc_reference as H                                       # noqa: E402

HALTON16 = [1 / 2, 1 / 4, 3 / 4, 1 / 8, 5 / 8, 3 / 8, 7 / 8, 1 / 16, 9 / 16, 5 / 16, 13 / 16, 3 / 16, 11 / 16, 7 / 16, 15 / 16, 1 / 32]
FAULTS = ("unweighted_mean", "no_jitter", "grad_wrt_tau", "arithmetic_mean", "halton_t")


@pytest.fixture(scope="module")
def lib():
    import pfmi
    return pfmi.lib()


def test_halton_values(lib):
    assert [R.halton(t) for t in range(16)] == HALTON16
    # the host build's: n = ceil(32 h) is 32 h itself, an integer, for these t
    assert [R.host_leapfrog(lib, t, 32.0, 1.0, 1024)[0] for t in range(16)] == [int(32 * h) for h in HALTON16]
    assert R.halton(2 ** 32 - 2) == 1.0 - 2.0 ** -32 and R.halton(2 ** 31 - 1) == 2.0 ** -32


def test_leapfrog_rule(lib):
    for args, want in (((0, 4.0, 1.0, 64), (2, False)),               # h tau / eps = 2 exactly: no step more
                       ((0, np.nextafter(4.0, 5.0), 1.0, 64), (3, False)),
                       ((2, 4.0, 0.5, 64), (6, False)),               # 3/4 * 4 / 0.5 = 6 exactly
                       ((0, 0.0, 1.0, 64), (1, False)),               # n = 0 steps once
                       ((3, 1e-9, 1.0, 64), (1, False)),
                       ((0, 1000.0, 1.0, 8), (8, True)),              # the clamp and its status bit
                       ((0, 16.0, 1.0, 8), (8, False)),               # n = Lmax exactly is not clamped
                       ((0, 2049.0, 1.0, 1024), (1024, True))):
        assert R.leapfrog(*args) == want, args
        assert R.host_leapfrog(lib, *args) == want, args
    rng = np.random.default_rng(5)
    for _ in range(400):
        t, tau, eps, Lmax = int(rng.integers(0, 5000)), float(np.exp(rng.normal(0, 2))), float(np.exp(rng.normal(-1, 1))), int(rng.integers(1, 1025))
        assert R.host_leapfrog(lib, t, tau, eps, Lmax) == R.leapfrog(t, tau, eps, Lmax)
    assert lib.pfmi_host_chees_leapfrog(0, 1.0, 1.0, 0, None) == -1 and lib.pfmi_host_chees_leapfrog(0, 1.0, 1.0, 1025, None) == -1
    assert lib.pfmi_host_chees_leapfrog(-1, 1.0, 1.0, 8, None) == -1


def _inputs(K, d, W, kind, rng):
    """W updates' inputs: x, x', u' (W, K, d) and a (W, K)"""
    x = 2.0 + rng.standard_normal((W, K, d))
    xp = x + 0.7 * rng.standard_normal((W, K, d))
    u = rng.standard_normal((W, K, d))
    a = rng.random((W, K)) * 0.9 + 0.1
    if kind == "divergent_chain":                                    # a chain with a = 0 whose x' and u' are not finite, in every update
        k = K // 2
        a[:, k] = 0.0
        xp[:, k] = np.nan
        u[:, k, 0] = np.inf
    elif kind == "all_rejected":                                     # every a = 0 in update 1: KEPT_TRAJ
        a[1 % W] = 0.0
        xp[1 % W] = np.inf
    elif kind == "one_point":                                        # all chains at one point: p = 0
        x[:] = x[:, :1]
    return x, xp, u, a


@pytest.mark.parametrize("K", (1, 3, 64))
@pytest.mark.parametrize("d", (1, 5, 257))
def test_host_update_and_numpy_mirror_match_the_long_double_replay(lib, K, d):
    rng = np.random.default_rng(100 * K + d)
    eps0, tau0, delta, Lmax, W = 0.3, 0.0, R.DELTA, 64, 5
    worst = {"host": 0.0, "numpy": 0.0}
    for kind in ("plain", "divergent_chain", "all_rejected", "one_point"):
        if kind == "divergent_chain" and K == 1:
            continue
        x, xp, u, a = _inputs(K, d, W, kind, rng)
        rep = R.replay_ld(eps0, tau0, delta, Lmax, x, xp, u, a)
        hs, ns = R.host_state(eps0, tau0, delta), R.np_state(eps0, tau0, delta)
        got = {"host": ([], [], []), "numpy": ([], [], [])}
        for t in range(W):
            assert R.host_update(lib, hs, x[t], xp[t], u[t], a[t], R.halton(t), Lmax, last=t == W - 1) == 0
            g, hm = R.update_np(ns, x[t], xp[t], u[t], a[t], R.halton(t), Lmax, last=t == W - 1)
            for key, vals in (("host", (hs.grad, hs.traj_length, hs.step_size)), ("numpy", (g, ns["tau"], ns["eps"]))):
                for lst, v in zip(got[key], vals):
                    lst.append(v)
            assert abs(hs.hmean - float(rep[t]["hm"])) <= (K + 3) * R.U * float(rep[t]["hm"])
        kept = any(o["kept"] for o in rep)
        assert kept == (kind == "all_rejected")
        assert bool(hs.status & R.KEPT_TRAJ) == kept and bool(ns["status"] & R.KEPT_TRAJ) == kept
        for key in got:
            q = max(R.ratios(rep, *got[key]))
            worst[key] = max(worst[key], q)
            assert q <= 1.0, (key, kind, K, d, R.ratios(rep, *got[key]))
    print("CHEES_PARITY K", K, "d", d, "largest ratio", worst)


def _small_run(pfmi, fault=None):
    rng = np.random.default_rng(9)
    d, K, W = 5, 8, 10
    tg = H.grid_target(pfmi, "gauss", d)
    Ms = [H.random_metric(d, 2, rng) for _ in range(K)]
    x0 = tg.mean[:, None] + rng.standard_normal((d, K))
    seeds = H.grid_seeds(d, 2)[:1].repeat(K) + np.arange(K, dtype=np.uint64)
    return R.mirror(Ms, tg.logp_and_grad, x0, seeds, 0.2, 0.0, 16, W, 2, fault=fault), (0.2, 0.0, R.DELTA, 16)


def test_the_mirror_meets_the_bound_and_every_fault_misses_it():
    import pfmi
    res, par = _small_run(pfmi)
    l_ok, qg, qt, qe = R.check_run(res, *par)
    print("CHEES_MIRROR small run ratios", qg, qt, qe, "L", res["n_leapfrog"].tolist())
    assert l_ok and max(qg, qt, qe) <= 1.0
    for fault in FAULTS:
        bad, _ = _small_run(pfmi, fault)
        l_ok, qg, qt, qe = R.check_run(bad, *par)
        assert not l_ok or max(qg, qt, qe) > 1e3, (fault, l_ok, qg, qt, qe)


def test_the_mirror_samples_the_target():
    """hmc_reference.sampling_case through the mirror: K = 256, W = 150, T = 60, Lmax = 64 (the GPU test's run)"""
    import pfmi
    tg, M, x0, _, Lc = H.sampling_case(pfmi)
    seeds = R.sampling_seeds(pfmi)
    X0 = np.repeat(x0[:, None], R.SAMPLING_K, axis=1)
    res = R.mirror([M] * R.SAMPLING_K, tg.logp_and_grad, X0, seeds, tg.d ** -0.25, 0.0, R.SAMPLING_LMAX, R.SAMPLING_W, R.SAMPLING_T)
    mean, var = H.sampling_stats(tg, Lc, res["draws"][-1].T)
    n = R.SAMPLING_K
    ratio = max(np.max(np.abs(mean)) / (5.0 / np.sqrt(n)), np.max(np.abs(var - 1.0)) / (5.0 * np.sqrt(2.0 / (n - 1))))
    Ls = res["n_leapfrog"][R.SAMPLING_W:]
    print("CHEES_SAMPLING mirror seed base", R.SEED_BASE, "worst ratio", ratio, "tau", res["traj_length"], "eps", res["step_size"], "mean L", Ls.mean(),
          "accept", res["accept_prob"].mean(), "status", res["status"])
    assert res["divergent"].sum() == 0
    assert res["traj_length"] > res["step_size"] and Ls.mean() >= 2
    assert H.sampling_ok(mean, var), (mean, var)
    assert ratio <= 0.8, ratio                                   # the margin the seed base was admitted with (profiles/chees.md: 0.648)
    l_ok, qg, qt, qe = R.check_run(res, tg.d ** -0.25, 0.0, R.DELTA, R.SAMPLING_LMAX)
    print("CHEES_SAMPLING mirror against the replay", l_ok, qg, qt, qe)
    assert l_ok and max(qg, qt, qe) <= 1.0
