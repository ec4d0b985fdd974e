"""The step-size update of the device-resident warm-up on the CPU: pfmi_host_dual_averaging (the host build of csrc/adapt.h, the source the
warm kernels run) against a long-double replay of the definition in include/pfmi.h and against pfmi.hmc.dual_averaging_update iterated in
NumPy; the keep-the-previous-step rule; and the float64 adaptive mirror of static HMC on the sampling case, with the W and T the GPU test
uses (tests/test_gpu_adapt.py is admitted only if the mirror passes here).  Bounds: tests/adapt_reference.py.  CPU only."""
import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import adapt_reference as A                                    # noqa: E402
import hmc_reference as H                                      # noqa: E402

EPS0 = (1e-6, 3e-3, 0.17782794100389228, 1.0, 250.0, 1e8)
_MAX = {"eps": 0.0, "eps_bar": 0.0}


@pytest.fixture(scope="module")
def lib():
    import pfmi
    return pfmi.lib()


def _sequences():
    rng = np.random.default_rng(20)
    seqs = [("zeros", np.zeros(40)), ("ones", np.ones(40)), ("alternating", np.arange(40) % 2.0)]
    for n in (1, 2, 3, 10, 200):
        seqs.append(("random%d" % n, rng.random(n)))
    seqs.append(("beta200", rng.beta(8.0, 2.0, 200)))
    return seqs


@pytest.mark.parametrize("name,acc", _sequences(), ids=[s[0] for s in _sequences()])
def test_host_update_matches_the_long_double_replay(lib, name, acc):
    for eps0 in EPS0:
        for delta in (0.8, 0.65):
            eps, bar = A.host_dual_averaging(lib, eps0, delta, acc)
            assert eps[0] == eps0 and np.all(np.isfinite(eps)) and np.all(eps > 0)
            qe, qb = A.ratios(eps, bar, eps0, delta, acc)
            _MAX["eps"], _MAX["eps_bar"] = max(_MAX["eps"], qe), max(_MAX["eps_bar"], qb)
            assert qe <= 1.0 and qb <= 1.0, (name, eps0, delta, qe, qb)
            # the NumPy statement of the window route is within its own share of the same bound
            ne, nb = A.replay_np(eps0, delta, acc)
            assert max(A.ratios(ne, nb, eps0, delta, acc)) <= 1.0
    print("ADAPT_PARITY", name, "largest ratio so far", _MAX)


def test_floor_is_small_and_the_bound_is_not_vacuous(lib):
    """the floor stays below 1e-9 on every case above, and a wrong constant (t0 = 9) misses the bound by orders of magnitude"""
    rng = np.random.default_rng(3)
    acc = rng.random(200)
    fe, fb = A.floor(0.3, 0.8, acc)
    assert fe.max() < 1e-9 and fb.max() < 1e-9, (fe.max(), fb.max())
    eps, _ = A.host_dual_averaging(lib, 0.3, 0.8, acc)
    hbar, wrong = 0.0, [0.3]
    for t, a in enumerate(acc):
        m = t + 1
        hbar = (1 - 1 / (m + 9.0)) * hbar + (0.8 - a) / (m + 9.0)
        wrong.append(float(np.exp(np.log(3.0) - np.sqrt(m) / 0.05 * hbar)))
    assert A.ratios(np.array(wrong), None, 0.3, 0.8, acc)[0] > 1e6
    assert A.ratios(eps, None, 0.3, 0.8, acc)[0] <= 1.0


def test_a_step_size_that_underflows_keeps_the_previous_one(lib):
    """accept = 0 throughout: Hbar_m = delta m / (m + 10) and le = mu - 20 sqrt(m) Hbar_m falls below log(DBL_TRUE_MIN) = -744.4 near
    m = 2200 for eps0 = 1: from there on exp(le) is 0 and the step size must stay the last positive one"""
    n = 3000
    acc = np.zeros(n)
    eps, bar = A.host_dual_averaging(lib, 1.0, 0.8, acc)
    _, _, le, _ = A.replay_ld(1.0, 0.8, acc)
    dead = np.asarray(le, dtype=np.float64) < -746.0                  # exp(le) is 0 in float64 beyond doubt
    live = np.asarray(le, dtype=np.float64) > -708.0                  # a normal number beyond doubt
    assert dead.any() and live.any()
    assert np.all(eps > 0) and np.all(np.isfinite(eps))
    first = int(np.argmax(dead))
    assert np.all(eps[1:][dead] == eps[first]) and eps[first] > 0     # eps[first] is the step after update `first`: the last one taken
    assert np.all(np.diff(eps[1:][live]) < 0)
    assert A.ratios(eps, None, 1.0, 0.8, acc, skip=~live)[0] <= 1.0
    assert np.all(bar >= 0) and np.all(np.isfinite(bar))              # eps_bar is the raw exp(leb): it may underflow, nothing is kept there


def test_argument_errors(lib):
    one = np.array([0.5])
    assert A.host_dual_averaging(lib, 0.1, 0.8, one, rc=True) == 0
    for eps0, delta in ((0.0, 0.8), (-1.0, 0.8), (np.inf, 0.8), (np.nan, 0.8), (0.1, 0.0), (0.1, 1.0), (0.1, np.nan)):
        assert A.host_dual_averaging(lib, eps0, delta, one, rc=True) == -1, (eps0, delta)     # PFMI_ERR_ARG
    eps, bar = A.host_dual_averaging(lib, 0.1, 0.8, np.zeros(0))
    assert eps.tolist() == [0.1] and len(bar) == 0


def test_adaptive_mirror_samples_the_target():
    """hmc_reference.sampling_case through the adaptive mirror with the W and T of the GPU test: the final states pass sampling_ok and no
    sampling transition is divergent.  (Warm-up transitions may be: dual averaging starts from mu = log(10 eps_0), so its first steps are
    several times eps_0 -- that is how it finds a step size that is too small -- and a divergent one counts as a_t = 0; their number is
    printed.)"""
    import pfmi
    tg, M, x0, seeds, Lc = H.sampling_case(pfmi)
    fin, div, wdiv, eps, acc = [], 0, 0, [], []
    for s in seeds:
        r = A.mirror(M, tg.logp_and_grad, x0, int(s), H.SAMPLING_EPS, H.SAMPLING_LF, A.SAMPLING_W, A.SAMPLING_T)
        fin.append(r["draws"][-1]); div += int(r["divergent"].sum()); wdiv += int(r["warm_divergent"].sum())
        eps.append(r["step_size"]); acc.append(r["accept_prob"].mean())
        assert r["status"] == 0
    mean, var = H.sampling_stats(tg, Lc, np.stack(fin, axis=1))
    print("ADAPT_SAMPLING mirror", np.max(np.abs(mean)), np.min(var), np.max(var), "eps", np.min(eps), np.max(eps), "accept", np.mean(acc),
          "divergent warm-up transitions", wdiv)
    assert div == 0
    assert H.sampling_ok(mean, var), (mean, var)
