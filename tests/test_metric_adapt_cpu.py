"""The windowed metric adaptation on the CPU: the host builds of the device's sources (pfmi_adapt_windows, pfmi_host_metric_update: csrc/adapt.h)
against the Python restatement and the long-double reference of tests/metric_adapt_reference.py; the float64 mirror (bit-equal to
adapt_reference.mirror without windows, admitted on the sampling case the GPU test uses); and the checkers against five injected faults.
CPU only."""
import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import adapt_reference as A                                    # noqa: E402
import hmc_reference as H                                      # noqa: E402
import metric_adapt_reference as MA                            # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import pfmi
    return pfmi.lib()


# ---- 1. the window rule
def test_windows_match_the_restatement_and_the_table(lib):
    shortest, most = 10 ** 9, 0
    for W in range(1, 1201):
        rc, init, term, ends = MA.host_windows(lib, W)
        assert rc == 0 and (init, term, ends) == MA.windows(W), W
        if W < 20:
            assert ends == [] and init == W and term == 0
            continue
        assert term >= 2 and ends[-1] == W - term and all(b > a for a, b in zip([init] + ends[:-1], ends)), (W, init, term, ends)
        sizes = np.diff([init] + ends)
        shortest, most = min(shortest, int(sizes.min())), max(most, len(ends))
    assert shortest == 15 and most <= 7, (shortest, most)
    for W, ends in MA.TABLE.items():
        assert MA.host_windows(lib, W)[3] == ends and MA.windows(W)[2] == ends, W
    import pfmi.core
    assert pfmi.core.adapt_windows(300)[0] == 75 and pfmi.core.adapt_windows(300)[2].tolist() == [100, 150, 250]


def test_windows_argument_errors(lib):
    assert MA.host_windows(lib, 0)[0] == -1 and MA.host_windows(lib, -5)[0] == -1              # PFMI_ERR_ARG
    assert MA.host_windows(lib, 300, cap=2)[0] == -1 and MA.host_windows(lib, 300, cap=3)[0] == 0
    assert MA.host_windows(lib, 12, cap=0)[0] == 0
    assert lib.pfmi_adapt_windows(100, None, None, None, 8, None) == -1


# ---- 2. the metric update
def _columns(n, d=7):
    rng = np.random.default_rng(100 + n)
    u = rng.standard_normal((n, d)) * np.exp(rng.standard_normal(d))
    u[:, 1] = 0.75                                             # constant: D = 5 / (n + 5)
    u[:, 2] = 1e8 + rng.standard_normal(n)                     # Welford must not cancel
    u[:, 3] += 50.0
    return u


@pytest.mark.parametrize("n", (15, 500))
def test_host_metric_update_matches_the_long_double_reference(lib, n):
    u = _columns(n)
    cin = np.full(u.shape[1], 0.5)
    c, status = MA.host_metric_update(lib, u, cin)
    assert status == 0 and np.all(c > 0)
    r = MA.scale_ratio(u, c)
    print("METRIC_PARITY host update n", n, "largest ratio", r, "floor, relative", np.asarray(MA.scale_floor(u) / MA.scale_ld(u)[0], dtype=np.float64))
    assert r <= 1.0, r
    assert abs(c[1] - np.sqrt(5.0 / (n + 5.0))) <= float(MA.scale_floor(u)[1]) + 2 * MA.U
    # the sum-of-squares formula on the 1e8 column misses the bound by orders of magnitude: the bound is not vacuous
    x = u[:, 2]
    naive = np.sqrt(n / (n + 5.0) * (np.sum(x * x) - n * np.mean(x) ** 2) / (n - 1.0) + 5.0 / (n + 5.0))
    cn = c.copy()
    cn[2] = naive
    assert not MA.scale_ratio(u, cn) <= 100.0


def test_host_metric_update_keeps_the_scale_on_a_nan(lib):
    u = _columns(15)
    u[4, 5] = np.nan
    cin = np.linspace(0.5, 2.0, u.shape[1])
    c, status = MA.host_metric_update(lib, u, cin)
    assert status == MA.KEPT_METRIC and np.array_equal(c, cin)
    u[4, 5] = np.inf
    c, status = MA.host_metric_update(lib, u, cin)
    assert status == MA.KEPT_METRIC and np.array_equal(c, cin)
    assert MA.host_metric_update(lib, u[:1], cin, rc=True) == -1                                # n < 2


def test_whiten_reference_inverts_the_metric():
    """whiten_ld is L^-1: on a synthetic factor L(whiten(dx)) gives dx back, and the float64 statement is inside its own bound"""
    rng = np.random.default_rng(4)
    for d, j in ((5, 2), (64, 6), (40, 16)):
        M = H.random_metric(d, j, rng)
        dx = rng.standard_normal(d)
        u = MA.whiten_ld(M, dx)
        assert np.max(np.abs(M.astype(H.LD).L(u) - dx)) < 1e-15 * np.max(np.abs(dx)) * 100
        assert MA.whiten_ratio(M, dx, MA.whiten_np(M, dx), H.kpad_for(j)) <= 1.0
        wrong = MA.whiten_np(M, dx)
        wrong[0] *= 1 + 1e-9
        assert MA.whiten_ratio(M, dx, wrong, H.kpad_for(j)) > 1.0


# ---- 3. the mirror
def _gauss_case(d=12, j=3):
    import pfmi
    tg = pfmi.t_lowrank(d, r=2, seed=2, wscale=2.0 / np.sqrt(d))
    M = H.random_metric(d, j, np.random.default_rng(9))
    x0 = tg.mean + 0.5 * np.random.default_rng(10).standard_normal(d)
    return tg, M, x0


def test_mirror_without_windows_is_the_step_size_mirror():
    tg, M, x0 = _gauss_case()
    a = A.mirror(M, tg.logp_and_grad, x0, 77, 0.2, 3, 12, 4)
    b = MA.mirror(M, tg.logp_and_grad, x0, 77, 0.2, 3, 12, 4)
    for q in a:
        if q != "status":
            assert np.array_equal(a[q], b[q]), q
    assert b["status"] == a["status"] | MA.NO_METRIC_WINDOW and len(b["window_ends"]) == 0 and np.all(b["scale"] == 1.0)


def test_checker_admits_the_mirror_and_rejects_every_fault():
    tg, M, x0 = _gauss_case()
    W, kpad = 200, H.kpad_for(3)
    good = MA.mirror(M, tg.logp_and_grad, x0, 77, 0.2, 3, W, 2)
    assert good["window_ends"].tolist() == [100, 150] and good["status"] == 0 and not np.allclose(good["scale_trace"][0], 1.0, atol=0.02)
    marg = MA.check_run(M, kpad, x0, W, 0.8, good)
    print("METRIC_PARITY mirror margins", marg)
    for fault in MA.FAULTS:
        bad = MA.mirror(M, tg.logp_and_grad, x0, 77, 0.2, 3, W, 2, fault=fault)
        with pytest.raises(MA.Mismatch):
            MA.check_run(M, kpad, x0, W, 0.8, bad)
    # the scale on the output side of the operators: the trajectory checker on the scaled metric
    c = good["scale"]
    S = MA.ScaledMetric(M, c)
    rec = H.mirror(S, tg.logp_and_grad, x0, 5, 0.2, 3, 4)
    assert H.check(S, rec, 5, 0.2, 3, kpad)["margins"]["X"] <= 1.0
    with pytest.raises(H.Mismatch):
        H.check(S, H.mirror(MA.ScaledMetric(M, c, fault="output_side"), tg.logp_and_grad, x0, 5, 0.2, 3, 4), 5, 0.2, 3, kpad)


def test_metric_mirror_samples_the_target():
    """hmc_reference.sampling_case with adapt_reference.SAMPLING_W warm-up transitions and metric windows, from the step size d^(-1/4) of
    pfmi.hmc(step_size="auto") -- the case of tests/test_gpu_metric_adapt.py: the final states pass sampling_ok, no sampling transition
    is divergent, every scale is positive"""
    import pfmi
    tg, M, x0, seeds, Lc = H.sampling_case(pfmi)
    fin, div, eps, scales = [], 0, [], []
    for s in seeds:
        r = MA.mirror(M, tg.logp_and_grad, x0, int(s), tg.d ** -0.25, H.SAMPLING_LF, A.SAMPLING_W, A.SAMPLING_T)
        fin.append(r["draws"][-1]); div += int(r["divergent"].sum()); eps.append(r["step_size"]); scales.append(r["scale"])
        assert r["status"] == 0 and r["window_ends"].tolist() == [100]
    mean, var = H.sampling_stats(tg, Lc, np.stack(fin, axis=1))
    scales = np.array(scales)
    print("METRIC_SAMPLING mirror", np.max(np.abs(mean)), np.min(var), np.max(var), "eps", np.min(eps), np.max(eps), "scale", scales.min(), scales.max())
    assert div == 0 and np.all(np.isfinite(scales)) and np.all(scales > 0)
    assert H.sampling_ok(mean, var), (mean, var)
