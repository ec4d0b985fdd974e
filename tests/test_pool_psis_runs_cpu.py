"""CPU side of the per-run Pareto diagnostics (pfmi_pool_psis_runs): the host arithmetic of RunDiagnostics on hand-made arrays, the
admission of the CPU oracle as the GPU test's reference on the very pools that test uses, and the prescribed vectors' own design."""
import numpy as np
import pytest

from oracle import pf_oracle as po
import margins as mg
import pool_psis_runs_reference as rr
import psis_reference as pr

needs_ld = pytest.mark.skipif(not pr.HAVE_LONGDOUBLE, reason=pr.SKIP_REASON)


def test_host_arithmetic_on_hand_made_arrays():
    import pfmi
    from pfmi.api import _run_diagnostics_host
    k = np.array([0.2, 0.7, np.nextafter(0.7, 1.0), np.nan, -0.1, 1.3])
    M = np.array([8, 8, 8, 8, 8, 8], dtype=np.int64)
    lse = np.array([-3.5, 0.0, 12.25, np.nan, -np.inf, 700.0])
    sumsq = np.array([1.0 / 37, 1.0, 0.125, np.nan, 0.0, 3e-4])
    elbo = [1.5, np.nan, -2.0, 0.0, 3.0, 4.0]
    ok_flags = [True, False, True, True, False, True]
    rd = _run_diagnostics_host(k, M, lse, sumsq, 37, elbo, ok_flags)
    assert isinstance(rd, pfmi.RunDiagnostics) and rd.ndraws_per_run == 37
    ess, lev, ok = rr.host_diagnostics(k, lse, sumsq, 37)
    for got, want in ((rd.ess, ess), (rd.log_evidence, lev), (rd.pareto_shape, k), (rd.elbo, np.array(elbo))):
        assert got.dtype == np.float64 and np.all(rr.same_bits(got, want)), (got, want)
    assert rd.ess[0] == 37.0 and rd.ess[1] == 1.0 and rd.ess[2] == 8.0 and np.isnan(rd.ess[3]) and rd.ess[4] == np.inf
    assert rd.log_evidence[1] == -np.log(37.0) and np.isnan(rd.log_evidence[3]) and rd.log_evidence[4] == -np.inf
    np.testing.assert_array_equal(rd.tail_length, M)
    assert rd.tail_length.dtype == np.int64 and rd.success.dtype == bool
    np.testing.assert_array_equal(rd.success, ok_flags)
    got = rd.ok()
    assert got.dtype == bool
    np.testing.assert_array_equal(got, ok)
    np.testing.assert_array_equal(got, [True, True, False, False, True, False])          # 0.7 itself passes, NaN never does
    np.testing.assert_array_equal(rd.ok(threshold=0.5), [True, False, False, False, True, False])
    np.testing.assert_array_equal(rd.ok(threshold=np.inf), [True, True, True, False, True, True])


def test_engine_method_rejects_an_unknown_source_name():
    from pfmi.core import RATIO_SOURCES, Engine
    assert RATIO_SOURCES == {"component": 0, "mixture": 1}
    with pytest.raises(ValueError, match="source"):
        Engine.pool_psis_runs(object(), source="pooled")


def test_header_defines_the_sources_the_python_layer_sends():
    import os
    import re
    from pfmi.core import RATIO_SOURCES
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfmi.h")).read()
    got = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define PFMI_RATIOS_([A-Z]+)\s+(\d+)", txt)}
    assert got == RATIO_SOURCES


@pytest.mark.parametrize("N_r", [37, 1000])
def test_prescribed_vectors_are_what_their_names_say(N_r):
    v = rr.prescribed(N_r)
    M = pr.tail_length(N_r)
    assert all(len(x) == N_r for x in v.values())
    assert {n for pool in rr.PRESCRIBED_POOLS for n in pool} == set(v)
    tail, cut = pr.tail_indices(v["nan_in_tail"])
    assert np.sum(np.isnan(v["nan_in_tail"])) == 1 and np.isnan(v["nan_in_tail"][tail]).sum() == 1
    tail, cut = pr.tail_indices(v["nan_outside_tail"])
    nan = np.isnan(v["nan_outside_tail"])
    assert nan.sum() == M + 2 and np.all(nan[tail]) and nan[cut] and np.sum(nan[np.setdiff1d(np.arange(N_r), tail)]) == 2
    assert np.unique(v["all_equal"]).size == 1 and np.all(v["all_neginf"] == -np.inf)
    assert np.sum(v["one_posinf"] == np.inf) == 1
    z = v["signed_zeros"]
    tail, cut = pr.tail_indices(z)
    zeros = np.flatnonzero(z == 0.0)
    assert np.signbit(z[zeros]).any() and not np.signbit(z[zeros]).all() and z[cut] == 0.0
    assert 0 < np.sum(z[tail] == 0.0) < len(zeros) and not np.signbit(z[tail][z[tail] == 0.0]).any()     # only +0.0 enters the tail
    c = v["constant_tail"]
    tail, cut = pr.tail_indices(c)
    assert np.all(c[tail] == c[cut])
    assert np.isnan(po.psis(c)[2]) and np.isfinite(po.psis(v["light"])[2]) and np.isfinite(po.psis(z)[2])


@needs_ld
@pytest.mark.parametrize("N_r", [37, 1000])
@pytest.mark.parametrize("name", ["lr10", "funnel12"])
def test_oracle_holds_every_run_of_the_named_pools_to_a_tenth_of_the_margins(name, N_r):
    """The admission rule of the PSIS edge suite on the slices the GPU test compares: oracle (fp64) minus long double under
    margin / 10 for pareto_k and the log weights of each run.  The ratios are the oracle's own (its fits, its draws)."""
    import pfmi
    K = 3
    lr = rr.oracle_pool_ratios(pfmi, name, K, N_r)
    assert lr.shape == (K * N_r,) and np.all(np.isfinite(lr))
    for k in range(K):
        s = np.ascontiguousarray(lr[k * N_r:(k + 1) * N_r])
        lw_o, w_o, k_o, M = po.psis(s)
        tail, cut = pr.tail_indices(s)
        assert M == pr.tail_length(N_r)
        lw, w, kk = pr.psis_longdouble(s, tail, cut)
        assert np.all(np.isfinite(lw_o)) and np.all(np.isfinite(lw.astype(np.float64)))
        assert np.isnan(k_o) == bool(np.isnan(kk)), (name, N_r, k, k_o, kk)     # (funnel12's third run: ratios of -1e50, no fit, on both sides)
        dev_lw = float(np.max(np.abs(lw - lw_o.astype(pr.LD)) / (1 + np.abs(lw_o))))
        dev_k = float(abs(kk - pr.LD(k_o))) if np.isfinite(k_o) else 0.0
        print(f"condition {name} N_r {N_r} run {k}: psis_logw {dev_lw:.3g} pareto_k {dev_k:.3g} (k {k_o:.4f})")
        assert dev_lw <= 0.1 * mg.CONTRACT["psis_logw"], (name, N_r, k, dev_lw)
        assert dev_k <= 0.1 * mg.CONTRACT["pareto_k"], (name, N_r, k, dev_k)
