"""PSIS and index selection at every route boundary and special value (csrc/psis_kernels.hip).

The pools are the rows of tests/psis_reference.py:CASES -- each pinned on the CPU to the launcher boundary it sits on, to a reference
error of less than a tenth of the parity margins, and (tie rows) to a visible effect of a tie broken the wrong way
(tests/test_psis_reference_cpu.py).  Every row runs on each route it lists: as launched, PFMI_PSIS_KERNEL=single (one workgroup) and
PFMI_PSIS_KERNEL=big (global sort), a fresh Engine per run, against the CPU oracle and against each other.  The second group runs the
four index samplers at their tile / chunk / route sizes against the oracle's samplers, bit for bit."""
import numpy as np
import pytest

from oracle import pf_oracle as po
import margins as mg
import psis_reference as pr

pytestmark = pytest.mark.gpu


def _psis_on_route(pfmi_mod, monkeypatch, lr, force):
    if force == "natural":
        monkeypatch.delenv("PFMI_PSIS_KERNEL", raising=False)
    else:
        monkeypatch.setenv("PFMI_PSIS_KERNEL", force)
    eng = pfmi_mod.Engine(0)
    try:
        return eng.psis(lr)
    finally:
        eng.close()
        monkeypatch.delenv("PFMI_PSIS_KERNEL", raising=False)


@pytest.mark.parametrize("id", [c.id for c in pr.CASES])
def test_psis_edge_case_on_every_route(pfmi_mod, monkeypatch, id):
    case = pr.CASE[id]
    lr = case.lr()
    S = len(lr)
    lw_o, w_o, k_o, M = pr.case_oracle(id)
    fin = np.isfinite(lw_o)
    res = {}
    for force in case.routes:
        a = res[force] = _psis_on_route(pfmi_mod, monkeypatch, lr, force)
        cfg = f"psis_edges {id} {force}:{pr.route(S, None if force == 'natural' else force)}"
        assert a["tail_length"] == M == pr.tail_length(S), cfg
        for name, ref in (("log_weights", lw_o), ("weights", w_o)):
            np.testing.assert_array_equal(np.isfinite(a[name]), np.isfinite(ref), err_msg=f"{cfg} isfinite({name})")
            np.testing.assert_array_equal(np.isnan(a[name]), np.isnan(ref), err_msg=f"{cfg} isnan({name})")
        np.testing.assert_array_equal(a["log_weights"][~fin & ~np.isnan(lw_o)], lw_o[~fin & ~np.isnan(lw_o)], err_msg=f"{cfg} +-Inf")
        assert np.isnan(a["pareto_shape"]) == np.isnan(k_o), (cfg, a["pareto_shape"], k_o)
        if fin.any():
            dev_lw = np.max(np.abs(a["log_weights"][fin] - lw_o[fin]) / (1 + np.abs(lw_o[fin])))
            wf = np.isfinite(w_o)                                      # (the zero weights of -Inf log ratios included)
            dev_w = np.max(np.abs(a["weights"][wf] - w_o[wf])) / np.max(w_o[wf])
            dev_k = abs(a["pareto_shape"] - k_o) if np.isfinite(k_o) else 0.0
            print(f"{cfg}: psis_logw {dev_lw:.3g} psis_w {dev_w:.3g} pareto_k {dev_k:.3g} (k {k_o:.4f})")
            mg.check(cfg, "psis_logw", dev_lw)
            mg.check(cfg, "psis_w", dev_w)
            mg.check(cfg, "pareto_k", dev_k)
        if np.isfinite(w_o.sum()):
            assert abs(a["weights"].sum() - 1.0) <= 1e-12, (cfg, a["weights"].sum())
        if id in pr.NAN_CASES:
            assert np.all(np.isnan(a["log_weights"])) and np.all(np.isnan(a["weights"])) and np.isnan(a["pareto_shape"]), cfg
    # the routes agree with each other far inside the margin against the oracle
    b = res["natural"]
    for force in case.routes[1:]:
        a = res[force]
        if np.isfinite(k_o):
            assert abs(a["pareto_shape"] - b["pareto_shape"]) <= 1e-13 * (1 + abs(b["pareto_shape"])), (id, force)
        if fin.any():
            assert np.max(np.abs(a["log_weights"][fin] - b["log_weights"][fin])) <= 1e-12 * (1 + np.abs(b["log_weights"][fin]).max()), (id, force)


# ---- index samplers ----------------------------------------------------------------------------------------------------------------
def _install(eng, lr):
    """the weights PSIS leaves on the engine for these log ratios (downloaded: the oracle samples from the same numbers)"""
    return eng.psis(lr)["weights"]


@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("S", pr.CDF_SIZES)
def test_fixed_point_cdf_sampler_at_tile_edges(pfmi_mod, eng, S, one_hot):
    """pf_cdf_kernel + pf_sample_kernel: 256-element tiles with 4 elements per lane (S = 1, 3, 255, 256, 257), 16 waves with one and
    two tiles each (4096 | 4097), S = 65 537; weights with exact zeros at both ends of the pool, or one weight 1 and the rest 0;
    uniforms 0, nextafter(1, 0) and ones whose scaled draw equals a CDF entry."""
    w = _install(eng, pr.sampler_log_ratios(S, S, one_hot))
    if one_hot:
        assert np.sum(w == 1.0) == 1 and np.sum(w == 0.0) == S - 1
    elif S >= 3:
        assert w[0] == 0.0 and w[-1] == 0.0 and np.all(np.isfinite(w))
    idx = eng.resample_indices(S, 300, seed=17)
    np.testing.assert_array_equal(idx, po.sample_weighted(w, 300, seed=17))
    assert np.all(w[idx] > 0.0)
    hits = pr.cdf_hit_uniforms(w)
    assert len(hits) > 0 or one_hot or S < 4096
    u = np.concatenate([[0.0, np.nextafter(1.0, 0.0), 0.5], hits, np.random.default_rng(S).random(200)])
    idx = eng.resample_indices(S, len(u), uniforms=u)
    np.testing.assert_array_equal(idx, po.sample_weighted(w, len(u), uniforms=u))
    assert np.all(w[idx] > 0.0)
    pos = np.flatnonzero(w > 0.0)
    assert idx[0] == pos[0] and idx[1] == pos[-1]                      # u = 0 and u -> 1 take the first and the last positive weight


@pytest.mark.parametrize("S", pr.SEQCDF_SIZES)
def test_direct_sampler_at_chunk_edges(pfmi_mod, eng, S):
    """pf_seqcdf_kernel + pf_direct_sample_kernel: 4096-element chunks with the running sum carried across them; uniforms 0,
    nextafter(1, 0) and exact entries of the running sum; zero weights at both ends.  Against the oracle's literal loop and the
    np.cumsum / searchsorted restatement (both sequential fp64 sums)."""
    w = _install(eng, pr.sampler_log_ratios(S, 7 * S))
    cw = np.cumsum(w)
    on = cw[np.unique(np.concatenate([[0, S // 2, S - 1], np.arange(4090, min(S, 4100)), np.arange(8186, min(S, 8193))]).clip(0, S - 1))]
    u = np.concatenate([[0.0, np.nextafter(1.0, 0.0), 0.5], on[on < 1.0], np.nextafter(on[on < 1.0], 2.0).clip(0.0, np.nextafter(1.0, 0.0)),
                        np.random.default_rng(S).random(300)])
    idx = eng.resample_indices_direct(S, u)
    np.testing.assert_array_equal(idx, po.sample_direct(w, u))
    np.testing.assert_array_equal(idx, np.minimum(np.searchsorted(cw, u, side="left"), S - 1))
    with pytest.raises(pfmi_mod.PfmiError, match="not in"):
        eng.resample_indices_direct(S, np.array([1.0]))


def _sparse_log_ratios(S, npos, seed):
    rng = np.random.default_rng(seed)
    lr = np.full(S, -np.inf)
    lr[rng.choice(S, npos, replace=False)] = rng.normal(size=npos) * 1.5
    return lr


@pytest.mark.parametrize("S,npos,ndraws", [
    (64, 64, (1, 64)),                        # S <= 64: ndraws = 1 and ndraws = S
    (37, 10, (1, 10)),                        # exactly ndraws positive weights
    (8192, 100, (1, 100)),                    # LDS route (ndraws <= 4096), power-of-two pool
    (8192, 5000, (4096, 4097, 5000)),         # global sort with n2 == S: no padding
    (8192, 8192, (8192,)),
    (8193, 5000, (4096, 4097, 5000)),         # global sort, nearly half the array is padding
    (8193, 8193, (8193,)),
])
def test_without_replacement_counts_and_routes(pfmi_mod, eng, S, npos, ndraws):
    """Efraimidis-Spirakis without replacement through the LDS select (ndraws <= 4096) and the global sort: bit-exact against the
    oracle; exactly ndraws positive weights succeed, one fewer raises"""
    w = _install(eng, _sparse_log_ratios(S, npos, S + npos))
    assert np.sum(w > 0.0) == npos
    for nd in ndraws:
        idx = eng.resample_indices(S, nd, replace=False, seed=23)
        assert len(set(idx.tolist())) == nd and np.all(w[idx] > 0.0)
        np.testing.assert_array_equal(idx, po.sample_weighted_norep(w, nd, seed=23))
    if npos < S:
        with pytest.raises(ValueError):
            po.sample_weighted_norep(w, npos + 1, seed=23)
        with pytest.raises(pfmi_mod.PfmiError):
            eng.resample_indices(S, npos + 1, replace=False, seed=23)


def test_sampling_from_a_pool_without_weight_raises(pfmi_mod, eng):
    """every log ratio -Inf: the weights are NaN, the fixed-point CDF is all zero, and drawing is an error, not index 0"""
    S = 1000
    w = _install(eng, np.full(S, -np.inf))
    assert np.all(np.isnan(w))
    with pytest.raises(ValueError):
        po.sample_weighted(w, 10, seed=1)
    with pytest.raises(pfmi_mod.PfmiError):
        eng.resample_indices(S, 10, seed=1)
    with pytest.raises(pfmi_mod.PfmiError):
        eng.resample_indices(S, 10, replace=False, seed=1)
