"""CPU side of the mixture-proposal weights (tests/test_gpu_pool_mixture.py): the long-double reference against itself at the shapes
the row-tiled kernel is checked at, the build of every instantiation of pf_pool_mixture_tiled_kernel for gfx950 with no more scratch
than the kernel it was cut from, and the `proposal` keyword where it is decided before any device is touched."""
import os
import sys

import numpy as np
import pytest

import mixture_reference as R
import pool_mixture_common as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.SKIP_REASON)
DENSE_MAX = 1500         # the long-double Cholesky of the dense route is d^3 / 3 long-double operations in NumPy: seconds up to here


@pytest.fixture(scope="module")
def pfmi_cpu():
    import pfmi
    return pfmi


def _last_fits(traces, J):
    """the oracle's fit of every trace's last point, as ref_logpdf takes it (the fits pool_common._pool pools)"""
    from gpu_common import _oracle_factor
    from oracle import pf_oracle as po
    fits = []
    for tr in traces:
        alpha_all, hl, hs, _ = po.lbfgs_history(tr.points, tr.gradients, J)
        l, d = len(tr) - 1, tr.points.shape[1]
        F = _oracle_factor(tr, alpha_all, hl, hs, l, d)
        assert F.status == 0
        fits.append(dict(alpha=F.alpha, B=F.B, D=F.D, mu=F.fit_mean(tr.points[l], tr.gradients[l])))
    return fits


def _columns(fits, n=4, seed=5):
    """of every fit: n points at the scale of its diagonal, the next fit's mean, and a point 50 such standard deviations out"""
    rng = np.random.default_rng(seed)
    cols = []
    for k, f in enumerate(fits):
        d = len(f["mu"])
        cols.append(f["mu"][:, None] + np.sqrt(f["alpha"])[:, None] * rng.normal(size=(d, n)))
        cols.append(fits[(k + 1) % len(fits)]["mu"][:, None])
        v = rng.normal(size=d)
        cols.append((f["mu"] + 50 * np.sqrt(f["alpha"]) * v / np.linalg.norm(v))[:, None])
    return np.concatenate(cols, axis=1)


@needs_ld
@pytest.mark.parametrize("J,d", M.SHAPES, ids=lambda v: str(v))
def test_reference_routes_agree_at_the_tiled_shapes(pfmi_cpu, J, d):
    """Where the dense route is affordable (d <= 1500) Cholesky and Woodbury in long double agree, per component relative to
    max(|logpdf|, 1), to 1e-14: ten times tighter than the floor of the tiled kernel's bound.  Above, the Woodbury route is the only
    one and is checked for what does not need the other: finite values, and the mean of a fit is its mode."""
    if d == 10000:
        from pool_common import _traces
        fits = _last_fits(_traces(pfmi_cpu, "d10000")[1][:2], 6)
    else:
        pts, all_fits, _ = R.oracle_components(R.grid_traces(pfmi_cpu, J, d), J, per_path=1)
        fits = [all_fits[p] for p in pts]
    X = _columns(fits)
    for k, f in enumerate(fits):
        w = R.ref_logpdf(f, X, route="woodbury")
        assert np.all(np.isfinite(w))
        at_mean = R.ref_logpdf(f, f["mu"][:, None], route="woodbury")[0]
        assert np.all(w <= at_mean)
        if d <= DENSE_MAX:
            a = R.ref_logpdf(f, X, route="dense")
            dev = float(np.max(np.abs(a - w) / np.maximum(np.abs(a), 1)))
            print(f"reference routes J={J} d={d} component {k}: max deviation {dev:.3e}")
            assert dev <= M.FLOOR / 10, (J, d, k, dev)


@needs_ld
def test_long_double_lse_matches_scipy():
    from scipy.special import logsumexp
    rng = np.random.default_rng(0)
    comp = rng.normal(size=(3, 50)) * 300
    np.testing.assert_allclose(np.asarray(M.lse_ld(comp), dtype=np.float64), logsumexp(comp, axis=0), rtol=1e-15)
    assert M.tiled_bound(0.0) == M.FLOOR and M.tiled_bound(1e-12) == 4e-12


# ---- the build ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    return kr.kernel_resources()


@pytest.mark.parametrize("kpad", [4, 8, 12, 16, 20, 32])
def test_tiled_kernel_builds_without_more_scratch_than_the_kernel_it_was_cut_from(table, kpad):
    """every instantiation is in the gfx950 code object, and spills no more than pf_mixture_mfma_kernel<KPAD, false> of the same build"""
    mine = [k for k in table if k.startswith(f"pf_pool_mixture_tiled_kernel<{kpad}>(")]
    base = [k for k in table if k.startswith(f"pf_mixture_mfma_kernel<{kpad}, false>(")]
    assert len(mine) == 1 and len(base) == 1, (mine, base)
    a, b = table[mine[0]], table[base[0]]
    assert a["private_segment_fixed_size"] <= b["private_segment_fixed_size"], (a, b)
    assert a["vgpr_spill_count"] <= b["vgpr_spill_count"], (a, b)
    assert a["vgpr_count"] <= 256                      # 512 threads: two waves per SIMD or the workgroup does not launch


def test_ratio_kernel_is_in_the_build(table):
    assert [k for k in table if k.startswith("pf_pool_mixture_ratio_kernel(")]


def test_entry_points_are_exported():
    import pfmi
    from pfmi._lib import SYMBOLS
    assert "pfmi_pool_mixture_ratios" in SYMBOLS and "pfmi_pool_mixture_ratios_dev" in SYMBOLS
    assert hasattr(pfmi.Engine, "pool_mixture_ratios") and hasattr(pfmi.Engine, "pool_mixture_ratios_dev")


# ---- the keyword ------------------------------------------------------------------------------------------------------------------------
def test_proposal_keyword_is_validated_before_any_device_work(pfmi_cpu):
    tg = pfmi_cpu.t_diag(3)
    with pytest.raises(ValueError, match="proposal"):
        pfmi_cpu.multipathfinder(tg, 10, nruns=2, proposal="balance")
    with pytest.raises(ValueError, match="importance"):
        pfmi_cpu.multipathfinder(tg, 10, nruns=2, proposal="mixture", importance=False)
    with pytest.raises(ValueError, match="one engine"):
        pfmi_cpu.multipathfinder(tg, 10, nruns=2, proposal="mixture", engines=[object(), object()])


def test_resample_inherits_and_validates_the_proposal(pfmi_cpu):
    from pfmi.api import MultiPathfinderResult
    res = MultiPathfinderResult(None, None, None, [], np.zeros((3, 0)), np.zeros(0), [], None, object(), 5, [object(), object()],
                                "mixture")
    assert MultiPathfinderResult(None, None, None, [], None, None, [], None).proposal == "component"
    with pytest.raises(ValueError, match="one engine"):        # proposal=None takes the result's "mixture": two engines
        pfmi_cpu.resample(res, 10)
    with pytest.raises(ValueError, match="importance"):
        pfmi_cpu.resample(res, 10, importance=False)
    with pytest.raises(ValueError, match="proposal"):
        pfmi_cpu.resample(res, 10, proposal="other")
