"""pf_mixture_mfma_kernel (csrc/mixture_kernels.hip) at every launch geometry and component group: the loop over the components of
a group (buffers restaged and reused per component), every reachable <kpad, STAGE> instantiation above one 128-row block, both
sides of each STAGE boundary, the d edges of the row mapping, and the claim that the result does not depend on the grid.

The rows, their targets and the rule that picks their components are tests/mixture_reference.py's; test_mixture_reference_cpu.py
shows on the CPU that for these components and points a stale T, V, Vh, mu or 1 / sqrt(alpha) of the previous component moves a
column by 100 x the bound asserted here.  PFMI_MIXTURE_CPB sets the components per workgroup."""
import numpy as np
import pytest
from scipy.special import logsumexp

import margins as mg
import mixture_reference as R
from helpers import fit_seeds, make_traces
from test_gpu_mixture import _check_case, _set_kernel

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.SKIP_REASON)]


def _set_cpb(pfmi_mod, n):
    assert pfmi_mod.lib().pfmi_debug_set(b"PFMI_MIXTURE_CPB", str(n).encode() if n else None) == 0


def _mix(pfmi_mod, eng, pts, X, cpb=None, kernel=None):
    """(lse, comp) with the group size / kernel forced for this call only"""
    _set_cpb(pfmi_mod, cpb)
    _set_kernel(pfmi_mod, kernel)
    try:
        return eng.mixture_logpdf(pts, X, componentwise=True)
    finally:
        _set_cpb(pfmi_mod, None)
        _set_kernel(pfmi_mod, None)


def _bits(a, b, what=None):
    np.testing.assert_array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64), err_msg=str(what))


def _ncu(eng):
    import torch
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


class Rows:
    """the fits of one (J, d) row live on the module's engine; traces, components and points of every row are kept"""

    def __init__(self, pfmi_mod, eng):
        self.pfmi, self.eng, self.current, self.rows, self.traces = pfmi_mod, eng, None, {}, {}

    def use(self, J, d, per_path=R.PER_PATH):
        key = (J, d, per_path)
        eng = self.eng
        row = self.rows.get(key)
        if self.current != (J, d):
            if (J, d) not in self.traces:
                self.traces[(J, d)] = R.grid_traces(self.pfmi, J, d)
            traces = self.traces[(J, d)]
            eng.set_target(R.grid_target(self.pfmi, d))
            eng.set_traces([t.points for t in traces], [t.gradients for t in traces])
            eng.fit_batch(J)
            self.current = (J, d)
        if row is None:
            status, jeff, _, _ = eng.fit_status()
            assert jeff.max() == J                        # the history fills: every kpad column of these components is real
            pts = R.pick_points(np.diff(eng.offsets), jeff, J, per_path)
            assert all(status[p] == 0 and jeff[p] == J for p in pts)
            fits = {p: eng.get_fit(p, J) for p in pts}
            seeds = fit_seeds(max(pts) + 1, 11)
            X = R.make_points(pts, fits, lambda p: eng.draws(p, seeds[p], 4)[0])
            row = self.rows[key] = dict(pts=pts, fits=fits, X=X)
        return row["pts"], row["fits"], row["X"]

    def forget(self):
        self.current = None


@pytest.fixture(scope="module")
def rows(pfmi_mod, eng):
    return Rows(pfmi_mod, eng)


# ---- a. instantiation x STAGE x d --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,d,stage", [r for r in R.GRID if r[2] is not None], ids=lambda v: str(v))
def test_every_instantiation_one_workgroup_per_tile(pfmi_mod, eng, rows, J, d, stage):
    """all six components in one workgroup (cpb = K): every buffer of the loop is reused five times; N = 37, a ragged last tile"""
    pts, fits, X = rows.use(J, d)
    assert X.shape[1] == 37 and len(pts) == 6
    geo = R.mixture_geometry(d, R.kpad_for(J), X.shape[1], len(pts), _ncu(eng))
    assert geo["route"] == "mfma" and geo["stage"] == stage, geo
    _set_cpb(pfmi_mod, len(pts))
    try:
        _check_case(pfmi_mod, eng, f"geom-J{J}-d{d}", pts, fits, X)
    finally:
        _set_cpb(pfmi_mod, None)


def test_lane_route_past_1024_rows(pfmi_mod, eng, rows):
    J, d, _ = R.GRID[-1]
    pts, fits, X = rows.use(J, d)
    assert R.mixture_geometry(d, R.kpad_for(J), X.shape[1], len(pts), _ncu(eng))["route"] == "lane"
    lse, comp = _mix(pfmi_mod, eng, pts, X, cpb=len(pts))                # the hook has no effect on this route
    for k, p in enumerate(pts):
        _bits(comp[:, k], eng.logpdf(p, X), k)
        mg.check(f"geom-J{J}-d{d}", "logq@mixture_vs_longdouble", mg.rel(comp[:, k], R.ref_logpdf(fits[p], X)))
    ref_lse = logsumexp(comp, axis=1)
    mg.check(f"geom-J{J}-d{d}", "lse@mixture", np.abs(lse - ref_lse) / np.maximum(np.abs(ref_lse), 1.0), bound=1e-13)


# ---- b. group-size invariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,d", R.INVARIANCE, ids=lambda v: str(v))
def test_group_size_does_not_change_a_bit(pfmi_mod, eng, rows, J, d):
    """K = 7 (six fits of both paths, the first again): cpb 1, 2, 3, 7 -- groups of 1; 2, 2, 2, 1; 3, 3, 1; 7 -- give the same bits,
    and every column is the K = 1 call of its component"""
    pts, fits, X = rows.use(J, d)
    pts7 = pts + [pts[0]]
    base = _mix(pfmi_mod, eng, pts7, X, cpb=1)
    assert np.all(np.isfinite(base[1])) and np.all(np.isfinite(base[0]))
    for cpb in (2, 3, 7):
        lse, comp = _mix(pfmi_mod, eng, pts7, X, cpb=cpb)
        _bits(comp, base[1], cpb)
        _bits(lse, base[0], cpb)
    for k, p in enumerate(pts7):
        lse1, comp1 = _mix(pfmi_mod, eng, [p], X)
        _bits(base[1][:, k], comp1[:, 0], k)
        _bits(lse1, comp1[:, 0], k)


# ---- c. failed fits inside a group ---------------------------------------------------------------------------------------------------------
def test_failed_fits_inside_a_group(pfmi_mod, eng, rows):
    """[ok, bad, ok, bad, bad, ok] in one group of six and in groups of two: a skipped component leaves its column NaN and the
    buffers to the next good one (the construction of test_gpu_mixture.py's failed fit)"""
    J, d = R.FAILED
    rows.forget()
    rng = np.random.default_rng(0)
    bad_th, bad_gr = np.cumsum(rng.normal(size=(9, d)), 0), rng.normal(size=(9, d))
    tg = pfmi_mod.t_diag(d, seed=3)
    good = make_traces(tg, 1, 3)[0]
    eng.set_target(tg)
    eng.set_traces([bad_th, good.points], [bad_gr, good.gradients])
    eng.fit_batch(J, -1e300)
    status, jeff, _, _ = eng.fit_status()
    bad = [p for p in range(9) if status[p] != 0]
    assert bad, status
    ok = [9 + p for p in R.pick_points([len(good)], jeff[9:], J)]
    assert all(status[p] == 0 for p in ok) and len(set(ok)) == 3
    pts = [ok[0], bad[0], ok[1], bad[-1], bad[len(bad) // 2], ok[2]]
    good_cols = [0, 2, 5]
    X = np.asfortranarray(np.random.default_rng(1).normal(size=(d, 20)))
    want_lse, want = _mix(pfmi_mod, eng, ok, X)
    assert np.all(np.isfinite(want))
    for k, p in enumerate(ok):
        mg.check("geom-failed-fit", "logq@mixture_vs_logpdf", mg.rel(want[:, k], eng.logpdf(p, X)))
    for cpb in (6, 2):
        for kernel in (None, "lane"):
            lse, comp = _mix(pfmi_mod, eng, pts, X, cpb=cpb, kernel=kernel)
            assert np.all(np.isnan(comp[:, [1, 3, 4]])) and np.all(np.isnan(lse)), (cpb, kernel)
            if kernel is None:
                _bits(comp[:, good_cols], want, cpb)
            else:
                for k, p in zip(good_cols, ok):
                    _bits(comp[:, k], eng.logpdf(p, X), (cpb, k))


# ---- d. the unforced launcher ----------------------------------------------------------------------------------------------------------------
def test_unforced_launcher_loops_over_components(pfmi_mod, eng, rows):
    """no hook: N = natural_N(ncu) and K = 20 make the launcher itself choose groups of 3 with a last group of 2"""
    J, d = R.NATURAL
    pts, fits, X0 = rows.use(J, d, per_path=10)
    ncu = _ncu(eng)
    N = R.natural_N(ncu)
    geo = R.mixture_geometry(d, R.kpad_for(J), N, len(pts), ncu)
    assert len(pts) == 20 and geo["route"] == "mfma" and geo["cpb"] == 3 and geo["ngroups"] == 7, geo
    seeds = fit_seeds(max(pts) + 1, 12)
    per = -(-(N - X0.shape[1]) // len(pts))
    X = np.asfortranarray(np.concatenate([X0] + [eng.draws(p, seeds[p], per)[0] for p in pts], axis=1)[:, :N])
    assert X.shape[1] == N
    lse, comp = eng.mixture_logpdf(pts, X, componentwise=True)
    lse1, comp1 = _mix(pfmi_mod, eng, pts, X, cpb=1)
    _bits(comp, comp1)
    _bits(lse, lse1)
    cols = np.unique(np.r_[np.arange(16), np.arange(N - N % 16, N), np.random.default_rng(3).choice(N, 64, replace=False)])
    for k, p in enumerate(pts):
        ref = R.ref_logpdf(fits[p], X[:, cols])
        mg.check("geom-natural-K20", "logq@mixture_vs_longdouble", mg.rel(comp[cols, k], ref))
    ref_lse = logsumexp(comp, axis=1)
    mg.check("geom-natural-K20", "lse@mixture", np.abs(lse - ref_lse) / np.maximum(np.abs(ref_lse), 1.0), bound=1e-13)


# ---- e. tile-position invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,d", [(6, 33), (10, 641)], ids=lambda v: str(v))
def test_a_column_has_the_same_bits_wherever_it_stands(pfmi_mod, eng, rows, J, d):
    pts, fits, X = rows.use(J, d)
    for src in (0, 5):                                    # a draw and a far point of the first component
        x = X[:, src:src + 1]
        lse1, comp1 = _mix(pfmi_mod, eng, pts, x)
        for N in (1, 17, 37):
            for j in sorted({0, 15, 16, N - 1}):
                if j >= N:
                    continue
                XN = np.asfortranarray(X[:, :N].copy())
                XN[:, j] = x[:, 0]
                for cpb in (None, len(pts)):
                    lse, comp = _mix(pfmi_mod, eng, pts, XN, cpb=cpb)
                    _bits(comp[j], comp1[0], (src, N, j, cpb))
                    _bits(lse[j], lse1[0], (src, N, j, cpb))


# ---- f. column isolation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,d", [(6, 33), (10, 641)], ids=lambda v: str(v))
def test_a_non_finite_column_stays_in_its_column(pfmi_mod, eng, rows, J, d):
    pts, fits, X = rows.use(J, d)
    j = 20
    others = np.arange(X.shape[1]) != j
    for kernel in (None, "lane"):
        clean = _mix(pfmi_mod, eng, pts, X, cpb=len(pts), kernel=kernel)
        for what in ("nan column", "inf entry"):
            Xb = X.copy(order="F")
            if what == "nan column":
                Xb[:, j] = np.nan
            else:
                Xb[d // 2, j] = np.inf
            lse, comp = _mix(pfmi_mod, eng, pts, Xb, cpb=len(pts), kernel=kernel)
            assert not np.any(np.isfinite(comp[j])) and not np.any(comp[j] == np.inf), (kernel, what, comp[j])
            assert not np.isfinite(lse[j]) and lse[j] != np.inf, (kernel, what, lse[j])
            _bits(comp[others], clean[1][others], (kernel, what))
            _bits(lse[others], clean[0][others], (kernel, what))


# ---- g. overflow -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,d", [(6, 33), (10, 641)], ids=lambda v: str(v))
def test_overflow_gives_minus_infinity_not_nan(pfmi_mod, eng, rows, J, d):
    """a column of 1e160: the squares overflow, every component is -inf and lse takes its all -inf branch"""
    pts, fits, X = rows.use(J, d)
    Xb = X.copy(order="F")
    Xb[:, 20] = 1e160
    for kernel in (None, "lane"):
        lse, comp = _mix(pfmi_mod, eng, pts, Xb, cpb=len(pts), kernel=kernel)
        assert np.all(comp[20] == -np.inf) and lse[20] == -np.inf, (kernel, comp[20], lse[20])
        assert np.all(np.isfinite(np.delete(lse, 20)))
