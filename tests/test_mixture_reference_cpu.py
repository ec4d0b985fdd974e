"""CPU side of the mixture geometry tests (tests/test_gpu_mixture_geometry.py): the restated launch rules of
pf_launch_mixture_logpdf pinned at the shapes the GPU tests rely on, the long-double reference against itself, and the condition
under which a stale buffer inside the component loop of pf_mixture_mfma_kernel cannot hide: for the very components and points the
grouped GPU tests use, built here from the oracle's factors, taking any one of T, V, Vh, mu or 1 / sqrt(alpha) from the previous
component of the group moves some test column by 100 x the bound those tests assert."""
import numpy as np
import pytest

import mixture_reference as R

LD = np.longdouble
needs_ld = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.SKIP_REASON)


# ---- the launcher's rules ------------------------------------------------------------------------------------------------------------
def test_static_lds_table_is_the_kernels_formula():
    for kpad, n in R.MX_STATIC_LDS.items():
        assert R.mx_static_lds(kpad) == n


@pytest.mark.parametrize("kpad", [4, 8, 12])
def test_stage_for_every_d_at_kpad_up_to_12(kpad):
    for d in range(1, 1025):
        g = R.mixture_geometry(d, kpad, 37, 6, 256)
        assert g["route"] == "mfma" and g["stage"], (d, g)


@pytest.mark.parametrize("kpad,last", [(16, 896), (20, 640), (32, 352)])
def test_stage_boundaries(kpad, last):
    for d in range(1, 1025):
        assert R.mixture_geometry(d, kpad, 37, 6, 256)["stage"] == (d <= last), d


def test_largest_lds_request():
    assert R.mixture_geometry(896, 16, 37, 6, 256)["lds_bytes"] == 159744
    # the largest request of any launch: kpad 20 at d = 640 (a row of the grid), 256 bytes under the limit
    most = max((R.mixture_geometry(d, kpad, 37, 6, 256)["lds_bytes"], kpad, d) for kpad in R.MX_STATIC_LDS for d in range(1, 1025))
    assert most == (163584, 20, 640) and most[0] <= R.MX_LDS_MAX


def test_lane_route():
    assert R.mixture_geometry(1025, 12, 37, 6, 256)["route"] == "lane"
    assert R.mixture_geometry(80, 64, 37, 6, 256)["route"] == "lane"
    assert R.mixture_geometry(1024, 32, 37, 6, 256)["route"] == "mfma"
    assert R.kpad_for(16) == 32 and R.kpad_for(17) == 64 and [R.kpad_for(J) for J in (2, 4, 6, 8, 10)] == [4, 8, 12, 16, 20]


def test_grid_rows_hit_what_they_are_meant_to():
    """the nine reachable instantiations at d > 128, and the expected STAGE of every row"""
    seen = set()
    for J, d, stage in R.GRID:
        g = R.mixture_geometry(d, R.kpad_for(J), 37, 6, 256)
        assert (g["route"] == "lane") == (stage is None) and (stage is None or g["stage"] == stage), (J, d, g)
        if stage is not None and d > 128:
            seen.add((R.kpad_for(J), g["stage"]))
    assert seen == {(4, True), (8, True), (12, True), (16, True), (16, False), (20, True), (20, False), (32, True), (32, False)}


@pytest.mark.parametrize("ncu", [15, 64, 104, 256, 304])
def test_natural_N_makes_the_launcher_loop(ncu):
    N = R.natural_N(ncu)
    g = R.mixture_geometry(64, 12, N, 20, ncu)
    assert g["cpb"] == 3 and g["ngroups"] == 7 and 20 - 3 * (g["ngroups"] - 1) == 2, g
    assert N % 16 == 5


def test_small_calls_never_loop():
    """what the suite had before: N <= 80 points and K <= 8 components give one component per workgroup"""
    for N in (20, 37, 80):
        for K in range(1, 9):
            assert R.mixture_geometry(50, 12, N, K, 256)["cpb"] == 1


# ---- the reference against itself ----------------------------------------------------------------------------------------------------
def _synthetic_fit(d, m, seed):
    """a well-conditioned fit: alpha in [0.5, 2], B with orthonormal columns, D = C C' with eigenvalues in [0.25, 4]"""
    rng = np.random.default_rng(seed)
    B = np.linalg.qr(rng.normal(size=(d, m)))[0]
    Q = np.linalg.qr(rng.normal(size=(m, m)))[0]
    D = (Q * np.exp(rng.uniform(np.log(0.25), np.log(4.0), m))) @ Q.T
    return dict(alpha=np.exp(rng.uniform(np.log(0.5), np.log(2.0), d)), B=B, D=(D + D.T) / 2, mu=rng.normal(size=d))


@needs_ld
@pytest.mark.parametrize("d", [40, 200])
def test_reference_routes_agree(d):
    """dense Cholesky and Woodbury in long double differ by long-double rounding only: 1e-15 (1 + |.|), six orders below the contract
    (measured: profiles/mixture_parity.md)"""
    f = _synthetic_fit(d, 12, d)
    rng = np.random.default_rng(1)
    X = f["mu"][:, None] + rng.normal(size=(d, 24)) * np.r_[np.ones(12), np.full(6, 7.0), np.full(6, 50.0)]
    a, b = R.ref_logpdf(f, X, route="dense"), R.ref_logpdf(f, X, route="woodbury")
    dev = np.max(np.abs(a - b) / (1 + np.abs(a)))
    print(f"reference routes d={d}: max deviation {dev:.3e}")
    assert dev <= 1e-15
    np.testing.assert_array_equal(R.ref_logpdf(f, X), a if d <= 64 else b)


# ---- a stale buffer would show ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pfmi_cpu():
    import pfmi
    return pfmi


def _sensitivity(name, pts, fits, comps, X):
    """every swap of one buffer of component k for that of component k - 1 moves a column by >= 1e-7 (1 + |ref|)"""
    worst = {}
    for k in range(1, len(pts)):
        cur, prev = comps[pts[k]], comps[pts[k - 1]]
        if pts[k] == pts[k - 1]:
            continue
        ref = R.lane_logpdf(cur, X)
        if R.HAVE_LONGDOUBLE:                             # the float64 statement is the density of the fit
            assert np.max(np.abs(ref - R.ref_logpdf(fits[pts[k]], X)) / (1 + np.abs(ref))) <= 1e-9, (name, k)
        for key in ("T", "V", "Vh", "mu", "rsqa"):
            moved = np.max(np.abs(R.lane_logpdf(dict(cur, **{key: prev[key]}), X) - ref) / (1 + np.abs(ref)))
            worst[key] = min(worst.get(key, np.inf), moved)
            assert moved >= 1e-7, (name, k, key, moved)
    print(f"sensitivity {name}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return worst


def _row(pfmi, J, d, per_path=R.PER_PATH):
    pts, fits, comps = R.oracle_components(R.grid_traces(pfmi, J, d), J, per_path)
    return pts, fits, comps, R.make_points(pts, fits, R.oracle_draws(fits, comps))


@pytest.mark.parametrize("J,d", [(J, d) for J, d, stage in R.GRID if stage is not None], ids=lambda v: str(v))
def test_stale_buffer_would_show_grid(pfmi_cpu, J, d):
    """rows of the instantiation grid and of the group-size invariance test: 6 components, the 7th of the invariance test repeats
    the first (its predecessor is the 6th, another fit)"""
    pts, fits, comps, X = _row(pfmi_cpu, J, d)
    assert X.shape[1] == 37 and len(set(pts)) == 6
    _sensitivity(f"J{J}-d{d}", pts + [pts[0]], fits, comps, X)


def test_stale_buffer_would_show_natural(pfmi_cpu):
    """the 20 components of the unforced-launcher test"""
    J, d = R.NATURAL
    pts, fits, comps, X = _row(pfmi_cpu, J, d, per_path=10)
    assert len(set(pts)) == 20
    _sensitivity(f"J{J}-d{d}-K20", pts, fits, comps, X)


def test_stale_buffer_would_show_failed_fit_case(pfmi_cpu):
    """the good components of the failed-fit test (a component after a skipped one meets the buffers of the last good one)"""
    from helpers import make_traces
    J, d = R.FAILED
    good = make_traces(pfmi_cpu.t_diag(d, seed=3), 1, 3)
    pts, fits, comps = R.oracle_components(good, J)
    X = np.asfortranarray(np.random.default_rng(1).normal(size=(d, 20)))
    _sensitivity("failed-fit", pts, fits, comps, X)
