"""Pins tests/draw_reference.py on the CPU: the long-double compact-WY reference against the reflector form, the reference's bounds
against two double-precision implementations that are right (they must stay inside) and against nine that are wrong (each must
exceed its bound a hundredfold), and the Python mirror of the draw kernels' dispatch with the grid of
tests/test_gpu_draw_reference.py (every reachable plan is hit; the unreachable ones are named with their reason).  CPU only.

The fits are the oracle's (oracle/pf_oracle.c) on its own L-BFGS traces; T is LAPACK's dlarft in long double, rounded to double where
the reference is to see what the GPU's draw kernels see (a T in double).  Sizes are small versions of the GPU grid: d below, at and
above KC, one and several 16-row blocks, a ragged last block, k = d < KC, k < KC <= d, and one d with two 128-row chunks."""
import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import draw_reference as dr                                    # noqa: E402
import margins as mg
import scan_reference as sr
from oracle import pf_oracle as po
from test_scan_reference_cpu import _fits, _gauss

EPS = dr.EPS

# (d, J): KC = 12 / 20 / 8 / 32; (10, 8): k = d = 10 < KC = 16; (50, 5): k = 10 < KC = 12 <= d; (33, 10): a one-row last block and the
# head transform in block 1; (150, 16): two 128-row chunks of KC = 32
CASES = [(30, 6), (50, 5), (10, 8), (33, 10), (65, 4), (150, 16)]
_CACHE = {}


def _fit_dict(F, mu, T=None):
    """the oracle factor in pfmi_get_fit's conventions; T: dlarft in long double rounded to double"""
    L = sr.LDFactor(F, mu)
    k = F.k
    return dict(alpha=np.array(F.alpha), B=F.B, D=F.D, qr_factors=np.asfortranarray(F.QR[:, :F.m]), V=np.asfortranarray(F.V[:k, :k]),
                T=np.asfortranarray(L.Tw.astype(np.float64) if T is None else T), mu=np.array(mu), logdet=F.logdet)


def _case(d, J):
    if (d, J) not in _CACHE:
        tg = _gauss(d, 2 + d, 3 if d > 3 else 0)
        fits, _, _ = _fits(tg, J, seed=d, maxiters=60)
        full = [ft for ft in fits if ft[1] == min(J, max(f[1] for f in fits))]
        l, j, F, mu = full[-1]
        assert F.k == min(d, 2 * j) and j >= min(J, 3)
        _CACHE[(d, J)] = (tg, F, mu, _fit_dict(F, mu))
    return _CACHE[(d, J)]


def test_wy_in_longdouble_equals_reflectors():
    """X_wy with T = dlarft(Vh, tau) in long double is the reflector product: both sum d terms per reflector in long double, so they
    agree to (d + 4 k + 16) 2^-63 S_x; the largest ratio to 2^-63 S_x is recorded"""
    for d, J in CASES:
        tg, F, mu, f = _case(d, J)
        L = sr.LDFactor(F, mu)
        U = po.randn_fill(5, d, 40)
        X, Ya = dr.wy_draws(L, L.Tw, U)
        Xr, _ = L.draws(U)
        S = np.abs(L.mu)[:, None] + L.s[:, None] * Ya
        r = (np.abs(X - Xr) / (dr.EPSLD * S)).astype(np.float64)
        mg.record(f"cpu:{d},{J}", "draws_epsld@wy_vs_refl", r, d + 4 * F.k + 16)
        assert r.max() <= d + 4 * F.k + 16, (d, J, r.max())


@pytest.mark.parametrize("d,J", CASES)
def test_double_implementations_stay_inside_the_bounds(d, J):
    """the oracle's reflector-by-reflector double (Factor.rand_and_logpdf) and the float64 statement of the lane kernel, both against
    X_wy with the lane kernel's C_x = d + 3 KC + 16; logq against d + 16"""
    tg, F, mu, f = _case(d, J)
    kc = dr.kpad_for(J)
    N, seed = 64, 77
    ref = dr.DrawRef(f, tg, seed, np.arange(N))
    U = po.randn_fill(seed, d, N)
    assert np.array_equal(U, ref.U)
    Xo, lqo = F.rand_and_logpdf(mu, U)
    Xl = dr.lane_f64(f, U, kc)
    Cx = dr.c_x("lane", d, kc)
    ro, rl = ref.x_ratio(Xo), ref.x_ratio(Xl)
    mg.record(f"cpu:{d},{J}", "draws_eps@oracle_vs_ld", ro, Cx)
    mg.record(f"cpu:{d},{J}", "draws_eps@lane_f64_vs_ld", rl, Cx)
    print(f"d={d} J={J} KC={kc}: oracle {ro.max():.2f}, lane_f64 {rl.max():.2f} of C_x = {Cx}; wy vs refl {ref.refl_ratio().max():.2f}")
    assert ro.max() <= Cx and rl.max() <= Cx, (ro.max(), rl.max(), Cx)
    rq = np.abs(lqo - ref.lq) / (EPS * ref.S_q)
    assert rq.max() <= dr.c_q("lane", d)
    rp = np.abs(tg.logp(Xl) - ref.lp) / (EPS * ref.S_p)
    assert rp.max() <= dr.c_p("lane", d, kc)
    # T rounded to double moves the draws by less than the bound too: the reflector form is inside C_x of X_wy
    assert ref.refl_ratio().max() <= Cx


def _mutation_cases(mut):
    if mut == "head_pad_rows":
        return [(50, 5)]                                   # needs k < KC <= d
    if mut == "w_last_chunk":
        return [(150, 16)]                                 # two chunks of 128 rows
    if mut == "t_offdiag_zero" or mut == "t_transposed":
        return [(30, 6), (33, 10), (150, 16)]
    return [(30, 6), (33, 10), (65, 4), (150, 16)]


@pytest.mark.parametrize("mut", dr.MUTATIONS)
def test_checker_catches_a_wrong_kernel(mut):
    """each wrong kernel exceeds C_x eps S_x by at least 100 x at some coordinate of some draw"""
    for d, J in _mutation_cases(mut):
        tg, F, mu, f = _case(d, J)
        kc = dr.kpad_for(J)
        N, seed = 64, 77
        ref = dr.DrawRef(f, None, seed, np.arange(N))
        U = po.randn_fill(seed, d, N)
        X = dr.lane_f64(f, U, kc, mut=mut, ch_rows=128, U_next=po.randn_fill(seed, d, N, 1))
        r = ref.x_ratio(X).max()
        Cx = dr.c_x("lane", d, kc)
        print(f"{mut} d={d} J={J}: {r:.3g} against C_x = {Cx}")
        assert r >= 100 * Cx, (mut, d, J, r, Cx)
        assert ref.x_ratio(dr.lane_f64(f, U, kc)).max() <= Cx


# ---- the dispatch mirror ----------------------------------------------------------------------------------------------------------
def test_writer_thresholds():
    """xw_lds_bytes: the largest resident d per KC, and the chunking of the streamed sizes of the grid"""
    assert {kc: dr.xw_max_resident_d(kc) for kc in dr.XW_KCS} == {4: 2992, 8: 1792, 12: 1264, 16: 976, 20: 800, 32: 496}
    for kc in dr.XW_KCS:
        dres = dr.xw_max_resident_d(kc)
        assert dr.xw_chunking(dres, kc)[1] == 1 and dr.xw_chunking(dres + 1, kc)[1] > 1
        assert dr.xw_lds_bytes(*dr.xw_chunking(dres + 1, kc), kc) <= dr.LDS_LIMIT
    assert dr.xw_chunking(512, 32) == (8, 4) and dr.xw_chunking(513, 32) == (8, 5)
    assert dr.xw_chunking(1281, 12) == (16, 6) and dr.xw_chunking(1536, 12) == (16, 6)
    assert dr.xw_lds_bytes(*dr.xw_chunking(100000, 32), 32) <= dr.LDS_LIMIT


def test_dispatch_routes():
    """pf_launch_elbo_draws: the route by shape, target, N and the hook"""
    P = dr.plan_for
    assert P(1000, 12, 1, 8, 1000, 64, True) == "mf:12,8,1,8:x:split"            # the pool of a built-in target, d <= 1024, J <= 8
    assert P(1000, 12, 0, 0, 1000, 64, True) == "xw:12:res:split"                 # no built-in target: the writer; 63 groups cut once (31 >= 16, 15 < 16)
    assert P(1000, 12, 0, 0, 1000, 512, True) == "xw:12:res:whole" and P(1000, 12, 0, 0, 496, 1, True) == "xw:12:res:whole"
    assert P(10000, 20, 2, 0, 160, 1, True) == "xw:20:stream:split"
    assert P(64, 12, 1, 8, 5, 30, False) == "mf:12,1,1,8:nox:whole"               # ndraws_elbo = 5
    assert P(64, 12, 1, 8, 64, 30, False) is None                                 # the scan
    assert P(2000, 12, 1, 8, 16, 30, False) is None and P(2000, 12, 1, 8, 15, 30, False) == "lane:12,1,8:rng:nox"
    assert P(50, 64, 1, 0, 100, 30, False) == "lane:64,1,0:rng:nox"               # history_length 17 .. 32: the lane kernel only
    assert P(50, 12, 1, 0, 100, 1, True, mem=True) == "lane:12,1,0:u:x"
    assert P(1000, 16, 1, 16, 100, 1, True) == "lane:16,1,16:rng:x"               # two-pass LDS exceeded: falls through
    assert not dr.mf_handles(1000, 16, 1, 0) and dr.mf_handles(688, 16, 1, 16) and not dr.mf_handles(1000, 12, 1, 16)


def test_grid_reaches_every_reachable_plan():
    """the calls of the GPU module take exactly the reachable plans; the others are excluded by name with a reason"""
    seen = dr.grid_plans()
    assert None not in seen                                                       # no grid call is a scan-only call
    missing = [nm for nm in dr.REACHABLE if nm not in seen]
    assert not missing, missing
    stray = [nm for nm in seen if nm not in dr.REACHABLE]
    assert not stray, stray
    out = [nm for nm in dr.ALL_PLANS if nm not in dr.REACHABLE]
    assert all(dr.excluded(nm) for nm in out)
    assert len(dr.ALL_PLANS) == 24 + 320 + 140 and len(out) == 32 + 14 and len(dr.EXCLUDED) == 2
    for nm in dr.ALL_PLANS:
        if nm.startswith("mf:") and dr.excluded(nm) is None:
            assert ",0,0:nox" not in nm
