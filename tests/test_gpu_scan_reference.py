"""The single-pass ELBO scan (pathfinder.jl_amd/csrc/elbo_qf_kernel.hip) draw by draw against the extended-precision reference of
tests/scan_reference.py, at every instantiation it has, resident and streamed, and at the edges of its block, chunk, group and launch
geometry.  Every comparison is `eng.elbo_logs(p, N)` (or `eng.draws` for the n0 route) against the long-double values of the SAME fit
(the GPU's own factor, eng.get_fit), and every scan call asserts the plan it ran (pfmi_kernel_time "qf:<KC>,<TGT>,<RPAD>,<NG>:<res|
stream>:<cut>", include/pfmi.h).

Tolerances (per draw, eps = 2^-52; S_p, S_q = the reference's per-draw scales, the scan's sums with every term in absolute value):
  |lq - lq_ref| <= C_q eps S_q,  C_q = 4 nblk + 16
      |u|^2 is one fma chain per lane over its 4 rows of each of the nblk = ceil(d / 16) blocks (<= 4 nblk roundings, each at most
      eps of the partial sum, which is <= S_q), two cross-lane adds, then d log 2pi + logdet + |u|^2 and the halving (< 16).
  |lp - lp_ref| <= C_p eps S_p,  C_p = 8 nblk + 4 KC + 32
      the three row contractions (w = Vh'z, A3 = Vh'(a s^2 z), A4 = Wd'(s z)) and the scalar q12 are chains of 4 nblk MFMA / fma steps
      (4 rows per k-step, 4 k-steps per block); the per-fit constants M, v, t0, Nn, C0 are the same chains over the pseudo columns.
      Each chain errs by <= 4 nblk eps times the sum of its terms' magnitudes, and the quadratic form uses two of them per term (tv'M tv,
      tv'(A3' - v)): 8 nblk.  The finish adds KC-deep contractions (T w, M tv, Nn tv; the head transform V'u is KC-deep too): 4 KC, and
      a constant for the input roundings (c = mu - m, a s^2, 2 a c s, s) and the final adds and exp of the funnel: 32.
  These are first-order worst cases; the recorded margins (`*_eps@scan_vs_ld` rows, in units of eps S) show the headroom, and the
  `logp@scan_vs_ld` / `logq@scan_vs_ld` rows the same deviations in the contract's units, |d| / (1 + |.|) against 1e-9.
  ELBO of a fit whose N draws are all checked: mean of the per-draw bounds + N eps mean|log ratio| (any summation order); SE: the
  per-draw bounds through the sample standard deviation (Cauchy-Schwarz) + (N + 8) eps SE.

Instantiations: launch_qf picks KC in {4, 8, 12, 16, 20, 32} (2J padded), (TGT, RPAD) in {(1, 0), (1, 8), (1, 16), (2, 0)} for the
built-in targets, NG = 2 when N >= 768 and (KC <= 12 or >= 128 fits), KC <= 20.  Not covered, by name:
  * <KC, 0, 0, NG> (no target): reachable only through pf_launch_elbo_draws(with_target = false) or a target kind that is neither
    Gaussian nor funnel, and every such call site (device / host closures, pool, pfmi_draws) also writes the draws (d_x != nullptr),
    which routes them to the draw writer -- pf_launch_elbo_qf returns unhandled for a launch with d_x set.  So no TGT = 0 scan runs.
  * <32, ., ., 2>: launch_qf has no two-group instance above QF_NG2_MAXKC = 20.
"""
import os

import numpy as np
import pytest

import margins as mg
import scan_reference as sr
from scan_setup import Setup, _target, _walk  # noqa: F401  (shared with tests/test_gpu_draw_reference.py)

pytestmark = pytest.mark.gpu

EPS = sr.EPS64
KCS = (4, 8, 12, 16, 20, 32)
FAMILIES = ((1, 0), (1, 8), (1, 16), (2, 0))                    # (TGT, RPAD) of the built-in targets
CUTS = ("whole", "split", "tail-share", "tail-two")
ALL_PLANS = [f"qf:{kc},{t},{r},{ng}:{st}:{cut}" for kc in KCS for t, r in ((0, 0),) + FAMILIES for ng in (1, 2)
             for st in ("res", "stream") for cut in CUTS]
EXCLUDED = {
    "qf:<KC>,0,0,<NG>": "no target: every call site without a built-in target also writes the draws and takes the draw writer",
    "qf:32,<TGT>,<RPAD>,2": "launch_qf has no two-group instance above QF_NG2_MAXKC = 20",
}
_SEEN = set()


# ---- helpers ---------------------------------------------------------------------------------------------------
def _plans(eng):
    return {nm: eng.kernel_time(nm)[1] for nm in ALL_PLANS}


def _scan(eng, N, seeds, expect):
    """eng.elbo_batch with the plan asserted: exactly one scan call, of a plan whose name starts with `expect`"""
    before = _plans(eng)
    elbo, se, best = eng.elbo_batch(N, seeds)
    after = _plans(eng)
    delta = {k: after[k] - before[k] for k in ALL_PLANS if after[k] != before[k]}
    assert len(delta) == 1 and list(delta.values()) == [1], delta
    name = next(iter(delta))
    assert name.startswith(expect), (name, expect)
    _SEEN.add(name)
    return name, elbo, se


def _check_draws(eng, su, tg, p, N, cfg, lp, lq, idx=None, n0=0, kc=None, elbo=None, se=None):
    """lp / lq (the GPU's, over draws 0 .. N-1, or over idx) of fit p against the reference; ELBO / SE when every draw is checked"""
    kc = kc or eng_kpad(su.J)
    if idx is None:
        idx = sr.draw_subset(N, np.random.default_rng(p))
    ref = sr.scan_reference(eng, p, su.jeff[p], tg, su.seeds[p], N, n0, idx)
    lp_g, lq_g = (lp[ref.idx], lq[ref.idx]) if len(lp) == N else (lp, lq)
    nblk = (su.d + 15) // 16
    Cp, Cq = 8 * nblk + 4 * kc + 32, 4 * nblk + 16
    dp = np.abs(lp_g - ref.lp)
    dq = np.abs(lq_g - ref.lq)
    ctx = (cfg, p, int(su.jeff[p]))
    mg.check(cfg, "logp_eps@scan_vs_ld", dp / (EPS * ref.S_p), Cp, ctx=ctx)
    mg.check(cfg, "logq_eps@scan_vs_ld", dq / (EPS * ref.S_q), Cq, ctx=ctx)
    mg.record(cfg, "logp@scan_vs_ld", mg.rel(lp_g, ref.lp), float(np.max(Cp * EPS * ref.S_p / (1 + np.abs(ref.lp)))))
    mg.record(cfg, "logq@scan_vs_ld", mg.rel(lq_g, ref.lq), float(np.max(Cq * EPS * ref.S_q / (1 + np.abs(ref.lq)))))
    if ref.elbo is not None and elbo is not None:
        tn = Cp * EPS * ref.S_p + Cq * EPS * ref.S_q
        r = ref.lp - ref.lq
        te = float(np.mean(tn) + N * EPS * np.mean(np.abs(r)))
        ts = float(np.sqrt(np.sum(tn ** 2) / (N * (N - 1))) + (N + 8) * EPS * float(ref.se))
        de, ds = abs(elbo[p] - float(ref.elbo)), abs(se[p] - float(ref.se))
        mg.check(cfg, "elbo_eps@scan_vs_ld", de / te, 1.0, ctx=ctx)
        mg.check(cfg, "se_eps@scan_vs_ld", ds / ts, 1.0, ctx=ctx)
        mg.record(cfg, "elbo@scan_vs_ld", de / (1 + abs(float(ref.elbo))), te / (1 + abs(float(ref.elbo))))
        mg.record(cfg, "se@scan_vs_ld", ds / (1 + abs(float(ref.se))), ts / (1 + abs(float(ref.se))))
    return ref


def eng_kpad(J):
    return next(o for o in KCS if 2 * J <= o)


def _run_checks(eng, su, tg, N, seeds_pts, cfg, elbo, se, kc, extra=None):
    refs = []
    for p in seeds_pts:
        lp, lq = eng.elbo_logs(int(p), N)
        idx = None
        if extra is not None and extra.get(int(p)) is not None:
            idx = np.unique(np.concatenate([sr.draw_subset(N, np.random.default_rng(int(p))), extra[int(p)]]))
        refs.append(_check_draws(eng, su, tg, int(p), N, cfg, lp, lq, idx=idx, kc=kc, elbo=elbo, se=se))
    return refs


# ---- 1. every instantiation, resident and streamed ------------------------------------------------------------------
# (KC, storage) -> (J, d): odd J pads columns where 2J < KC; the streamed d end their last chunk with 2 blocks (KC 4: 162 blocks of 16),
# 1 block (KC 8: 113), a full chunk (KC 12: 80 blocks), a full chunk less one row (KC 16: d = 1023), one row past a full chunk (KC 20:
# d = 769), 2 blocks of KC 32's 8-block chunks (d = 530)
MATRIX = {(4, "res"): (1, 100), (4, "stream"): (2, 2577), (8, "res"): (3, 77), (8, "stream"): (4, 1800),
          (12, "res"): (5, 50), (12, "stream"): (6, 1280), (16, "res"): (7, 45), (16, "stream"): (8, 1023),
          (20, "res"): (9, 40), (20, "stream"): (10, 769), (32, "res"): (11, 70), (32, "stream"): (16, 530)}
_DONE = set()


def _matrix_case(pfmi, eng, kc, storage):
    if (kc, storage) in _DONE:
        return
    J, d = MATRIX[(kc, storage)]
    su = Setup(pfmi, eng, d, J, K=4, L=33, seed=kc + (7 if storage == "stream" else 0))
    assert len(su.fits) >= 128
    checks = [int(su.fits[1]), int(su.fits[-1])]                  # an early fit (j_eff < J: partial ring) and a full one
    assert su.status[checks[0]] == 0 and (su.jeff[checks[0]] < J or J <= 2)
    for tgt, rpad in FAMILIES:
        tg = _target(pfmi, tgt, rpad, su.m, su.sig, seed=kc)
        eng.set_target(tg)
        for ng, N in ((1, 100), (2, 1000)):
            if ng == 2 and kc > 20:
                continue
            cfg = f"scan:{kc},{tgt},{rpad},{ng}:{storage}"
            name, elbo, se = _scan(eng, N, su.seeds, f"qf:{kc},{tgt},{rpad},{ng}:{storage}:")
            _run_checks(eng, su, tg, N, checks, cfg, elbo, se, kc)
    _DONE.add((kc, storage))


@pytest.mark.parametrize("kc,storage", list(MATRIX))
def test_scan_instantiation_matches_longdouble(pfmi_mod, eng, kc, storage):
    """(KC, storage) x every built-in target family x NG in {1, 2}: N = 100 (one group per wave; every draw checked, ELBO and SE too)
    and N = 1000 over 132 fits (two groups per wave, also at KC = 16 / 20; 112 draws of each checked fit, the ragged last group
    among them)"""
    _matrix_case(pfmi_mod, eng, kc, storage)


# ---- 2. d edges: blocks, the ragged last block, the head transform's blocks ------------------------------------------------
@pytest.mark.parametrize("J", [4, 10])
def test_scan_d_edges(pfmi_mod, eng, J):
    """d in {1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65}: nblk = 1 .. 5 with a full or a 1-row last block, the first block
    also the last, and (J = 10, KC = 20) the second special block of the head transform as the last block or beyond d"""
    kc = eng_kpad(J)
    for d in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65):
        su = Setup(pfmi_mod, eng, d, J, K=2, L=12, seed=d)
        for tgt, rpad in ((1, 0), (2, 0)) if d > 1 else ((1, 0),):
            tg = _target(pfmi_mod, tgt, rpad, su.m, su.sig, seed=d)
            eng.set_target(tg)
            N = 65
            _, elbo, se = _scan(eng, N, su.seeds, f"qf:{kc},{tgt},{rpad},1:res:")
            _run_checks(eng, su, tg, N, sorted({int(su.ok[0]), int(su.ok[-1])}), f"scan_d:{kc},{tgt}:res", elbo, se, kc)


# ---- 3. N edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc,J", [(8, 4), (20, 10)])
def test_scan_n_edges(pfmi_mod, eng, kc, J):
    """N in {64, 65, 100, 128, 767, 768, 1000, 1009}: one / two groups per wave (768 is the switch at KC <= 12; at KC = 20 it needs
    >= 128 fits, so it stays at one here), a ragged last group, and N = 128 (8 groups + 1 pseudo group = 2 batches of 8 slots) / 1009
    (64 groups + 1 or 2 pseudo groups: 5 batches of 16) where the pseudo groups push the first batch over a batch boundary"""
    su = Setup(pfmi_mod, eng, 37, J, K=2, L=10, seed=kc)
    tg = _target(pfmi_mod, 1, 8, su.m, su.sig, seed=3)
    eng.set_target(tg)
    for N in (64, 65, 100, 128, 767, 768, 1000, 1009):
        ng = 2 if (N >= 768 and kc <= 12) else 1
        _, elbo, se = _scan(eng, N, su.seeds, f"qf:{kc},1,8,{ng}:res:")
        _run_checks(eng, su, tg, N, [int(su.fits[0]), int(su.fits[-1])], f"scan_N:{kc},1,8,{ng}:res", elbo, se, kc)


# ---- 4. launch geometry ----------------------------------------------------------------------------------------------------
def _with_hook(key, val, fn):
    old = os.environ.get(key)
    os.environ[key] = val
    try:
        return fn()
    finally:
        os.environ.pop(key, None)
        if old is not None:
            os.environ[key] = old


def test_scan_split_few_fits(pfmi_mod, eng):
    """3 fits, N = 1000: each fit cut into pieces of whole batches (split > 1), every piece recomputing the per-fit constants"""
    su = Setup(pfmi_mod, eng, 90, 4, K=1, L=3, seed=5)
    tg = _target(pfmi_mod, 1, 16, su.m, su.sig, seed=5)
    eng.set_target(tg)
    _, elbo, se = _scan(eng, 1000, su.seeds, "qf:8,1,16,2:res:split")
    for p in su.ok:
        _check_draws(eng, su, tg, int(p), 1000, "scan_geo:split", *eng.elbo_logs(int(p), 1000), idx=np.arange(1000), kc=8,
                     elbo=elbo, se=se)


@pytest.mark.parametrize("ng,K,N", [(1, 12, 200), (2, 22, 1000)])
@pytest.mark.parametrize("hook,cut", [(None, "tail-share"), ("PFMI_QF_TWO_LAUNCHES", "tail-two"), ("PFMI_QF_NO_TAIL", "whole")])
def test_scan_tail_routes(pfmi_mod, eng, hook, cut, ng, K, N):
    """more fits than the CUs and not a multiple of them, and too many to split (600 fits at N = 200, one group per wave; 1100 at
    N = 1000, two): the one-launch tail with its publishers and dependents, the two-launch cut, and one workgroup per fit -- each against
    the reference, every draw of the last two fits (hand-over pieces in the tail routes) with their ELBO / SE"""
    su = Setup(pfmi_mod, eng, 40, 3, K=K, L=50, seed=11)
    assert len(su.fits) == 50 * K
    tgt = 2 if cut == "tail-two" else 1
    tg = _target(pfmi_mod, tgt, 0, su.m, su.sig, seed=11)
    eng.set_target(tg)
    run = lambda: _scan(eng, N, su.seeds, f"qf:8,{tgt},0,{ng}:res:{cut}")
    _, elbo, se = run() if hook is None else _with_hook(hook, "1", run)
    for p in (int(su.ok[0]), int(su.fits[-2]), int(su.fits[-1])):
        _check_draws(eng, su, tg, p, N, f"scan_geo:{cut}", *eng.elbo_logs(p, N), idx=np.arange(N) if p != su.ok[0] else None,
                     kc=8, elbo=elbo, se=se)


# ---- 5. ill-scaled targets: the fold's worst case --------------------------------------------------------------------------
@pytest.mark.parametrize("kc,J", [(8, 4), (20, 10)])
def test_scan_ill_scaled_target(pfmi_mod, eng, kc, J):
    """target precisions a spanning 1e-6 .. 1e6 and a target mean shifted by up to 1e4 fit standard deviations from the fits' means:
    the draws' A3' = A3 + 2v is dominated by 2v, and the finish's A3' - v cancels most of it (|c| / s ~ 1e4)"""
    d = 60
    sig = np.exp(np.linspace(np.log(1e-3), np.log(1e3), d))             # a = 1 / sig^2: 1e6 .. 1e-6
    su = Setup(pfmi_mod, eng, d, J, K=4, L=33, seed=21, sig=sig)
    shift = sig * np.where(np.arange(d) % 2, 1e4, -3e3)
    for rpad, N, ng in ((0, 100, 1), (8, 1000, 2)):
        tg = _target(pfmi_mod, 1, rpad, su.m, su.sig, seed=21, mean_shift=shift)
        eng.set_target(tg)
        _, elbo, se = _scan(eng, N, su.seeds, f"qf:{kc},1,{rpad},{ng}:res:")
        pts = sorted({int(su.ok[0]), int(su.ok[1]), int(su.fits[-1])})
        _run_checks(eng, su, tg, N, pts, f"scan_ill:{kc},1,{rpad},{ng}", elbo, se, kc)
        f = sr.LDFactor.from_gpu(eng, pts[0], su.jeff[pts[0]])
        assert float(np.max(np.abs(f.mu - np.asarray(tg.mean, dtype=sr.LD)) / f.s)) > 1e3     # the regime this test is about


# ---- 6. writer + scan at draw offsets (pfmi_draws) ---------------------------------------------------------------------------
def test_scan_draw_offsets_writer_route(pfmi_mod, eng):
    """eng.draws(p, seed, N, n0) at J = 10 (KC = 20 > 16: the writer makes x, the scan the same draws' logp / logq) for n0 in {0, 17,
    2^32 - 5} and N in {1, 5, 16, 33}: the counter wraps to 32 bits on both sides"""
    su = Setup(pfmi_mod, eng, 41, 10, K=1, L=14, seed=31)
    for tgt, rpad in ((1, 16), (2, 0)):
        tg = _target(pfmi_mod, tgt, rpad, su.m, su.sig, seed=31)
        eng.set_target(tg)
        p = int(su.fits[-1])
        for n0 in (0, 17, 2 ** 32 - 5):
            for N in (1, 5, 16, 33):
                before = _plans(eng)
                X, lp, lq = eng.draws(p, int(su.seeds[p]), N, n0=n0)
                after = _plans(eng)
                delta = {k: after[k] - before[k] for k in ALL_PLANS if after[k] != before[k]}
                assert list(delta) == [f"qf:20,{tgt},{rpad},1:res:whole"] and list(delta.values()) == [1], delta
                _SEEN.update(delta)
                ref = _check_draws(eng, su, tg, p, N, f"scan_n0:20,{tgt},{rpad}", lp, lq, idx=np.arange(N), n0=n0, kc=20)
                xs = np.abs(np.asarray(ref.X, dtype=np.float64))
                assert np.all(np.abs(X - ref.X.astype(np.float64)) <= 1e-12 * (1 + xs))


# ---- 7. the look-up's miss path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,J", [(48, 3), (2577, 2)])
def test_scan_miss_path(pfmi_mod, eng, d, J):
    """draws whose normals fall outside the scan's LDS table (|word| < 2^12, one normal in 2^19: the fix-up pf_icdf4_fix) are found on
    the host from the Philox words and checked: at d = 48 (< 64: the look-up's front guard is the only LDS in front of the table) and
    streamed at d = 2577.  The reference counts the misses among the checked draws; at least one must be there."""
    K, L = (6, 40) if d < 64 else (2, 20)
    su = Setup(pfmi_mod, eng, d, J, K=K, L=L, seed=41)
    tg = _target(pfmi_mod, 1, 0, su.m, su.sig, seed=41)
    eng.set_target(tg)
    N = 1000
    kc = eng_kpad(J)
    _, elbo, se = _scan(eng, N, su.seeds, f"qf:{kc},1,0,2:{'res' if d < 64 else 'stream'}:")
    found = 0
    for p in su.ok:
        W = sr.philox_words(int(su.seeds[p]), np.arange(N, dtype=np.uint64)[:, None], np.arange((d + 3) // 4, dtype=np.uint64)[None, :])
        mag = (W & np.uint64(0x7FFFFFFF)).transpose(1, 2, 0).reshape(N, -1)[:, :d]
        per = np.sum(mag < sr.MISS_BELOW, axis=1)
        hit = np.nonzero(per)[0]
        if hit.size == 0:
            continue
        lp, lq = eng.elbo_logs(int(p), N)
        ref = _check_draws(eng, su, tg, int(p), N, f"scan_miss:{kc}", lp, lq, idx=hit, kc=kc)
        found += ref.misses
        if found >= 3:
            break
    assert found >= 1, "no draw with a look-up miss among the checked ones"


# ---- 8. coverage -----------------------------------------------------------------------------------------------------------
def test_scan_plan_coverage(pfmi_mod, eng):
    """every reachable (KC, TGT, RPAD, NG) x {resident, streamed} was launched by this module (the matrix cases run here if they have
    not run yet), and the geometry cuts split / tail-share / tail-two / whole each at least once; the exclusions are EXCLUDED"""
    for kc, storage in MATRIX:
        _matrix_case(pfmi_mod, eng, kc, storage)
    seen_inst = {nm.rsplit(":", 1)[0] for nm in _SEEN}
    missing = []
    for kc in KCS:
        for tgt, rpad in FAMILIES:
            for ng in ((1, 2) if kc <= 20 else (1,)):
                for st in ("res", "stream"):
                    if f"qf:{kc},{tgt},{rpad},{ng}:{st}" not in seen_inst:
                        missing.append(f"qf:{kc},{tgt},{rpad},{ng}:{st}")
    assert not missing, missing
    assert not any(nm.startswith(tuple(f"qf:{kc},0,0," for kc in KCS)) for nm in _SEEN)
    assert not any(nm.startswith("qf:32,") and ",2:" in nm for nm in _SEEN)
    cuts = {nm.rsplit(":", 1)[1] for nm in _SEEN}
    assert set(CUTS) <= cuts, cuts
    assert len(EXCLUDED) == 2
