"""The three kernels that write draws -- the streaming writer pf_elbo_xw_kernel<KC>, the two-pass MFMA kernel
pf_elbo_mfma_kernel<KC, NBW, TGT, RPAD, WX> and the lane-per-draw kernel pf_elbo_draws_kernel<KPAD, TGT, RPAD, MEM> -- coordinate by
coordinate against the extended-precision reference of tests/draw_reference.py, at every instantiation the API can reach.  Every
comparison is against the long-double values of the SAME fit (the GPU's own factor and its own T, eng.get_fit), and every call asserts
the single plan it ran by the delta of the host-side launch counters (pfmi_kernel_time "xw:..", "mf:..", "lane:..", include/pfmi.h).
The calls are draw_reference.GROUPS; tests/test_draw_reference_cpu.py proves on the CPU that they take every reachable plan, and the
last test here asserts that every one of them was launched.

What is asserted (eps = 2^-52; S_x, S_q, S_p = the reference's scales: the kernels' sums with every term in absolute value):
  |x - X_wy| <= C_x eps S_x per coordinate,  C_x = L_w + 3 KC + 16
      X_wy = mu + s . (z - Vh T Vh'z), z = [V'u_1; u_2], with the GPU's downloaded T: the operation the kernels perform.  The
      reflector-by-reflector form differs from it by the fit kernel's rounding in T; that difference is recorded (`draws_eps@wy_vs_refl`,
      bound inf), not asserted.
      L_w, the accumulation chain of w = Vh'z as read from the kernels:
        lane      d            elbo_kernels.hip: `w[j] += row[j] * zh[i]` over the KPAD head rows, then `w[j] += row[j] * z4[t]` row after
                               row through pass 1 -- one fused multiply-add per row and column, sequential in the row index
        writer    4 nblk       elbo_xw_kernel.hip body1: per 16-row block, `accw[g][T] = xw_mfma4(av[r][T], z[g][r], accw[g][T])` for
                               r = 0 .. 3 -- four v_mfma_f64_4x4x4 per block chained through the accumulator, each contracting rows
                               4 k + r (k = the lane quarter q) of the block; lane (q', c) ends with w[4 T + q'] of draw c complete: a wave
                               owns its 16 draws, there is no cross-wave or cross-lane sum, and the chunks of a streamed factor continue
                               the same accumulator.  nblk = ceil(d / 16)
        two-pass  4 NBW + 8    elbo_mfma_kernel.hip: wave wv accumulates its NBW blocks the same way (4 MFMAs per block), writes its
                               partial tile to `red`, and the 8 partial tiles are added through LDS into `wsum`
      3 KC: the head transform V'u_1, tv = T w and Vh[i, :] tv (each at most KC terms; on the MFMA kernels KC / 4 chained k-steps of
      4 terms).  16: the input roundings and the final x = fma(s, x~, mu).
      A step is counted as one eps = two unit roundoffs, so an MFMA that rounds more than once per k-step is still covered twice over.
  |lq - lq_ref| <= C_q eps S_q,  C_q = 4 nblk + 16 (writer and two-pass: the scan's chain, |u|^2 one fma per own row and block, two
      cross-lane adds, the final sum); lane: d + 16.  On the writer route lq is also BIT-equal to the scan's (elbo_logs) for the same
      (fit, seed).
  |lp - lp_ref| <= C_p eps S_p,  C_p = 8 nblk + 4 KC + 32 (two-pass kernel: x's chain plus the target's row contraction, each 4 nblk
      steps summed over waves, used twice in the quadratic form; the writer's lp is the scan's, same bound); lane: 2 d + 4 KPAD + 32
      (x's chain and the target's row sums, d each; the rank part G (Wd'e) adds RPAD <= 16 < KPAD-deep terms).
These are derived from the code, not from what the GPU returns; the recorded margins (profiles/draw_parity.md) show the headroom.
The same deviations are recorded in the contract's units (`draws@..` relative per column against 1e-10).
"""

import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import draw_reference as dr                                    # noqa: E402
import margins as mg                                           # noqa: E402
import scan_reference as sr                                    # noqa: E402
from gpu_common import _with_kernel                            # noqa: E402
from scan_setup import Setup, _target, _walk                   # noqa: E402

pytestmark = pytest.mark.gpu

EPS = dr.EPS
_SEEN = set()
_DONE = set()


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _counts(eng):
    return {nm: eng.kernel_time(nm)[1] for nm in dr.ALL_PLANS}


def _asserting(eng, expect, fn, force=None):
    """run fn (under PFMI_ELBO_KERNEL=force) and assert that exactly one draw-kernel launch happened, of plan `expect`"""
    before = _counts(eng)
    out = fn() if force is None else _with_kernel(force, fn)
    after = _counts(eng)
    delta = {k: after[k] - before[k] for k in dr.ALL_PLANS if after[k] != before[k]}
    assert delta == {expect: 1}, (delta, expect)
    _SEEN.add(expect)
    return out


def _no_target(pfmi, d):
    return pfmi.CallbackTarget(d, lambda x: 0.0, logp_batch=lambda X: np.zeros(np.asarray(X).shape[1]))


def _tg(pfmi, su, tgt, rpad, cache):
    key = (tgt, rpad)
    if key not in cache:
        cache[key] = _no_target(pfmi, su.d) if tgt == 0 else _target(pfmi, tgt, rpad, su.m, su.sig, seed=su.d + rpad)
    return cache[key]


def _kern(plan):
    return plan.split(":")[0]


def _check(plan, d, kc, ref, tg, X=None, lp=None, lq=None, ctx=None):
    """X (columns ref.idx) / lp / lq of the GPU against the reference, in units of eps S through mg.check and in the contract's units"""
    kern = _kern(plan)
    if X is not None:
        mg.check(plan, f"draws_eps@{kern}_vs_ld", ref.x_ratio(X), dr.c_x(kern, d, kc), ctx=ctx)
        mg.record(plan, f"draws@{kern}_vs_ld", ref.col_rel(X), 1e-10)
        mg.record(plan, "draws_eps@wy_vs_refl", ref.refl_ratio(), np.inf)
    if lq is not None:
        mg.check(plan, f"logq_eps@{kern}_vs_ld", np.abs(lq - ref.lq) / (EPS * ref.S_q), dr.c_q(kern, d), ctx=ctx)
        mg.record(plan, f"logq@{kern}_vs_ld", mg.rel(lq, ref.lq), 1e-9)
    if lp is not None and tg is not None and tg.kind in (0, 1):                   # a built-in target (Gaussian family, funnel)
        rlp, Sp = ref.target(tg)
        mg.check(plan, f"logp_eps@{kern}_vs_ld", np.abs(lp - rlp) / (EPS * Sp), dr.c_p(kern, d, kc), ctx=ctx)
        mg.record(plan, f"logp@{kern}_vs_ld", mg.rel(lp, rlp), 1e-9)


def _below(seed, d, draws, below):
    """normals of rows < d of the given draw counters whose Philox word magnitude is below `below`"""
    draws = np.asarray(draws, dtype=np.int64) & 0xFFFFFFFF
    ng = (d + 3) // 4
    W = sr.philox_words(seed, draws[:, None].astype(np.uint64), np.arange(ng, dtype=np.uint64)[None, :])
    mag = (W & np.uint64(0x7FFFFFFF)).transpose(1, 2, 0).reshape(len(draws), 4 * ng)[:, :d]
    return np.sum(mag < below, axis=1)


class _Refs:
    """the references of one fitted setup, cached by (point, N, n0, host normals or not)"""

    def __init__(self, eng, su):
        self.eng, self.su, self.fits, self.refs = eng, su, {}, {}

    def fit(self, p):
        if p not in self.fits:
            self.fits[p] = self.eng.get_fit(p, int(self.su.jeff[p]))
        return self.fits[p]

    def ref(self, p, N, n0=0, U=None):
        """draws draw_subset(N) of fit p (host normals U: not cached, they are fresh per call)"""
        idx = sr.draw_subset(N, np.random.default_rng(p))
        if U is not None:
            return dr.DrawRef(self.fit(p), None, 0, idx, 0, U)
        key = (p, N, n0)
        if key not in self.refs:
            self.refs[key] = dr.DrawRef(self.fit(p), None, int(self.su.seeds[p]), idx, n0)
        return self.refs[key]


def _run_calls(pfmi, eng, fit, calls, seed=1):
    """fit the setup, make every call with its plan asserted, compare with the reference; returns the setup"""
    su = Setup(pfmi, eng, fit.d, fit.J, fit.K, fit.L, seed=seed)
    assert len(su.fits) == fit.K * fit.L and eng.P == fit.K * (fit.L + 1)
    kc = dr.kpad_for(fit.J)
    refs, tcache = _Refs(eng, su), {}
    pts = sorted({int(su.ok[0]), int(su.fits[-1])})                # an early fit (j_eff = 1: k = 2 < KC) and a full one
    assert su.jeff[pts[-1]] == min(fit.J, fit.L) and su.status[pts[-1]] == 0
    rng = np.random.default_rng(fit.d + 7 * fit.J)
    for c in calls:
        plan = dr.call_plan(fit, c)
        tg = _tg(pfmi, su, c.tgt, c.rpad, tcache)
        eng.set_target(tg)
        ctx = (fit, c)
        if c.route == "draws":
            for p in pts:
                U = rng.normal(size=(fit.d, c.N)) if c.mem else None
                X, lp, lq = _asserting(eng, plan, lambda: eng.draws(p, int(su.seeds[p]), c.N, n0=c.n0, u=U), c.force)
                ref = refs.ref(p, c.N, c.n0, U)
                _check(plan, fit.d, kc, ref, tg, X[:, ref.idx], lp[ref.idx], lq[ref.idx], ctx=ctx + (p,))
        elif c.route == "batch":
            Uall = rng.normal(size=(eng.P, c.N, fit.d)) if c.mem else None
            _asserting(eng, plan, lambda: eng.elbo_batch(c.N, su.seeds, u=Uall), c.force)
            for p in pts:
                lp, lq = eng.elbo_logs(p, c.N)
                ref = refs.ref(p, c.N, 0, Uall[p].T if c.mem else None)
                _check(plan, fit.d, kc, ref, tg, None, lp[ref.idx], lq[ref.idx], ctx=ctx + (p,))
        else:
            pool_pts = [int(su.offsets[k + 1]) - 1 for k in range(fit.K)]
            _asserting(eng, plan, lambda: eng.pool_build(c.N, pool_pts, su.seeds[pool_pts]), c.force)
            Xp, lr = eng.pool_get()
            for k, p in enumerate(pool_pts):
                ref = refs.ref(p, c.N)
                _check(plan, fit.d, kc, ref, tg, Xp[:, ref.idx, k], ctx=ctx + (p,))
                rlp, Sp = ref.target(tg)
                tol = dr.c_p(_kern(plan), fit.d, kc) * EPS * Sp + dr.c_q(_kern(plan), fit.d) * EPS * ref.S_q
                assert np.all(np.abs(lr[k * c.N:(k + 1) * c.N][ref.idx] - (rlp - ref.lq)) <= tol)
    return su, refs, tcache


def _group_case(pfmi, eng, group, i):
    if (group, i) in _DONE:
        return
    fit, calls = dr.GROUPS[group]()[i]
    _run_calls(pfmi, eng, fit, calls, seed=1 + i)
    _DONE.add((group, i))


def _ids(group):
    return [f"d{f.d}-J{f.J}" for f, _ in dr.GROUPS[group]()]


# ---- 1. the writer: every KC, resident and streamed -------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(dr.writer_matrix())), ids=_ids("writer_matrix"))
def test_writer_every_kc_resident_and_streamed(pfmi_mod, eng, i):
    """KC in {4 .. 32} at the largest resident d and the smallest streamed one (xw_lds_bytes), KC = 32 at d = 512 (four full 128-row
    chunks) and 513 (a one-row last chunk), KC = 12 at d = 1281 and 1536: the pure writer (no built-in target) at N = 100 (whole) and
    N = 512 (split), and the writer-then-scan pair on a Gaussian target, whose logq is also bit-equal to the scan's own"""
    fit, calls = dr.writer_matrix()[i]
    if ("writer_matrix", i) in _DONE:
        return
    su, refs, tcache = _run_calls(pfmi_mod, eng, fit, calls, seed=1 + i)
    _DONE.add(("writer_matrix", i))
    kc = dr.kpad_for(fit.J)
    st = "stream" if dr.xw_chunking(fit.d, kc)[1] > 1 else "res"
    assert {f"xw:{kc}:{st}:whole", f"xw:{kc}:{st}:split"} <= _SEEN
    eng.set_target(tcache[(1, 0)])
    eng.elbo_batch(100, su.seeds)                              # N >= 64: the single-pass scan
    p = int(su.fits[-1])
    _, lq_scan = eng.elbo_logs(p, 100)
    c = calls[1]
    _, _, lq = _with_kernel(c.force, lambda: eng.draws(p, int(su.seeds[p]), 100)) if c.force else eng.draws(p, int(su.seeds[p]), 100)
    np.testing.assert_array_equal(lq, lq_scan)


# ---- 2. the writer: d edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(dr.writer_d_edges())), ids=_ids("writer_d_edges"))
def test_writer_d_edges(pfmi_mod, eng, i):
    """KC = 12 / 20 at d in {1, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 65}, KC = 32 at d = 31 / 33: k = d < KC, the head transform
    spilling into block 1 (KC > 16) with block 1 the last block or beyond d, one-row last blocks"""
    _group_case(pfmi_mod, eng, "writer_d_edges", i)


# ---- 3. the writer: N, offset and cut edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(dr.writer_n_edges())), ids=_ids("writer_n_edges"))
def test_writer_bits_do_not_depend_on_n_offset_cut_or_route(pfmi_mod, eng, i):
    """KC = 8 / 20: N in {1, 15, 16, 17, 255, 256, 257, 512, 1000} (512 and 1000 reach `split`) x n0 in {0, 53, 2^32 - 5}: every draw
    is the same bits as in ONE base run of 1100 draws (checked against the reference, every draw), whatever N, n0 and the cut; the
    counter wraps at 2^32; pool_build gives the same bits as pfmi_draws"""
    fit, calls = dr.writer_n_edges()[i]
    su = Setup(pfmi_mod, eng, fit.d, fit.J, fit.K, fit.L, seed=3 + i)
    kc = dr.kpad_for(fit.J)
    tg = _no_target(pfmi_mod, fit.d)
    eng.set_target(tg)
    p = int(su.fits[-1])
    seed = int(su.seeds[p])
    f = eng.get_fit(p, int(su.jeff[p]))
    NB = 1100
    base_plan = dr.plan_for(fit.d, kc, 0, 0, NB, 1, True)
    Xb, _, lqb = _asserting(eng, base_plan, lambda: eng.draws(p, seed, NB))
    _check(base_plan, fit.d, kc, dr.DrawRef(f, None, seed, np.arange(NB)), None, Xb, None, lqb)
    for c in calls:
        plan = dr.call_plan(fit, c)
        X, _, lq = _asserting(eng, plan, lambda: eng.draws(p, seed, c.N, n0=c.n0))
        if c.n0 < 2 ** 31:
            np.testing.assert_array_equal(X, Xb[:, c.n0:c.n0 + c.N])
            np.testing.assert_array_equal(lq, lqb[c.n0:c.n0 + c.N])
        else:
            w = 2 ** 32 - c.n0                                 # draws before the wrap: against the reference; after it: the base run
            ref = dr.DrawRef(f, None, seed, np.arange(min(w, c.N)), c.n0)
            _check(plan, fit.d, kc, ref, None, X[:, :w], None, lq[:w], ctx=c)
            np.testing.assert_array_equal(X[:, w:], Xb[:, :max(c.N - w, 0)])
            np.testing.assert_array_equal(lq[w:], lqb[:max(c.N - w, 0)])
    pp = [int(su.offsets[1]) - 1]
    assert pp[0] == p
    for N_r in (17, 100):
        _asserting(eng, dr.plan_for(fit.d, kc, 0, 0, N_r, 1, True), lambda: eng.pool_build(N_r, pp, su.seeds[pp]))
        Xp, _ = eng.pool_get()
        np.testing.assert_array_equal(Xp[:, :, 0], Xb[:, :N_r])
    _DONE.add(("writer_n_edges", i))


# ---- 4. the pool route --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,tgt,rpad", [(4, 1, 8), (4, 0, 0), (10, 1, 0)])
def test_pool_route_with_a_failed_fit(pfmi_mod, eng, J, tgt, rpad):
    """pool_build of K = 3 fits at N_r = 17 and 100, the middle one failed (its log ratios are NaN, its draws do not exist): every column
    of the good fits against the reference -- the two-pass kernel (KC = 8, rank-8 Gaussian), the pure writer (no built-in target) and
    the writer-then-scan pair (KC = 20)"""
    d, L = 40, 8
    rng = np.random.default_rng(5)
    m, sig = rng.normal(size=d), np.exp(rng.uniform(-0.7, 0.7, d))
    th, gr = _walk(pfmi_mod, m, sig, 2, L, 9)
    bad_th, bad_gr = np.cumsum(rng.normal(size=(L + 1, d)), 0), rng.normal(size=(L + 1, d))
    eng.set_target(pfmi_mod.GaussTarget(m, sig ** 2))
    eng.set_traces([th[0], bad_th, th[1]], [gr[0], bad_gr, gr[1]])
    eng.fit_batch(J, -1e300)
    status, jeff, _, _ = eng.fit_status()
    off = np.asarray(eng.offsets)
    bad = [p for p in range(int(off[1]) + 1, int(off[2])) if status[p] != 0]
    assert bad, status
    pts = [int(off[1]) - 1, bad[0], int(off[3]) - 1]
    assert status[pts[0]] == 0 and status[pts[2]] == 0
    seeds = np.array([sr.po.rand_u64(21, p, 9) for p in pts], dtype=np.uint64)
    kc = dr.kpad_for(J)
    tg = _no_target(pfmi_mod, d) if tgt == 0 else _target(pfmi_mod, tgt, rpad, m, sig, seed=4)
    eng.set_target(tg)
    for N_r in (17, 100):
        plan = dr.plan_for(d, kc, tgt, rpad, N_r, 3, True)
        _asserting(eng, plan, lambda: eng.pool_build(N_r, pts, seeds))
        X, lr = eng.pool_get()
        assert np.all(np.isnan(lr[N_r:2 * N_r]))
        for k in (0, 2):
            f = eng.get_fit(pts[k], int(jeff[pts[k]]))
            ref = dr.DrawRef(f, None, int(seeds[k]), np.arange(N_r))
            _check(plan, d, kc, ref, None, X[:, :, k], ctx=(J, tgt, N_r, k))
            Xd, lp, lq = eng.draws(pts[k], int(seeds[k]), N_r)
            np.testing.assert_array_equal(X[:, :, k], Xd)
            np.testing.assert_array_equal(lr[k * N_r:(k + 1) * N_r], lp - lq)
            _check(plan, d, kc, ref, tg, None, lp, lq, ctx=(J, tgt, N_r, k))


# ---- 5. the two-pass kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(dr.mf_matrix())), ids=_ids("mf_matrix"))
def test_two_pass_every_kc_nbw_family(pfmi_mod, eng, i):
    """KC in {4, 8, 12, 16} x d in {113, 250, 500, 1000} (NBW = 1, 2, 4, 8) x the five target families, draws written (pfmi_draws,
    N = 100: split, N = 16: whole) and not (pfmi_elbo_batch, N = 48 < 64: split, N = 5: whole).  At d = 1000 the factor block of
    KC = 16 (and of KC = 12 with a rank-16 target) exceeds the kernel's LDS and the call falls through to the lane kernel, as
    draw_reference.call_plan says; those KC reach NBW = 8 at the largest d where every family fits (912, 688).  The d = 1000 cases
    must contain look-up misses: the kernel keeps 12 binades of the table in LDS, words below 2^19 take the global-table path."""
    fit, calls = dr.mf_matrix()[i]
    if ("mf_matrix", i) not in _DONE:
        su, _, _ = _run_calls(pfmi_mod, eng, fit, calls, seed=1 + i)
        _DONE.add(("mf_matrix", i))
        if fit.d == 1000:
            p = int(su.fits[-1])
            if any(dr.call_plan(fit, c).startswith("mf:") for c in calls):
                assert _below(int(su.seeds[p]), fit.d, np.arange(100), 1 << 19).sum() >= 1


@pytest.mark.parametrize("i", range(len(dr.mf_edges())), ids=_ids("mf_edges"))
def test_two_pass_nbw_boundaries_and_n_edges(pfmi_mod, eng, i):
    """d = 128 / 129, 256 / 257, 512 / 513, 1024 (the NBW switches and the kernel's last d) x N in {5, 16, 17, 48}, draws written and
    not, and a pool of N_r = 1000 (63 groups cut over many workgroups)"""
    _group_case(pfmi_mod, eng, "mf_edges", i)


# ---- 6. the lane kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(dr.lane_matrix())), ids=_ids("lane_matrix"))
def test_lane_every_kpad_family_and_source(pfmi_mod, eng, i):
    """KPAD in {4 .. 64} x {host normals, in-kernel generator} x {draws written, not}: the five families at d = 50, the rank-0 Gaussian
    at d = 257, and N = 257 (two blocks of 256 threads)"""
    _group_case(pfmi_mod, eng, "lane_matrix", i)


@pytest.mark.parametrize("i", range(len(dr.lane_d_edges())), ids=_ids("lane_d_edges"))
def test_lane_d_edges(pfmi_mod, eng, i):
    """d in {1, 3, KPAD - 1, KPAD, KPAD + 1} for every KPAD: head rows beyond d, k = d < KPAD, the first row after the head"""
    _group_case(pfmi_mod, eng, "lane_d_edges", i)


# ---- 7. the writer's miss path ----------------------------------------------------------------------------------------------------------
def test_writer_miss_path(pfmi_mod, eng):
    """the writer keeps all 19 binades in LDS: only words below 2^12 (one normal in 2^19) take the fix-up.  Draws with such a word are
    found on the host from the Philox words and checked; at least one must be there."""
    d, J, N = 600, 4, 1000
    su = Setup(pfmi_mod, eng, d, J, 2, 6, seed=41)
    eng.set_target(_no_target(pfmi_mod, d))
    found = 0
    plan = dr.plan_for(d, 8, 0, 0, N, 1, True)
    for p in su.ok:
        seed = int(su.seeds[p])
        hit = np.nonzero(_below(seed, d, np.arange(N), sr.MISS_BELOW))[0]
        if hit.size == 0:
            continue
        X, _, lq = _asserting(eng, plan, lambda: eng.draws(int(p), seed, N))
        ref = dr.DrawRef(eng.get_fit(int(p), int(su.jeff[p])), None, seed, hit)
        _check(plan, d, 8, ref, None, X[:, hit], None, lq[hit], ctx=("miss", int(p)))
        found += int(hit.size)
        if found >= 3:
            break
    assert found >= 1, "no draw with a look-up miss among the checked ones"


# ---- 8. the hook the forced routes above depend on ---------------------------------------------------------------------------------------
def test_unsetting_a_hook_returns_it_to_the_environment(pfmi_mod, eng):
    """pfmi_debug_set(key, NULL) after a set: PFMI_ELBO_KERNEL from the environment selects the kernel again.  (An unset used to leave an
    entry that hid the environment for the rest of the process: in a whole-suite run, after tests/test_gpu_abi.py had set and unset the
    hook, every later `_with_kernel` ran the default route -- the plan assertions of this module are what showed it.)"""
    L = pfmi_mod.lib()
    su = Setup(pfmi_mod, eng, 40, 4, 1, 6, seed=2)
    eng.set_target(_target(pfmi_mod, 1, 0, su.m, su.sig, seed=2))
    p = int(su.fits[-1])
    run = lambda: eng.draws(p, int(su.seeds[p]), 20)
    assert L.pfmi_debug_set(b"PFMI_ELBO_KERNEL", b"lane") == 0
    try:
        _asserting(eng, "lane:8,1,0:rng:x", run)
    finally:
        assert L.pfmi_debug_set(b"PFMI_ELBO_KERNEL", None) == 0
    _asserting(eng, "mf:8,1,1,0:x:split", run)
    _asserting(eng, "xw:8:res:whole", run, force="xw")
    _asserting(eng, "lane:8,1,0:rng:x", run, force="lane")


# ---- 9. coverage ------------------------------------------------------------------------------------------------------------------------
def test_draw_plan_coverage(pfmi_mod, eng):
    """every reachable plan of the CPU mirror was launched by this module (the grid cases run here if they have not run yet); the
    excluded ones never were"""
    for group, make in dr.GROUPS.items():
        if group == "writer_n_edges":
            continue                                           # its plans are among the writer matrix's
        for i in range(len(make())):
            _group_case(pfmi_mod, eng, group, i)
    missing = [nm for nm in dr.REACHABLE if nm not in _SEEN]
    assert not missing, missing
    assert not [nm for nm in _SEEN if dr.excluded(nm)]
    counts = _counts(eng)
    assert not [nm for nm in dr.ALL_PLANS if dr.excluded(nm) and counts[nm]]
