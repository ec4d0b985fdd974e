"""ChEES-HMC on the device (include/pfmi.h: pfmi_chees_enqueue; csrc/chees_kernel.hip, the rule in csrc/adapt.h).  As for the device
warm-up, the main check needs no new trajectory checker: a ChEES run must be BIT-IDENTICAL to a replay of its own (step size, leapfrog
count) trace through the plain calls of static HMC, whose arithmetic tests/test_gpu_hmc_steps.py pins.  The leapfrog counts are the rule
applied to the recorded (tau, eps), exactly; the cross-chain update is checked from its recorded inputs against the long-double replay of
tests/chees_reference.py within the bound tests/test_chees_reference_cpu.py has met on the CPU.

The cases are adapt_reference.BIT_CASES' shapes: J = 2, 6 and 16 give the column paddings 4, 12 and 32, d = 20000 the streamed factor."""
import ctypes as C

import numpy as np
import pytest

import chees_reference as R
import hmc_reference as H
from helpers import demo_device_target
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON
from test_gpu_adapt import _setup

pytestmark = pytest.mark.gpu

_ROWS = ("draws", "logp", "accept_prob", "energy_error", "divergent")
_DONE = {}                         # bit-equality case -> what the later tests look at: each case runs once


PUMP_WINDOW = 4                    # PF_CHAIN_WINDOW (csrc/api_hmc.hip): rounds the pump issues ahead of the last progress word it has read


def _chees(eng, pts, x0, seeds, eps0, tau0, Lmax, W, T, pump=False, plan=None, **kw):
    """one run; with `plan` ("chees:<KPAD>:<route>", the plan its step launches are counted under) also its accounting:
      * rounds until the chains were idle = (fresh ? 1 : 0) + sum L_t;
      * no closure call is wasted: K columns per round issued, and the pump issues at most PUMP_WINDOW rounds beyond the idle one;
      * launches: one step launch per round issued (plus the opening one of a CONTINUE), and an opening launch behind every round issued
        while the last word read said "warming up".  The word says so until round r_w = 1 + sum of the warm-up's L_t, the host has read
        the word of round r - PUMP_WINDOW at the latest when it issues round r, so these are the rounds 1 .. n_w with
        r_w <= n_w <= r_w + PUMP_WINDOW - 1 (and no more than were issued)."""
    before = eng.kernel_time(plan)[1] if plan else 0
    eng.chees_enqueue(pts, x0, seeds, eps0, tau0, Lmax, W, T, **kw)
    if pump:
        for _ in range(2 + (W + T) * Lmax):
            if eng.chees_pump():
                break
            eng.sync()
    eng.chees_wait()
    got, ch = eng.hmc_get(), eng.chees_get()
    if plan:
        K, cont, nl = len(pts), bool(kw.get("cont")), ch["n_leapfrog"]
        rounds, columns = eng.chees_stats()
        issued, launches = columns // K, eng.kernel_time(plan)[1] - before
        assert rounds == (0 if cont else 1) + int(nl.sum()), (rounds, nl)
        assert columns == K * issued and rounds <= issued <= rounds + PUMP_WINDOW, (rounds, columns)
        if W == 0:
            assert launches == issued + (1 if cont else 0), (launches, issued)
        else:
            r_w = 1 + int(nl[:W].sum())
            assert r_w <= launches - issued <= min(issued, r_w + PUMP_WINDOW - 1), (launches, issued, r_w)
    return got, ch


def _same(a, b):
    return all(np.array_equal(a[q], b[q], equal_nan=True) for q in a)


def _bit_case(pfmi_mod, eng, case):
    if case in _DONE:
        return _DONE[case]
    d, J, tn, W, T = case
    kpad = H.kpad_for(J)
    route = "res" if H.resident(d, kpad) else "stream"
    pts, x0, _, seeds = _setup(pfmi_mod, eng, case)
    K, Lmax, eps0 = H.GRID_K, R.BIT_LMAX, d ** -0.25
    plan, plain = "chees:%d:%s" % (kpad, route), "hmc:%d:%s" % (kpad, route)
    before, pbefore = eng.kernel_time(plan)[1], eng.kernel_time(plain)[1]
    got, ch = _chees(eng, pts, x0, seeds, eps0, 0.0, Lmax, W, T, plan=plan, record_path=True, record_update=True)
    warm = eng.adapt_get()
    rounds, _ = eng.chees_stats()
    launches = eng.kernel_time(plan)[1] - before
    assert eng.kernel_time(plain)[1] == pbefore                          # the plain run's counter is untouched
    nl = ch["n_leapfrog"]
    assert got["draws"].shape == (d, T, K) and nl.shape == (W + T,) and np.all((1 <= nl) & (nl <= Lmax))
    # ---- the traces of pfmi_adapt_get: the shared step size in every chain, L_t, and the sampling step size
    assert np.all(warm["eps_trace"] == warm["eps_trace"][0]) and warm["eps_trace"][0, 0] == eps0 and np.all(warm["n_leapfrog"] == nl[:W])
    assert np.all(warm["step_size"] == ch["step_size"]) and np.all(warm["status"] == 0)
    assert ch["tau_trace"][0] == eps0 and np.all(ch["tau_trace"] > 0) and ch["traj_length"] > 0
    x, xp, vel = eng.chees_get_update()
    path = eng.chees_path(0, rounds)
    _, jeff, _, _ = eng.fit_status()
    Ms = [H.Metric.from_fit(eng.get_fit(int(p), int(jeff[int(p)]))) for p in pts]
    # ---- the replay through the plain calls: one transition each, all chains at the recorded step size and leapfrog count
    eps_t = np.append(warm["eps_trace"][0], [ch["step_size"]] * T)
    states = [x0.T.copy()]
    for t in range(W + T):
        eng.hmc_enqueue(pts, None if t else x0, seeds, np.full(K, eps_t[t]), int(nl[t]), 1, cont=t > 0)
        eng.hmc_wait()
        one = eng.hmc_get()
        if t < W:
            assert np.array_equal(one["accept_prob"][:, 0], warm["accept_trace"][:, t]), (case, t)
            assert np.array_equal(one["divergent"][:, 0], warm["divergent"][:, t]), (case, t)
        else:
            for q in _ROWS:
                assert np.array_equal(np.take(one[q], 0, axis=1), np.take(got[q], t - W, axis=1)), (case, t, q)
        states.append(one["draws"][:, 0, :].T.copy())
    # (the replay's launches: one per round, and the opening launch of every CONTINUE; only the plain plan's counter moved)
    assert eng.kernel_time(plain)[1] - pbefore == W + T + int(nl.sum()) and eng.kernel_time(plan)[1] - before == launches
    out = {"plan": plan, "case": case, "pts": pts, "eps0": eps0, "ch": ch, "warm": warm, "updates": (x, xp, vel), "path": path, "states": states, "Ms": Ms}
    _DONE[case] = out
    return out


@pytest.mark.parametrize("case", R.BIT_CASES, ids=[R.bit_case_id(c) for c in R.BIT_CASES])
def test_chees_run_is_bit_identical_to_its_replay_through_the_plain_calls(pfmi_mod, eng, case):
    out = _bit_case(pfmi_mod, eng, case)
    ch, warm, (d, J, tn, W, T) = out["ch"], out["warm"], case
    # the L trace is the rule applied in float64 to the recorded (tau, eps), exactly
    tau_t = np.append(ch["tau_trace"], [ch["traj_length"]] * T)
    eps_t = np.append(warm["eps_trace"][0], [ch["step_size"]] * T)
    want = [R.leapfrog(t, tau_t[t], eps_t[t], R.BIT_LMAX) for t in range(W + T)]
    assert ch["n_leapfrog"].tolist() == [w[0] for w in want]
    assert bool(ch["status"] & R.CLAMPED) == any(w[1] for w in want)


def test_both_factor_routes_and_three_paddings_ran(pfmi_mod, eng):
    ran = {_bit_case(pfmi_mod, eng, case)["plan"] for case in R.BIT_CASES}
    assert ran == {"chees:4:res", "chees:12:res", "chees:32:res", "chees:12:stream"}, ran


@pytest.mark.skipif(not HAVE_LONGDOUBLE, reason=SKIP_REASON)
@pytest.mark.parametrize("case", R.BIT_CASES, ids=[R.bit_case_id(c) for c in R.BIT_CASES])
def test_device_updates_match_the_long_double_replay(pfmi_mod, eng, case):
    out = _bit_case(pfmi_mod, eng, case)
    d, J, tn, W, T = case
    ch, warm, (x, xp, vel), (X, _, _, v), states = out["ch"], out["warm"], out["updates"], out["path"], out["states"]
    kpad = H.kpad_for(J)
    Ms = out["Ms"]
    ends = np.cumsum(ch["n_leapfrog"])                                   # the round that consumed transition t's last evaluation
    worst_u = 0.0
    for t in range(W):
        assert np.array_equal(x[t], states[t]), (case, t)                # the state the replay had before transition t
        assert np.array_equal(xp[t], X[:, :, ends[t]].T, equal_nan=True), (case, t)
        for k in range(H.GRID_K):
            vk = v[:, k, ends[t]]
            if warm["accept_trace"][k, t] == 0.0 or not np.all(np.isfinite(vk)):
                continue
            ML = Ms[k].astype(H.LD)
            err = np.abs(np.asarray(vel[t, k], dtype=H.LD) - ML.L(np.asarray(vk, dtype=H.LD)))
            bound = H.c_apply(d, kpad) * H.EPS * ML.L_abs(np.abs(np.asarray(vk, dtype=H.LD)))
            worst_u = max(worst_u, float(np.max(err / bound)))
    res = {"tau_trace": ch["tau_trace"], "eps_trace": warm["eps_trace"][0], "grad_trace": ch["grad_trace"], "n_leapfrog": ch["n_leapfrog"],
           "traj_length": ch["traj_length"], "step_size": ch["step_size"], "accept_trace": warm["accept_trace"].T, "updates": (x, xp, vel)}
    l_ok, qg, qt, qe = R.check_run(res, out["eps0"], 0.0, R.DELTA, R.BIT_LMAX)
    print("CHEES_PARITY gpu", R.bit_case_id(case), "u'", worst_u, "g", qg, "tau", qt, "eps", qe, "kept", bool(ch["status"] & R.KEPT_TRAJ))
    assert worst_u <= 1.0 and l_ok and max(qg, qt, qe) <= 1.0, (worst_u, l_ok, qg, qt, qe)


def test_drive_equality_continue_and_the_clamp(pfmi_mod, eng):
    case = (64, 6, "gauss", 6, 3)
    pts, x0, _, seeds = _setup(pfmi_mod, eng, case)
    eps0, plan = 64 ** -0.25, "chees:%d:res" % H.kpad_for(6)
    a = _chees(eng, pts, x0, seeds, eps0, 0.0, 8, 6, 3, plan=plan)
    b = _chees(eng, pts, x0, seeds, eps0, 0.0, 8, 6, 3, plan=plan)
    wa = eng.adapt_get()
    p = _chees(eng, pts, x0, seeds, eps0, 0.0, 8, 6, 3, pump=True, plan=plan)
    wp = eng.adapt_get()
    assert _same(a[0], b[0]) and _same(a[1], b[1]), "two equal runs differ"
    assert _same(a[0], p[0]) and _same(a[1], p[1]) and _same(wa, wp), "a pumped run differs from a waited one"
    # W = 0: a run and its CONTINUE are one run of the summed length; the jitter index goes on
    whole, chw = _chees(eng, pts, x0, seeds, eps0, 3 * eps0, 8, 0, 7, plan=plan)
    first, ch1 = _chees(eng, pts, x0, seeds, eps0, 3 * eps0, 8, 0, 3, plan=plan)
    second, ch2 = _chees(eng, pts, None, seeds, eps0, 3 * eps0, 8, 0, 4, plan=plan, cont=True)      # (no start round in a CONTINUE)
    for q in _ROWS:
        assert np.array_equal(np.concatenate([first[q], second[q]], axis=1), whole[q]), q
    assert chw["n_leapfrog"].tolist() == ch1["n_leapfrog"].tolist() + ch2["n_leapfrog"].tolist()
    assert chw["n_leapfrog"].tolist() == [R.leapfrog(t, 3 * eps0, eps0, 8)[0] for t in range(7)] and chw["step_size"] == eps0
    assert chw["status"] == 0 and len(chw["tau_trace"]) == 0
    # Lmax = 2: every L <= 2 and the CLAMPED bit (tau = 40 eps wants 20 steps at t = 0)
    _, chc = _chees(eng, pts, x0, seeds, eps0, 40 * eps0, 2, 0, 4, plan=plan)
    assert np.all(chc["n_leapfrog"] <= 2) and chc["n_leapfrog"][0] == 2 and chc["status"] & R.CLAMPED


def test_return_codes(pfmi_mod):
    from pfmi import _lib
    L = _lib.lib()
    d, K = 12, 2
    tg = pfmi_mod.t_diag(d, seed=3)
    e = pfmi_mod.Engine(0)
    x0 = np.asfortranarray(np.repeat(tg.mean[:, None], K, axis=1))
    seeds = np.array([1, 2], dtype=np.uint64)
    i64p, u64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)

    def enq(pts=(0, 0), x=x0, eps=0.1, tau=0.0, Lmax=4, W=3, T=2, delta=0.651, flags=0, k=K):
        pts = np.array(pts, dtype=np.int64)
        return L.pfmi_chees_enqueue(e.ctx, k, pts.ctypes.data_as(i64p), None if x is None else x.ctypes.data_as(dp), seeds.ctypes.data_as(u64p),
                                    eps, tau, Lmax, W, T, delta, flags)

    def no_chains():
        return L.pfmi_hmc_get(e.ctx, None, None, None, None, None) == -3 and L.pfmi_chees_get(e.ctx, None, None, None, None, None, None, None) == -3

    try:
        with pytest.raises(pfmi_mod.PfmiError):
            e.chees_get()
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        assert enq() == -3 and no_chains()                                              # PFMI_ERR_STATE: not fitted
        e.fit_batch(6)
        P = e.P
        for bad in (dict(Lmax=0), dict(Lmax=1025), dict(delta=0.0), dict(delta=1.0), dict(delta=np.nan), dict(tau=-1.0), dict(tau=np.inf), dict(W=-1),
                    dict(T=0), dict(flags=1), dict(flags=4), dict(flags=16), dict(k=0), dict(pts=(0, P)), dict(eps=0.0), dict(eps=np.inf), dict(x=None)):
            assert enq() == 0 and L.pfmi_chees_wait(e.ctx) == 0 and L.pfmi_hmc_get(e.ctx, None, None, None, None, None) == 0
            assert enq(**bad) == -1, bad                                                # PFMI_ERR_ARG (flags=1: CONTINUE with W > 0)
            assert no_chains(), bad                                                     # a refused call leaves no chains
        assert enq(W=2 ** 31 - 1, T=1) == -4 and no_chains()                            # PFMI_ERR_UNSUPPORTED: W + T >= 2^31
        # a staged scale (ChEES chains never carry a resident one, and a CONTINUE is on ChEES chains only)
        e.chain_scale_set(np.ones((K, d)))
        assert enq() == -4 and no_chains()
        assert L.pfmi_chees_stats(e.ctx, None, None) == -3                              # no stale figures after a refused call
        assert enq(W=0) == 0 and L.pfmi_chees_wait(e.ctx) == 0
        assert enq(W=0, x=None, flags=1) == 0 and L.pfmi_chees_wait(e.ctx) == 0         # CONTINUE on ChEES chains
        # CONTINUE across samplers: PFMI_ERR_STATE either way
        eps2 = np.array([0.1, 0.1])
        for fn, wait, param in ((L.pfmi_hmc_enqueue, L.pfmi_hmc_wait, 2), (L.pfmi_nuts_enqueue, L.pfmi_nuts_wait, 3)):
            pts = np.zeros(K, dtype=np.int64)
            head = (e.ctx, K, pts.ctypes.data_as(i64p))
            tail = (seeds.ctypes.data_as(u64p), eps2.ctypes.data_as(dp), param, 2)
            assert enq(W=0) == 0 and L.pfmi_chees_wait(e.ctx) == 0
            assert fn(*head, None, *tail, 1) == -3 and no_chains()                      # HMC / NUTS CONTINUE on ChEES chains
            assert fn(*head, x0.ctypes.data_as(dp), *tail, 0) == 0 and wait(e.ctx) == 0
            assert enq(W=0, x=None, flags=1) == -3 and no_chains()                      # ChEES CONTINUE on HMC / NUTS chains
            assert L.pfmi_chees_wait(e.ctx) == -3
        fin = C.c_int32(0)
        assert L.pfmi_chees_pump(e.ctx, C.byref(fin)) == -3 and L.pfmi_chees_get_update(e.ctx, 0, 0, None, None, None) == -3
        assert enq() == 0 and L.pfmi_chees_wait(e.ctx) == 0
        assert L.pfmi_chees_get_update(e.ctx, 0, 0, None, None, None) == -3             # no RECORD_UPDATE
        assert L.pfmi_hmc_wait(e.ctx) == -3 and L.pfmi_nuts_wait(e.ctx) == -3           # the run is pfmi_chees_wait's
        # PFMI_ERR_UNSUPPORTED, as for the plain enqueues: no gradient closure; PFMI_ERR_NUMERIC: a bad start point, reported by the wait
        e.set_target(demo_device_target(tg))
        assert enq() == -4 and b"gradient" in L.pfmi_last_error()
        e.set_target(demo_device_target(tg, grad=True))
        xbad = x0.copy()
        xbad[0, 1] = np.inf
        assert enq(x=xbad) == 0 and L.pfmi_chees_wait(e.ctx) == -5 and no_chains()
    finally:
        e.close()


def test_chains_sample_the_target(pfmi_mod, eng):
    """the sampling case of tests/test_chees_reference_cpu.py on the device: K = 256, W = 150, T = 60, Lmax = 64"""
    tg, M, x0, _, Lc = H.sampling_case(pfmi_mod)
    eng.set_target(demo_device_target(tg, grad=True))
    x = pfmi_mod.HostRNG(5).rand(tg.d).reshape(1, tg.d) * 4 - 2
    eng.optimize_batch(x, 6, 40, 1e-8)
    eng.fit_batch(6)
    assert np.array_equal(eng.get_fit(0, 0)["alpha"], np.ones(eng.d)), "the first point's fit is not the identity the CPU mirror assumes"
    X0 = np.asfortranarray(np.repeat(x0[:, None], R.SAMPLING_K, axis=1))
    got, ch = _chees(eng, [0] * R.SAMPLING_K, X0, R.sampling_seeds(pfmi_mod), tg.d ** -0.25, 0.0, R.SAMPLING_LMAX, R.SAMPLING_W, R.SAMPLING_T,
                     plan="chees:%d:res" % H.kpad_for(6))
    mean, var = H.sampling_stats(tg, Lc, got["draws"][:, -1, :])
    Ls = ch["n_leapfrog"][R.SAMPLING_W:]
    print("CHEES_SAMPLING gpu", np.max(np.abs(mean)), np.min(var), np.max(var), "accept", got["accept_prob"].mean(), "eps", ch["step_size"], "tau",
          ch["traj_length"], "mean L", Ls.mean(), "status", ch["status"])
    assert got["divergent"].sum() == 0
    assert ch["traj_length"] > ch["step_size"] and Ls.mean() >= 2
    assert H.sampling_ok(mean, var), (mean, var)


def test_public_call(pfmi_mod):
    import torch
    d = 20
    tg = pfmi_mod.t_diag(d, 1)
    m, a = torch.tensor(tg.mean, device="cuda"), torch.tensor(tg.a, device="cuda")
    e = pfmi_mod.Engine(0)
    try:
        target = pfmi_mod.TorchDeviceTarget(d, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), host=tg, grad="autograd")
        res = pfmi_mod.multipathfinder(target, 8, nruns=4, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        out = pfmi_mod.chees(res, 16, nchains=8, nwarmup=40, rng=pfmi_mod.HostRNG(8))
        assert isinstance(out, pfmi_mod.CheesResult) and isinstance(out, pfmi_mod.HMCResult) and out.nwarmup == 40 and out.max_leapfrog == 64
        assert out.draws.shape == (d, 16, 8) and np.all(np.isfinite(out.draws))
        for q in ("logp", "accept_prob", "energy_error", "divergent"):
            assert getattr(out, q).shape == (8, 16)
        assert out.n_leapfrog.shape == (16,) and np.all((1 <= out.n_leapfrog) & (out.n_leapfrog <= 64))
        assert out.step_size.shape == (8,) and np.all(out.step_size == out.step_size[0]) and out.step_size[0] != d ** -0.25
        assert out.trajectory_length >= out.step_size[0]
        assert sorted(out.warmup) == ["accept_trace", "divergent", "eps_trace", "grad_trace", "hmean_trace", "n_leapfrog", "status", "tau_trace"]
        assert out.warmup["eps_trace"].shape == (8, 40) and out.warmup["tau_trace"].shape == (40,) and np.all(out.warmup["eps_trace"][:, 0] == d ** -0.25)
        # summary() is served from the resident records while this is the engine's latest run, and gives the host copy's numbers
        runs = e.hmc_runs
        s = out.summary()
        assert e.hmc_runs == runs == out.run and s.nchains == 8 and s.ndraws == 16 and s.rhat.shape == (d,) and np.all(np.isfinite(s.mean))
        host = pfmi_mod.chain_diagnostics(out.draws, e)
        assert np.array_equal(s.mean, host["mean"]) and np.array_equal(s.ess_bulk, host["ess_bulk"])
        txt = str(out)
        assert "ChEES-HMC result" in txt and "chains: 8" in txt and "trajectory length" in txt and "(warm-up: 40)" in txt
        with pytest.raises(ValueError, match="max_leapfrog"):
            pfmi_mod.chees(res, 4, max_leapfrog=0)
        with pytest.raises(ValueError, match="auto"):
            pfmi_mod.chees(res, 4, step_size="big")
    finally:
        e.close()
