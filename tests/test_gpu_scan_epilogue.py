"""The per-batch draw finish of the ELBO scan (pathfinder.jl_amd/csrc/elbo_qf_kernel.hip, the section "finish the 16 draws of each group
in registers") draw by draw against the extended-precision reference of tests/scan_reference.py.  The finish reads the A operands of
T, M, Nn and G once per batch and runs the chains of a wave's groups in lockstep (T w; M tv with Nn tv; G tt); what can go wrong there
is an operand tile read under the wrong predicate, a group finished with the other group's vector, or a store for a group that has no
draws.  Tolerances are those of tests/test_gpu_scan_reference.py (per draw, C_p = 8 nblk + 4 KC + 32 and C_q = 4 nblk + 16 in units of
eps S): any of these moves logp by O(1).

  KC in {4, 8, 12, 16, 20, 32} (J = 2, 4, 6, 8, 10, 16)   every operand tile count; KC > 16 has two row tiles, KC = 32 one group only
  d in {5, 17, 48}                                     one block; first + last; first + interior + last
  targets                                              rank-8 and rank-16 Gaussian (RPAD 8, 16), diagonal Gaussian, funnel (RPAD 0)
  N = 100, 771                                         one group per wave; two (KC <= 12): 48 full groups + 3 draws, the store guard
  KC in {16, 20} with 132 fits, N = 771                two groups per wave in the register-lean body
  N = 1000 at d = 17                                   64 slots: the pseudo group's partner in wave 0, every slot of the last batch used
  a failed fit among good ones                         NaN rows, the good fits against the reference
Route identity: 300 fits at d = 17, N = 771, rank-8: tables, ELBOs and standard errors bit for bit the same on the default cut, with
PFMI_QF_NO_TAIL = 1 and with PFMI_QF_TWO_LAUNCHES = 1 (at 300 fits all three are the plan "split", see the test).
"""
import types

import numpy as np
import pytest

import scan_reference as sr
import test_gpu_scan_reference as base
from scan_setup import _walk
from test_gpu_scan_first_batch import _gauss
from test_gpu_scan_philox_hoist import HOOKS, _edge_seeds, _tables

pytestmark = pytest.mark.gpu

J_OF = {4: 2, 8: 4, 12: 6, 16: 8, 20: 10, 32: 16}


def _targets(pfmi, su, seed):
    return ((_gauss(pfmi, su, 8, seed), 1, 8), (_gauss(pfmi, su, 16, seed), 1, 16), (_gauss(pfmi, su, 0, seed), 1, 0),
            (pfmi.FunnelTarget(su.d), 2, 0))


def _ng(N, kc, nfits):
    return 2 if (N >= 768 and kc <= 20 and (kc <= 12 or nfits >= 128)) else 1


@pytest.mark.parametrize("kc", sorted(J_OF))
def test_finish_every_tile_count(pfmi_mod, eng, kc):
    J = J_OF[kc]
    assert base.eng_kpad(J) == kc
    for d in (5, 17, 48):
        su = base.Setup(pfmi_mod, eng, d, J, K=3, L=7, seed=11 * d + J)
        picks = sorted({int(su.ok[0]), int(su.ok[-1])})              # a partial ring and a full history
        for tg, tgt, rpad in _targets(pfmi_mod, su, d):
            eng.set_target(tg)
            for N in (771, 100):
                ng = _ng(N, kc, len(su.fits))
                _, elbo, se = base._scan(eng, N, su.seeds, f"qf:{kc},{tgt},{rpad},{ng}:res:")
                base._run_checks(eng, su, tg, N, picks, f"scan_epi:{kc},{tgt},{rpad},{ng}", elbo, se, kc)


@pytest.mark.parametrize("kc", [16, 20])
def test_finish_two_groups_register_lean_body(pfmi_mod, eng, kc):
    """132 fits: two groups per wave at KC = 16 and 20 (two row tiles at 20), N = 771"""
    J, N = J_OF[kc], 771
    su = base.Setup(pfmi_mod, eng, 17, J, K=4, L=33, seed=kc + 5)
    assert len(su.fits) >= 128
    picks = [int(su.fits[1]), int(su.fits[-1])]
    for tg, tgt, rpad in _targets(pfmi_mod, su, kc):
        eng.set_target(tg)
        _, elbo, se = base._scan(eng, N, su.seeds, f"qf:{kc},{tgt},{rpad},2:res:")
        base._run_checks(eng, su, tg, N, picks, f"scan_epi_lean:{kc},{tgt},{rpad},2", elbo, se, kc)


def test_finish_full_last_batch(pfmi_mod, eng):
    """N = 1000 at d = 17: 63 groups (the last with 8 draws) + the pseudo group fill 4 batches of 16 slots; every draw checked"""
    kc, N = 12, 1000
    su = base.Setup(pfmi_mod, eng, 17, 6, K=3, L=7, seed=61)
    for tg, tgt, rpad in _targets(pfmi_mod, su, 3)[:1] + _targets(pfmi_mod, su, 3)[3:]:
        eng.set_target(tg)
        _, elbo, se = base._scan(eng, N, su.seeds, f"qf:{kc},{tgt},{rpad},2:res:")
        p = int(su.ok[-1])
        base._check_draws(eng, su, tg, p, N, f"scan_epi_full:{kc},{tgt},{rpad},2", *eng.elbo_logs(p, N), idx=np.arange(N), kc=kc,
                          elbo=elbo, se=se)


def test_finish_with_a_failed_fit(pfmi_mod, eng):
    """three paths, the middle one a random walk with random gradients (its fits fail): NaN rows and NaN ELBOs for the failed fits, the
    good fits on either side against the reference"""
    d, L, J, kc, N = 17, 8, 6, 12, 771
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
    good = [int(off[1]) - 1, int(off[3]) - 1]
    assert bad and all(status[p] == 0 for p in good), status
    seeds = np.array([sr.po.rand_u64(23, p, 9) for p in range(eng.P)], dtype=np.uint64)
    su = types.SimpleNamespace(m=m, sig=sig, d=d, J=J, jeff=jeff, seeds=seeds)
    tg = _gauss(pfmi_mod, su, 8, 2)
    eng.set_target(tg)
    _, elbo, se = base._scan(eng, N, seeds, f"qf:{kc},1,8,2:res:")
    for p in bad:
        lp, lq = eng.elbo_logs(int(p), N)
        assert np.all(np.isnan(lp)) and np.all(np.isnan(lq)) and np.isnan(elbo[p])
    base._run_checks(eng, su, tg, N, good, f"scan_epi_failed:{kc},1,8,2", elbo, se, kc)


def test_finish_same_bits_on_every_tail_route(pfmi_mod, eng):
    """300 fits at d = 17, N = 771, rank-8 target, under the default cut and both hooks: the same tables, ELBOs and standard errors, bit
    for bit.  The launch code cuts a fit in two while 2 x fits < 1024 and each piece keeps a full batch ((49 + 1) / 2 >= 16 slots), so
    at 300 fits every one of the three runs is the plan "split" -- two pieces per fit, the second starting at a batch boundary with a
    pseudo group of its own -- and the tail hooks, which act on whole fits only, must change nothing.  (The tail routes proper, from
    1024 fits on, are compared in tests/test_gpu_scan_first_batch.py and tests/test_gpu_scan_philox_hoist.py at 1100 fits.)"""
    J, kc, N = 6, 12, 771
    su = base.Setup(pfmi_mod, eng, 17, J, K=6, L=50, seed=37)
    assert len(su.fits) == 300
    su.seeds, picks = _edge_seeds(su)
    picks = picks + [int(su.fits[-1])]
    eng.set_target(_gauss(pfmi_mod, su, 8, 13))
    got = {}
    for hook in HOOKS:
        run = lambda: base._scan(eng, N, su.seeds, f"qf:{kc},1,8,2:res:split")
        _, elbo, se = run() if hook is None else base._with_hook(hook, "1", run)
        got[hook] = (_tables(eng, picks, N), elbo.copy(), se.copy())
    for hook in HOOKS[1:]:
        for a, b in zip(got[None][0], got[hook][0]):
            assert np.array_equal(a, b, equal_nan=True), hook
        assert np.array_equal(got[None][1], got[hook][1], equal_nan=True), hook
        assert np.array_equal(got[None][2], got[hook][2], equal_nan=True), hook
