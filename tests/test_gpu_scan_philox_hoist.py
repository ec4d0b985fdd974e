"""The ELBO scan's hoisted generator call (per-draw Philox rounds formed once per batch, pathfinder.jl_amd/csrc/elbo_qf_kernel.hip) draw
by draw against the extended-precision reference of tests/scan_reference.py, at the shapes where the hoist can go wrong:

  d in {5, 17, 48}    one block; first + last; first + interior + last (the interior loop is where the hoisted call runs)
  N = 771             two 16-draw groups per wave (KC <= 12), a partial last group; N = 100: one group per wave
  J in {2, 6, 10}     KC = 4, 12, 20
  targets             low-rank r = 8, diagonal, funnel
  seeds               per fit, among them 0, 2^32 - 1 in either half and 2^64 - 1 (key words 0 and all-ones: the round keys k + j W)

Tolerances are those of tests/test_gpu_scan_reference.py (per draw, C_p = 8 nblk + 4 KC + 32 and C_q = 4 nblk + 16 in units of
eps S): a wrong Philox word moves a normal, and with it logq, by O(1).  The log-density tables of the same fits are also bit-identical
between the default cut, PFMI_QF_NO_TAIL = 1 and PFMI_QF_TWO_LAUNCHES = 1 -- for the short paths, and for 1100 fits, where the tail
routes (publishers, dependents, second launch) are the ones that run.
"""
import numpy as np
import pytest

import scan_reference as sr
import test_gpu_scan_reference as base

pytestmark = pytest.mark.gpu

EDGE_SEEDS = [0, 0xFFFFFFFF, 0xFFFFFFFF00000000, 0xFFFFFFFFFFFFFFFF, 0x00000001FFFFFFFF, 0x8000000080000000]
HOOKS = (None, "PFMI_QF_NO_TAIL", "PFMI_QF_TWO_LAUNCHES")


def _edge_seeds(su):
    """the fixture's seeds with the edge values on the last fits (full history) and the first ones (partial ring)"""
    seeds = su.seeds.copy()
    ok = [int(p) for p in su.ok]
    picks = ok[-3:] + ok[:3]
    for p, s in zip(picks, EDGE_SEEDS):
        seeds[p] = np.uint64(s)
    return seeds, picks


def _target(pfmi, kind, su):
    if kind == "funnel":
        return pfmi.FunnelTarget(su.d), 2, 0
    if kind == "diag":
        return pfmi.GaussTarget(su.m, su.sig ** 2, None, offset=1.25), 1, 0
    W = 0.3 * np.random.default_rng(su.d).normal(size=(su.d, 8))
    return pfmi.GaussTarget(su.m, su.sig ** 2, W, offset=-0.5), 1, 8


def _tables(eng, pts, N):
    return [np.stack(eng.elbo_logs(p, N)) for p in pts]


@pytest.mark.parametrize("J", [2, 6, 10])
@pytest.mark.parametrize("d", [5, 17, 48])
def test_hoisted_scan_matches_longdouble(pfmi_mod, eng, d, J):
    kc = base.eng_kpad(J)
    su = base.Setup(pfmi_mod, eng, d, J, K=3, L=7, seed=3 * d + J)
    su.seeds, picks = _edge_seeds(su)
    for kind in ("lowrank", "diag", "funnel"):
        tg, tgt, rpad = _target(pfmi_mod, kind, su)
        eng.set_target(tg)
        for N in (771, 100):
            ng = 2 if (N >= 768 and kc <= 12) else 1
            plan = f"qf:{kc},{tgt},{rpad},{ng}:res:"
            _, elbo, se = base._scan(eng, N, su.seeds, plan)
            base._run_checks(eng, su, tg, N, picks, f"scan_philox:{kc},{tgt},{rpad},{ng}", elbo, se, kc)
            ref = _tables(eng, picks, N)
            for hook in HOOKS[1:]:
                base._with_hook(hook, "1", lambda: base._scan(eng, N, su.seeds, plan))
                for a, b in zip(ref, _tables(eng, picks, N)):
                    assert np.array_equal(a, b, equal_nan=True), (kind, N, hook)


@pytest.mark.parametrize("kind,J", [("lowrank", 6), ("funnel", 2)])
def test_hoisted_scan_same_bits_on_every_tail_route(pfmi_mod, eng, kind, J):
    """1100 fits at d = 17, N = 771: more fits than CUs, so the default cut ends in the one-launch tail (a publisher and its dependents per
    fit), the hooks give the two-launch tail and one workgroup per fit.  Same seeds, same fits: the same tables, bit for bit, and the
    last fit (a tail fit, edge seed) against the reference."""
    kc = base.eng_kpad(J)
    su = base.Setup(pfmi_mod, eng, 17, J, K=22, L=50, seed=17 + J)
    su.seeds, picks = _edge_seeds(su)
    tg, tgt, rpad = _target(pfmi_mod, kind, su)
    eng.set_target(tg)
    N = 771
    got = {}
    for hook, cut in zip(HOOKS, ("tail-share", "whole", "tail-two")):
        run = lambda: base._scan(eng, N, su.seeds, f"qf:{kc},{tgt},{rpad},2:res:{cut}")
        _, elbo, se = run() if hook is None else base._with_hook(hook, "1", run)
        got[cut] = (_tables(eng, picks, N), elbo.copy(), se.copy())
        if hook is None:
            p = picks[0]
            base._check_draws(eng, su, tg, p, N, f"scan_philox_tail:{kc},{tgt},{rpad}", *eng.elbo_logs(p, N), idx=np.arange(N), kc=kc,
                              elbo=elbo, se=se)
    for cut in ("whole", "tail-two"):
        for a, b in zip(got["tail-share"][0], got[cut][0]):
            assert np.array_equal(a, b, equal_nan=True), cut
        assert np.array_equal(got["tail-share"][1], got[cut][1], equal_nan=True), cut
        assert np.array_equal(got["tail-share"][2], got[cut][2], equal_nan=True), cut
