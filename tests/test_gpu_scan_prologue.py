"""The ELBO scan's pseudo group with the c/s column loaded in one flight (`pseudo_cols`, pathfinder.jl_amd/csrc/elbo_qf_kernel.hip) draw by
draw against the extended-precision reference of tests/scan_reference.py.  The column yields the per-fit constants v, t0 and C0, which
enter the logp of every draw of the fit.  Its loads come from clamped rows, so the shapes are those where a clamp or a chunk edge can go
wrong.  Tolerances are those of tests/test_gpu_scan_reference.py (per draw, C_p = 8 nblk + 4 KC + 32 and C_q = 4 nblk + 16 in units of
eps S): a c/s entry from the wrong row moves the constants, and with them logp, by O(1).

K = 3 paths of L = 7 steps, N in {771, 100} (two 16-draw groups per wave beside the pseudo group at KC <= 12, and one):
  d in {5, 17, 48}       one block, most of its rows beyond d; a one-row last block; an exact multiple of 16
  d = 608, 624 at J = 10 KC = 20: two pseudo groups (20 columns of the factor, then c/s in the second), 38 and 39 blocks, resident
  d = 1200 at J = 6      streamed: the column's rows come chunk by chunk
  targets                low-rank r = 8 and diagonal (the flight), funnel (its column keeps the guarded loads)
Geometry: the tables of the same fits are bit-identical between the default cut, PFMI_QF_NO_TAIL = 1 and PFMI_QF_TWO_LAUNCHES = 1, at
1100 fits of d = 17, where publishers hand the constants to their dependents.
"""
import numpy as np
import pytest

import test_gpu_scan_reference as base
from test_gpu_scan_philox_hoist import HOOKS, _edge_seeds, _tables

pytestmark = pytest.mark.gpu

NS = (771, 100)


def _gauss(pfmi, su, rank, seed):
    W = 0.3 * np.random.default_rng(seed).normal(size=(su.d, rank)) if rank else None
    return pfmi.GaussTarget(su.m, su.sig ** 2, W, offset=-0.5 if rank else 1.25)


def _targets(pfmi, su, seed):
    return ((_gauss(pfmi, su, 8, seed), 1, 8), (_gauss(pfmi, su, 0, seed), 1, 0), (pfmi.FunnelTarget(su.d), 2, 0))


def _check(eng, su, tg, tgt, rpad, kc, picks, storage, cfg):
    for N in NS:
        ng = 2 if (N >= 768 and kc <= 12) else 1
        _, elbo, se = base._scan(eng, N, su.seeds, f"qf:{kc},{tgt},{rpad},{ng}:{storage}:")
        base._run_checks(eng, su, tg, N, picks, f"{cfg}:{kc},{tgt},{rpad},{ng}", elbo, se, kc)


@pytest.mark.parametrize("d", [5, 17, 48])
def test_pseudo_column_small_d(pfmi_mod, eng, d):
    J, kc = 6, 12
    su = base.Setup(pfmi_mod, eng, d, J, K=3, L=7, seed=5 * d + J)
    su.seeds, picks = _edge_seeds(su)
    for tg, tgt, rpad in _targets(pfmi_mod, su, d):
        eng.set_target(tg)
        _check(eng, su, tg, tgt, rpad, kc, picks, "res", "scan_pseudo")


@pytest.mark.parametrize("d,J,storage", [(608, 10, "res"), (624, 10, "res"), (1200, 6, "stream")])
def test_pseudo_column_many_blocks(pfmi_mod, eng, d, J, storage):
    kc = base.eng_kpad(J)
    su = base.Setup(pfmi_mod, eng, d, J, K=3, L=7, seed=d + J)
    picks = [int(su.ok[0]), int(su.ok[-1])]                       # a partial ring and a full history
    for tg, tgt, rpad in _targets(pfmi_mod, su, d):
        eng.set_target(tg)
        _check(eng, su, tg, tgt, rpad, kc, picks, storage, "scan_pseudo_big")


def test_same_bits_on_every_tail_route(pfmi_mod, eng):
    """1100 fits at d = 17, N = 771, rank-8 target: the default cut ends in the one-launch tail (publishers and dependents), the hooks
    give one workgroup per fit and the two-launch tail.  The same tables, ELBOs and standard errors, bit for bit."""
    J, kc, N = 6, 12, 771
    su = base.Setup(pfmi_mod, eng, 17, J, K=22, L=50, seed=23)
    su.seeds, picks = _edge_seeds(su)
    tg = _gauss(pfmi_mod, su, 8, 9)
    eng.set_target(tg)
    got = {}
    for hook, cut in zip(HOOKS, ("tail-share", "whole", "tail-two")):
        run = lambda: base._scan(eng, N, su.seeds, f"qf:{kc},1,8,2:res:{cut}")
        _, elbo, se = run() if hook is None else base._with_hook(hook, "1", run)
        got[cut] = (_tables(eng, picks, N), elbo.copy(), se.copy())
        if hook is None:
            p = picks[0]
            base._check_draws(eng, su, tg, p, N, f"scan_pseudo_tail:{kc},1,8", *eng.elbo_logs(p, N), idx=np.arange(N), kc=kc, elbo=elbo, se=se)
    for cut in ("whole", "tail-two"):
        for a, b in zip(got["tail-share"][0], got[cut][0]):
            assert np.array_equal(a, b, equal_nan=True), cut
        assert np.array_equal(got["tail-share"][1], got[cut][1], equal_nan=True), cut
        assert np.array_equal(got["tail-share"][2], got[cut][2], equal_nan=True), cut
