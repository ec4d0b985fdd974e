"""The first batch of the ELBO scan's publishing wave (pathfinder.jl_amd/csrc/elbo_qf_kernel.hip: the `any_pseudo` loop, `pseudo_cols`,
`stage_direct`) draw by draw against the extended-precision reference of tests/scan_reference.py.  In that batch wave 0 carries the
pseudo group(s), whose column KC is c/s and yields the per-fit constants v, t0 and C0 of every draw's logp, and (two groups per wave) one
real 16-draw group.  With a resident factor block and room in LDS the staging code forms c/s once per fit and the wave reads it back;
otherwise the column's inputs are loaded and divided in every block.  The real group of the mixed wave has the row mask of the last
block and the head transform of block 0 (and 1 at KC > 16) in the same loop.  Tolerances are those of tests/test_gpu_scan_reference.py
(per draw, C_p = 8 nblk + 4 KC + 32 and C_q = 4 nblk + 16 in units of eps S): a c/s entry from the wrong row, or a row that should have
been staged as zero, moves the constants and with them logp by O(1).

K = 3 paths of L = 7 steps, N in {771, 100} (two 16-draw groups per wave at KC <= 12: the mixed wave; and one: wave 0 all pseudo):
  d in {5, 17, 48} at J = 6     a block mostly beyond d; a one-row last block; an exact multiple of 16
  d in {608, 624} at J = 10     KC = 20: two pseudo groups, c/s is a column of the second (38 and 39 blocks)
  resident boundary at J = 6    rank-8 target only, see below
  targets                       low-rank r = 8, diagonal, funnel

The resident boundary, from qf_lds_bytes(nblk, 1, 12, 8, NG) = 8 (240 nblk + F) bytes, F = 144 (T) + 276 (constants) + 64 (G) + 256 (head
operands, NG = 2 only) + 1 + 2432 + 128 (table, guard) = 3301 doubles at NG = 2 and 3045 at NG = 1:
  resident while 8 (240 nblk + F) <= 156 KB:           nblk <= 69 (d <= 1104) at NG = 2, nblk <= 70 at NG = 1
  the array (16 nblk doubles more) within 160 KB:      256 nblk + F <= 20480: nblk <= 67 (d <= 1072) at NG = 2, nblk <= 68 (d <= 1088) at NG = 1
So at N = 771 (NG = 2) d = 1072 is the largest shape with the array and d = 1088 (68 blocks) the next block count, resident without it;
at N = 100 (NG = 1) both have it and d = 1104 (69 blocks) is the first without, which is why 1104 is here as well.  d = 1200 streams.

Route identity: PFMI_QF_NO_CS_LDS = 1 makes the launch code leave the array out where it would fit.  Rank-8 target, N = 771 (the
instantiation <12, 1, 8, 2> of the headline configuration, with the mixed wave), d = 48 and d = 1072: tables, ELBOs and standard errors
bit for bit the same on both routes.
Tail routes: 1100 fits of d = 17 (K = 22, L = 50), rank-8, N = 771: tables bit-identical between the default cut (publishers and
dependents), PFMI_QF_NO_TAIL = 1 and PFMI_QF_TWO_LAUNCHES = 1.
"""
import numpy as np
import pytest

import test_gpu_scan_reference as base
from test_gpu_scan_philox_hoist import HOOKS, _edge_seeds, _tables

pytestmark = pytest.mark.gpu

NS = (771, 100)
NO_CS = "PFMI_QF_NO_CS_LDS"


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
def test_first_batch_small_d(pfmi_mod, eng, d):
    J, kc = 6, 12
    su = base.Setup(pfmi_mod, eng, d, J, K=3, L=7, seed=7 * d + J)
    su.seeds, picks = _edge_seeds(su)
    for tg, tgt, rpad in _targets(pfmi_mod, su, d):
        eng.set_target(tg)
        _check(eng, su, tg, tgt, rpad, kc, picks, "res", "scan_first")


@pytest.mark.parametrize("d", [608, 624])
def test_first_batch_two_pseudo_groups(pfmi_mod, eng, d):
    J = 10
    kc = base.eng_kpad(J)
    assert kc == 20
    su = base.Setup(pfmi_mod, eng, d, J, K=3, L=7, seed=d + J + 1)
    picks = [int(su.ok[0]), int(su.ok[-1])]                       # a partial ring and a full history
    for tg, tgt, rpad in _targets(pfmi_mod, su, d):
        eng.set_target(tg)
        _check(eng, su, tg, tgt, rpad, kc, picks, "res", "scan_first_two")


@pytest.mark.parametrize("d,storage", [(1072, "res"), (1088, "res"), (1104, "res"), (1200, "stream")])
def test_first_batch_resident_boundary(pfmi_mod, eng, d, storage):
    """see the module docstring: with the array (1072; 1088 at N = 100), resident without it (1088 at N = 771; 1104), streamed (1200)"""
    J, kc = 6, 12
    su = base.Setup(pfmi_mod, eng, d, J, K=3, L=7, seed=d + J + 2)
    picks = [int(su.ok[0]), int(su.ok[-1])]
    tg = _gauss(pfmi_mod, su, 8, d)
    eng.set_target(tg)
    _check(eng, su, tg, 1, 8, kc, picks, storage, "scan_first_edge")


@pytest.mark.parametrize("d", [48, 1072])
def test_same_bits_with_and_without_the_staged_column(pfmi_mod, eng, d):
    """rank-8 target, N = 771: the staged column against the loads and divisions of every block (PFMI_QF_NO_CS_LDS = 1)"""
    J, kc, N = 6, 12, 771
    su = base.Setup(pfmi_mod, eng, d, J, K=3, L=7, seed=d + J + 3)
    su.seeds, picks = _edge_seeds(su)
    eng.set_target(_gauss(pfmi_mod, su, 8, d))
    run = lambda: base._scan(eng, N, su.seeds, f"qf:{kc},1,8,2:res:")
    _, elbo, se = run()
    staged = (_tables(eng, picks, N), elbo.copy(), se.copy())
    _, elbo, se = base._with_hook(NO_CS, "1", run)
    for a, b in zip(staged[0], _tables(eng, picks, N)):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(staged[1], elbo, equal_nan=True)
    assert np.array_equal(staged[2], se, equal_nan=True)


def test_same_bits_on_every_tail_route(pfmi_mod, eng):
    """1100 fits at d = 17, N = 771, rank-8 target: the default cut ends in the one-launch tail (publishers and dependents), the hooks
    give one workgroup per fit and the two-launch tail.  The same tables, ELBOs and standard errors, bit for bit."""
    J, kc, N = 6, 12, 771
    su = base.Setup(pfmi_mod, eng, 17, J, K=22, L=50, seed=29)
    su.seeds, picks = _edge_seeds(su)
    tg = _gauss(pfmi_mod, su, 8, 11)
    eng.set_target(tg)
    got = {}
    for hook, cut in zip(HOOKS, ("tail-share", "whole", "tail-two")):
        run = lambda: base._scan(eng, N, su.seeds, f"qf:{kc},1,8,2:res:{cut}")
        _, elbo, se = run() if hook is None else base._with_hook(hook, "1", run)
        got[cut] = (_tables(eng, picks, N), elbo.copy(), se.copy())
        if hook is None:
            p = picks[0]
            base._check_draws(eng, su, tg, p, N, f"scan_first_tail:{kc},1,8", *eng.elbo_logs(p, N), idx=np.arange(N), kc=kc, elbo=elbo, se=se)
    for cut in ("whole", "tail-two"):
        for a, b in zip(got["tail-share"][0], got[cut][0]):
            assert np.array_equal(a, b, equal_nan=True), cut
        assert np.array_equal(got["tail-share"][1], got[cut][1], equal_nan=True), cut
        assert np.array_equal(got["tail-share"][2], got[cut][2], equal_nan=True), cut
