"""What the GPU tests of the passes over the pool share (test_gpu_pool_moments.py, test_gpu_pool_quantiles.py, test_gpu_pool_cross.py): the
named cases and their pools, the shape list at which the column walk switches paths, the longdouble unit roundoff, the ratio of an error
to a derived bound, the walk through the error codes every pass shares, and the child process that compares one engine with two."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_common import _targets
from helpers import ROOT, STANDIN_LIB, make_traces

LD = np.longdouble
U = LD(2.0) ** -53
J = 6
_TRACES = {}

# (case, N_r, K): d = 1 (a single row), 10 / 12 / 30 / 50 / 63 (several columns per wave, one column per wave), 64 and 65 (lanes along
# rows, one load per lane, odd d), 130 (paired loads, two row waves), 257 (odd d over two row tiles), 1000 and 10 000 (paired loads,
# several row tiles, many chunks); N_r = 1, 5, 37, 1000 (one column, fewer columns than slots, a ragged last chunk, many chunks)
CASES = [("d1", 1, 1), ("d1", 5, 3), ("d1", 1000, 3), ("lr10", 5, 1), ("lr10", 1000, 3), ("funnel12", 37, 3), ("diag30", 37, 3),
         ("diag30", 1000, 1), ("lr50", 1, 3), ("lr50", 1000, 1), ("d63", 37, 1), ("d64", 37, 3), ("lr65", 37, 3), ("lr65", 1000, 1),
         ("d130", 37, 3), ("d257", 37, 3), ("d1000", 1000, 3), ("d1000", 5, 1), ("d10000", 37, 3), ("d10000", 5, 1)]


def _traces(pfmi, name):
    """(target, three traces) of a named case, built once per session"""
    if name not in _TRACES:
        small = _targets(pfmi)
        if name in small:
            tg, maxit = small[name], (25 if name.startswith("funnel") else 1000)
        elif name == "d1":
            tg, maxit = pfmi.t_diag(1), 1000
        elif name == "lr65":
            tg, maxit = pfmi.t_lowrank(65, r=3), 1000
        else:                                                  # "d<dim>": diagonal target, three iterations
            tg, maxit = pfmi.t_diag(int(name[1:])), 3
        _TRACES[name] = (tg, make_traces(tg, 3, 11, history_length=J, maxiters=maxit))
    return _TRACES[name]


def _pool(pfmi, eng, name, K, N_r, runs=None):
    """fit the first K (or the given) traces of the case, pool N_r draws of every path's last fit; returns the pool and its PSIS"""
    tg, traces = _traces(pfmi, name)
    traces = [traces[k] for k in (runs if runs is not None else range(K))]
    eng.set_target(tg)
    eng.set_traces([t.points for t in traces], [t.gradients for t in traces])
    eng.fit_batch(J)
    pts = [int(eng.offsets[k + 1]) - 1 for k in range(len(traces))]
    seeds = np.array([1000 + 7 * k for k in (runs if runs is not None else range(K))], dtype=np.uint64)
    eng.pool_build(N_r, pts, seeds)
    P, lr = eng.pool_get()
    assert np.all(np.isfinite(P))
    return np.array(P), lr


def ratio_to_bound(bound, got, ref, A, n):
    """max over entries of |got - ref| / bound(n, A) (an entry with A = 0 must be exact)"""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    b = bound(n, A)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def check_pool_error_codes(pfmi, call, then=None):
    """The error codes every pass over the pool shares, on an engine of its own; call(engine, col_offset, importance) invokes the
    method under test.  No pool: -3; importance without a PSIS result: -3; PSIS weights that do not cover the window: -3; a negative
    col_offset: -1.  then(engine): the caller's own assertions on the engine as the walk leaves it (d = 10, K = 2, N_r = 5, pooled,
    with PSIS weights), before it is closed."""
    e = pfmi.Engine(0)
    try:
        tg, traces = _traces(pfmi, "lr10")
        e.set_target(tg)
        e.set_traces([t.points for t in traces[:2]], [t.gradients for t in traces[:2]])
        e.fit_batch(J)
        with pytest.raises(pfmi.PfmiError) as ex:                # no pool
            call(e, 0, False)
        assert ex.value.code == -3
        pts = [int(e.offsets[k + 1]) - 1 for k in range(2)]
        e.pool_build(5, pts, np.array([1, 2], dtype=np.uint64))
        with pytest.raises(pfmi.PfmiError) as ex:                # importance without a PSIS result
            call(e, 0, True)
        assert ex.value.code == -3
        call(e, 0, False)                                        # uniform weights need none
        _, lr = e.pool_get(draws=False)
        e.psis(lr)
        call(e, 0, True)
        with pytest.raises(pfmi.PfmiError) as ex:                # the PSIS result does not cover [1, 1 + K N_r)
            call(e, 1, True)
        assert ex.value.code == -3
        for imp in (True, False):
            with pytest.raises(pfmi.PfmiError) as ex:
                call(e, -1, imp)
            assert ex.value.code == -1
        if then is not None:
            then(e)
    finally:
        e.close()


def run_two_engines(script, ok_line):
    """run `script` (argv[1]: the repository root) in a child process in which two engines may share GPU 0 through the RCCL stand-in;
    it must exit with 0 and print `ok_line`"""
    assert os.path.exists(STANDIN_LIB), "tests/rccl_standin/librccl_standin.so missing: run __graft_entry__.build()"
    env = dict(os.environ, PFMI_RCCL_LIB=STANDIN_LIB, PFMI_COMM_ALLOW_SHARED_GPU="1", PFMI_STANDIN_TIMEOUT_S="60")
    env.pop("PFMI_COMM_FORCE_RCCL", None)
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=550)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    assert ok_line in r.stdout
