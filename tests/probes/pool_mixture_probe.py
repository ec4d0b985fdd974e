"""Mixture-proposal weights of the pool (pfmi_pool_mixture_ratios): what the call costs next to the ELBO scan of the same shape, what
the lane route (pfmi_mixture_logpdf_dev on the pool's pointer, the only route for these columns before the row-tiled kernel) costs on
a slice of the same columns, and k-hat / tail length / ESS of the pooled PSIS under both proposals.

    python tests/probes/pool_mixture_probe.py time  --shape c3 | c5 [--reps 5] [--lane-slice 32]
    python tests/probes/pool_mixture_probe.py khat  [--target c3 | small]

`time` prints one JSON line: seconds of the scan, of the call (every repetition), of the lane route on 1 / lane-slice of the columns
(every repetition, NOT scaled), the bytes of the kernel's traffic model and the rate they give.  Shapes: c3 = config 3's pool (K = 64,
N_r = 1000, d = 1000, J = 6, low-rank target), c5 = one GPU's share of config 5 (K = 32, N_r = 1000, d = 10 000, J = 10, funnel).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "pathfinder.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pfmi  # noqa: E402
from pfmi.hostrng import rand_u64  # noqa: E402

SHAPES = {"c3": dict(K=64, d=1000, J=6, N=1000, target=lambda d: pfmi.t_lowrank(d, r=8, seed=2)),
          "c5": dict(K=32, d=10000, J=10, N=1000, target=lambda d: pfmi.t_funnel(d))}


def kpad_for(J):
    return next(o for o in (4, 8, 12, 16, 20, 32, 64) if 2 * J <= o)


def traffic_model_bytes(d, kpad, K, S):
    """bytes pf_pool_mixture_tiled_kernel asks the memory system for: per 16-column tile and component, X twice (2 x 16 d doubles) and the
    factor twice (2 d (kpad + 2) doubles); ceil(S / 16) tiles, K components"""
    return 8.0 * (-(-S // 16)) * K * (2 * 16 * d + 2 * d * (kpad + 2))


def pooled(eng, shape, master=20260928, maxiters=1000):
    """optimise, fit, scan (timed), pool of the winners: returns (scan seconds, points of the pool)"""
    K, d, J, N = shape["K"], shape["d"], shape["J"], shape["N"]
    eng.set_target(shape["target"](d))
    run_seeds = rand_u64(master, np.arange(K, dtype=np.uint64), 9)
    x0 = np.stack([pfmi.HostRNG(int(s)).rand(d) * 4 - 2 for s in run_seeds])
    npts = eng.optimize_batch(x0, J, maxiters)
    seeds = np.concatenate([rand_u64(int(run_seeds[i]), np.arange(n, dtype=np.uint64), 10) for i, n in enumerate(npts)])
    eng.fit_batch(J)
    eng.elbo_batch(N, seeds)                             # warm-up of the shape
    eng.sync()
    t0 = time.perf_counter()
    eng.elbo_batch(N, seeds)
    eng.sync()
    t_scan = time.perf_counter() - t0
    eng.pool_build_best(N)
    pts, _, ok = eng.pool_winners()
    return t_scan, pts, int(eng.P), int(ok.sum())


def psis_stats(eng, ptr, S):
    r = eng.psis_dev(ptr, S)
    w = r["weights"]
    return dict(khat=r["pareto_shape"], tail=int(r["tail_length"]), ess=float(1.0 / np.sum((w / w.sum()) ** 2)), S=int(S))


def cmd_time(args):
    shape = SHAPES[args.shape]
    K, d, J, N = shape["K"], shape["d"], shape["J"], shape["N"]
    S = K * N
    eng = pfmi.Engine(0)
    t_scan, pts, P, nok = pooled(eng, shape)
    eng.pool_mixture_ratios(want=False)                  # warm-up: code object, scratch
    eng.sync()
    t_call = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        eng.pool_mixture_ratios(want=False)              # blocks
        t_call.append(time.perf_counter() - t0)
    out = dict(shape=args.shape, K=K, d=d, J=J, N_r=N, fits=P, successful_runs=nok, scan_s=t_scan, call_s=t_call)
    out["mixture"] = psis_stats(eng, eng.pool_mixture_ratios_dev()[0], S)
    out["component"] = psis_stats(eng, eng.pool_log_ratios_dev()[0], S)
    if d > 1024:
        out["model_bytes"] = traffic_model_bytes(d, kpad_for(J), K, S)
        out["model_bytes_per_s"] = out["model_bytes"] / min(t_call)
    if args.lane_slice > 0:                              # the lane route on the first S / lane_slice columns of the same pool
        n = max(16, S // args.lane_slice)
        ptr, _ = eng.pool_draws_dev()
        buf = eng.malloc_dev(8 * n)
        p64 = np.ascontiguousarray(pts, dtype=np.int64)
        t_lane = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            rc = pfmi.lib().pfmi_mixture_logpdf_dev(eng.ctx, C.c_int32(K), p64.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int64(n),
                                                    C.c_void_p(ptr), C.c_void_p(buf), None)
            assert rc == 0, rc
            eng.sync()
            t_lane.append(time.perf_counter() - t0)
        lse = eng.memcpy_d2h(np.empty(n), buf)
        eng.free_dev(buf)
        lmix, _ = eng.pool_mixture_ratios()
        ref = lse - np.log(K)
        out.update(lane_columns=n, lane_s=t_lane[1:], lane_first_s=t_lane[0],
                   lane_route="mfma" if d <= 1024 and J <= 16 else "lane",
                   max_rel_diff_vs_lane=float(np.nanmax(np.abs(lmix[:n] - ref) / np.maximum(np.abs(ref), 1))))
    print(json.dumps(out), flush=True)
    eng.close()


def cmd_khat(args):
    from gpu_common import _targets
    eng = pfmi.Engine(0)
    if args.target == "c3":
        cases = {"config3 lowrank d=1000 K=64": (pfmi.t_lowrank(1000, r=8, seed=2), dict(nruns=64, ndraws_elbo=1000), 1000)}
    else:
        cases = {f"small:{n}": (tg, dict(nruns=8, ndraws_elbo=200), 400) for n, tg in _targets(pfmi).items()}
    for name, (tg, kw, ndraws) in cases.items():
        row = dict(target=name)
        for proposal in ("component", "mixture"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                r = pfmi.multipathfinder(tg, ndraws, rng=pfmi.HostRNG(20260928), engine=eng, proposal=proposal, **kw)
            w = r.psis_result.weights
            row[proposal] = dict(khat=r.psis_result.pareto_shape, tail=int(r.psis_result.tail_length), S=len(w),
                                 ess=float(1.0 / np.sum((w / w.sum()) ** 2)), runs_resampled=int(len(set(r.draw_component_ids.tolist()))))
        print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--shape", choices=sorted(SHAPES), default="c3")
    t.add_argument("--reps", type=int, default=5)
    t.add_argument("--lane-slice", type=int, default=32, help="time the lane route on 1/n of the columns (0: not at all)")
    k = sub.add_parser("khat")
    k.add_argument("--target", choices=["c3", "small"], default="small")
    a = ap.parse_args()
    {"time": cmd_time, "khat": cmd_khat}[a.cmd](a)
