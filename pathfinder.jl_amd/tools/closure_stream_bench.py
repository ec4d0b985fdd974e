"""Streaming pipeline for device closures with a gradient, against the packed route, in one process on the same inputs.

Shapes K = 8 and K = 64 (d = 1000, J = 6, N = 1000 ELBO draws, maxiters 1000, x0 seeded from t_lowrank(1000, 8, 2)); closures:
  * hip    the example HIP value and value-and-gradient closures (examples/device_logp)
  * torch  TorchDeviceTarget(grad="autograd") on the same model
routes:
  * packed    optimize_batch ; fit_batch ; elbo_batch_enqueue ; elbo_batch_wait
  * streamed  stream_enqueue ; stream_wait ; elbo_batch_wait
One JSON line per (closure, K, route):
  * wall_ms        host clock from the first call to the reduced ELBO table on the host (median of --reps after one warm-up)
  * rounds         optimiser rounds (pfmi_optimize_stats)
  * opt_ms         host clock until the pump has seen every path finish: the optimiser alone (packed: nothing else runs) or under the
                   concurrent fits and scans (streamed); round_us = opt_ms / rounds
  * bit_identical  (streamed lines) trace lengths, ELBO / SE tables and best iterations equal the packed route's bit for bit;
                   max_rel_elbo the largest relative ELBO difference
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pfmi  # noqa: E402
from closure_lbfgs_bench import hip_target, torch_target  # noqa: E402


def packed(eng, x0, J, N, sd, cap):
    K = x0.shape[0]
    t0 = time.perf_counter()
    eng.optimize_batch_enqueue(x0, J)
    while not eng.optimize_batch_pump():
        pass
    t_opt = time.perf_counter()
    npts = eng.optimize_batch_wait()
    eng.fit_batch(J)
    seeds = np.concatenate([np.concatenate([[np.uint64(0)], sd[k * cap:k * cap + int(npts[k]) - 1]]) for k in range(K)]).astype(np.uint64)
    eng.elbo_batch_enqueue(N, seeds)
    elbo, se, best = eng.elbo_batch_wait()
    t1 = time.perf_counter()
    off = eng.offsets
    el = np.full(K * cap, np.nan)
    ss = np.full(K * cap, np.nan)
    for k in range(K):                                  # packed -> fixed-stride slots, for the comparison
        n = int(npts[k])
        el[k * cap:k * cap + n] = elbo[off[k]:off[k] + n]
        ss[k * cap:k * cap + n] = se[off[k]:off[k] + n]
    return (t1 - t0) * 1e3, (t_opt - t0) * 1e3, npts, el, ss, best


def streamed(eng, x0, J, N, sd, cap):
    K = x0.shape[0]
    t0 = time.perf_counter()
    eng.stream_enqueue(x0, N, sd, J)
    while not eng.stream_pump():                        # the pass that finds every path finished enqueues the reduction and returns True
        pass
    t_opt = time.perf_counter()
    npts = eng.stream_wait()
    elbo, se, best = eng.elbo_batch_wait()
    t1 = time.perf_counter()
    el, ss = elbo.copy(), se.copy()
    for k in range(K):
        el[k * cap + int(npts[k]):(k + 1) * cap] = np.nan
        ss[k * cap + int(npts[k]):(k + 1) * cap] = np.nan
    return (t1 - t0) * 1e3, (t_opt - t0) * 1e3, npts, el, ss, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Ks", default="8,64")
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--closures", default="hip,torch")
    a = ap.parse_args()
    tg = pfmi.t_lowrank(a.d, 8, 2)
    cap = 1001
    eng = pfmi.Engine(0)
    makers = {"hip": lambda: hip_target(tg), "torch": lambda: torch_target(tg)}
    for cname in a.closures.split(","):
        t = makers[cname]()
        eng.set_target(t)
        for K in (int(k) for k in a.Ks.split(",")):
            x0 = pfmi.HostRNG(11).rand(K * a.d).reshape(K, a.d) * 4 - 2
            sd = pfmi.hostrng.rand_u64(77, np.arange(K * cap, dtype=np.uint64), 9)
            out = {}
            for route, fn in (("packed", packed), ("streamed", streamed)):
                fn(eng, x0, a.J, a.N, sd, cap)                                 # warm-up: allocation, code objects, torch
                walls, opts = [], []
                for _ in range(a.reps):
                    eng.sync()
                    w, o, npts, el, ss, best = fn(eng, x0, a.J, a.N, sd, cap)
                    walls.append(w)
                    opts.append(o)
                rounds, cols = eng.optimize_stats()
                out[route] = (npts, el, ss, best)
                line = {"closure": cname, "K": K, "d": a.d, "J": a.J, "N": a.N, "route": route, "wall_ms": float(np.median(walls)),
                        "wall_ms_all": walls, "opt_ms": float(np.median(opts)), "rounds": rounds, "closure_columns": cols,
                        "round_us": float(np.median(opts)) * 1e3 / max(rounds, 1), "points": int(npts.sum()), "fits": int((npts - 1).sum())}
                if route == "streamed":
                    p = out["packed"]
                    ok = np.isfinite(p[1])
                    same = (np.array_equal(p[0], npts) and np.array_equal(p[1], el, equal_nan=True) and np.array_equal(p[2], ss, equal_nan=True)
                            and np.array_equal(p[3], best))
                    line["bit_identical"] = bool(same)
                    line["max_rel_elbo"] = float(np.max(np.abs(el[ok] - p[1][ok]) / np.maximum(1.0, np.abs(p[1][ok])))) if ok.any() else 0.0
                    line["speedup_vs_packed"] = float(np.median(out["packed_walls"]) / np.median(walls))
                else:
                    out["packed_walls"] = walls
                print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
