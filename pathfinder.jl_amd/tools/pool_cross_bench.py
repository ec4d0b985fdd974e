"""Time the cross-moment pass over the pool (pfmi_pool_cross) against the f64 MFMA peak and against what a user has without it
(download the pool, form (P * w) @ P.T with NumPy).

    python tools/pool_cross_bench.py [--configs 1000:64:1000,10000:32:1000,100:64:1000] [--reps 5] [--tiles 64,128]
                                     [--baseline-max-d 10000] [--out FILE]

A config is d:K:N_r.  Per config one JSON object:
  kernel_ms                   {tile: ms} of the pool_cross kernel alone (hipEvent pairs in the stream, pfmi_kernel_time), mean of --reps
                              after one warm-up call; tile = "default" (what pf_launch_pool_cross picks) and each of --tiles, forced
                              through the PFMI_POOL_CROSS_TILE hook (the bits do not depend on it: same_bits)
  tflops                      {tile: d (d + 1) / 2 * 2 * K N_r flops per second of that kernel time, in 1e12}: the one triangle that is
                              computed; the MFMAs of the unkept half of a diagonal tile are not counted
  frac_of_peak                {tile: tflops / 78.6}, the f64 MFMA peak bench.py and DESIGN.md quote
  workgroups                  {tile: lower-triangle tiles = workgroups of the launch}
  call_ms                     Engine.pool_cross end to end at the default tile: upload of the centre, the kernel, download of d^2 doubles
  pool_get_ms, numpy_ms       the alternative: Engine.pool_get() of the draws, then ((P - c) * w) @ (P - c).T in float64 (skipped above
                              --baseline-max-d: null)
  max_rel_diff_vs_numpy       max |C - numpy| / max |numpy| where the baseline ran
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

PEAK_TF = 78.6


def run(pfmi, d, K, N_r, reps, tiles, baseline_max_d, J=6):
    tg = pfmi.t_lowrank(d, r=8, seed=2)
    eng = pfmi.Engine(0)
    eng.set_target(tg)
    x0 = pfmi.HostRNG(11).rand(K * d).reshape(K, d) * 4 - 2
    eng.optimize_batch(x0, J, 30)
    eng.fit_batch(J)
    pts = [int(eng.offsets[k + 1]) - 1 for k in range(K)]
    eng.pool_build(N_r, pts, np.arange(1, K + 1, dtype=np.uint64))
    _, lr = eng.pool_get(draws=False)
    w = eng.psis(lr)["weights"]
    center = np.asarray(tg.mean, dtype=np.float64)
    flops = d * (d + 1) / 2 * 2 * K * N_r
    L = pfmi.lib()

    kernel_ms, groups, same = {}, {}, {}
    first = None
    for tile in ["default"] + [str(t) for t in tiles]:
        assert L.pfmi_debug_set(b"PFMI_POOL_CROSS_TILE", None if tile == "default" else tile.encode()) == 0
        C = eng.pool_cross(0, True, center)                       # warm-up
        first = C if first is None else first
        same[tile] = bool(np.array_equal(C, first))
        eng.profile(2)
        m0, n0 = eng.kernel_time("pool_cross")
        for _ in range(reps):
            eng.pool_cross(0, True, center)
        m1, n1 = eng.kernel_time("pool_cross")
        eng.profile(0)
        kernel_ms[tile] = (m1 - m0) / max(n1 - n0, 1)
        t = 64 if tile == "default" and d < 4096 else 128 if tile == "default" else int(tile)
        nb = (d + t - 1) // t
        groups[tile] = nb * (nb + 1) // 2
    assert L.pfmi_debug_set(b"PFMI_POOL_CROSS_TILE", None) == 0
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.pool_cross(0, True, center)
        ts.append((time.perf_counter() - t0) * 1e3)
    call_ms = float(np.median(ts))

    pool_get_ms = numpy_ms = rel = None
    if d <= baseline_max_d:
        t0 = time.perf_counter()
        P, _ = eng.pool_get()
        pool_get_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        T = P.reshape(d, K * N_r, order="F") - center[:, None]
        ref = (T * w) @ T.T
        numpy_ms = (time.perf_counter() - t0) * 1e3
        rel = float(np.max(np.abs(first - ref)) / np.max(np.abs(ref)))
    eng.close()
    tf = {k: flops / (ms * 1e-3) / 1e12 for k, ms in kernel_ms.items()}
    return dict(d=d, K=K, N_r=N_r, pool_bytes=8 * d * K * N_r, flops=flops, kernel_ms=kernel_ms, tflops=tf,
                frac_of_peak={k: v / PEAK_TF for k, v in tf.items()}, workgroups=groups, same_bits=same, call_ms=call_ms,
                pool_get_ms=pool_get_ms, numpy_ms=numpy_ms, max_rel_diff_vs_numpy=rel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1000:64:1000,10000:32:1000,100:64:1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiles", default="64,128")
    ap.add_argument("--baseline-max-d", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pfmi
    rows = []
    tiles = [int(t) for t in a.tiles.split(",") if t]
    for cfg in a.configs.split(","):
        d, K, N_r = (int(x) for x in cfg.split(":"))
        rows.append(run(pfmi, d, K, N_r, a.reps, tiles, a.baseline_max_d))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
