"""Time one moment pass over the pool (pfmi_pool_moments) against a device-to-device copy of as many bytes and against what a user
has without it (download the pool, reduce with NumPy).

    python tools/pool_moments_bench.py [--configs 1000:64:1000,10000:32:1000] [--reps 20] [--out FILE]

A config is d:K:N_r.  Per config one JSON object:
  kernel_ms / sum_kernel_ms   the moment kernel and the chunk-sum kernel (hipEvent pairs in the stream, pfmi_kernel_time), mean of --reps
  pool_bytes, read_GBps       bytes of the pool (8 d K N_r) and pool bytes per second of the two kernels together
  copy_ms, copy_GBps          torch copy of a device buffer of pool_bytes into another (hipEvents, same process); the rate counts the
                              bytes once, like read_GBps, although the copy also writes them
  read_vs_copy                read_GBps / copy_GBps: >= 1 means the pass is no slower than copying the buffer
  call_ms                     Engine.pool_moments end to end (upload of the centre, both kernels, download of 3 K d + 2 K numbers)
  pool_get_ms, numpy_ms       the alternative: Engine.pool_get() of the draws, then the same four sums with NumPy on the host
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _numpy_moments(P, w, c):
    d, N_r, K = P.shape
    wk = w.reshape(K, N_r)
    T = P - c[:, None, None]
    s1 = np.einsum("dnk,kn->kd", T, wk)
    s2 = np.einsum("dnk,kn->kd", T * T, wk)
    s2w = np.einsum("dnk,kn->kd", T * T, wk * wk)
    return np.stack([wk.sum(axis=1), (wk * wk).sum(axis=1)], axis=1), s1, s2, s2w


def run(pfmi, torch, d, K, N_r, reps, J=6):
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
    nbytes = 8 * d * K * N_r

    got = eng.pool_moments(0, True, center)                     # warm-up
    eng.profile(2)
    m0, n0 = eng.kernel_time("pool_moments")
    s0, _ = eng.kernel_time("pool_moments_sum")
    for _ in range(reps):
        eng.pool_moments(0, True, center)
    m1, n1 = eng.kernel_time("pool_moments")
    s1, _ = eng.kernel_time("pool_moments_sum")
    eng.profile(0)
    kern, ksum = (m1 - m0) / max(n1 - n0, 1), (s1 - s0) / max(n1 - n0, 1)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.pool_moments(0, True, center)
        ts.append((time.perf_counter() - t0) * 1e3)
    call_ms = float(np.median(ts))

    src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda:0").normal_()
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / reps
    del src, dst

    t0 = time.perf_counter()
    P, _ = eng.pool_get()
    pool_get_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = _numpy_moments(P, w, center)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    err = max(float(np.max(np.abs(a - b)) / (1e-300 + np.max(np.abs(b)))) for a, b in zip(got, ref))
    eng.close()
    read = nbytes / ((kern + ksum) * 1e-3) / 1e9
    copy = nbytes / (copy_ms * 1e-3) / 1e9
    return dict(d=d, K=K, N_r=N_r, pool_bytes=nbytes, kernel_ms=kern, sum_kernel_ms=ksum, read_GBps=read, copy_ms=copy_ms, copy_GBps=copy,
                read_vs_copy=read / copy, call_ms=call_ms, pool_get_ms=pool_get_ms, numpy_ms=numpy_ms,
                alternative_over_call=(pool_get_ms + numpy_ms) / call_ms, max_rel_diff_vs_numpy=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1000:64:1000,10000:32:1000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pfmi
    rows = []
    for cfg in a.configs.split(","):
        d, K, N_r = (int(x) for x in cfg.split(":"))
        rows.append(run(pfmi, torch, d, K, N_r, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
