"""Time the logpdf of a uniform mixture of K fits at N points (pfmi_mixture_logpdf) against what a user has without it.

    python tools/mixture_logpdf_bench.py [--K 64] [--dim 1000] [--J 6] [--N 10000] [--reps 10] [--out FILE]

Reports (one JSON object):
  kernel_ms          the main mixture kernel (pfmi_kernel_time "mixture_logpdf", event pairs in the stream) and the lse reduction
  lane_kernel_ms     the general path (PFMI_MIXTURE_KERNEL=lane: pfmi_logpdf's lane-per-point algebra, one grid row per component)
  host_ms / dev_ms   Engine.mixture_logpdf end to end from a host array / from a torch tensor on the device (median of --reps)
  loop_ms            the per-component loop a user has today: K calls of pfmi_logpdf on the same host X + a host log-sum-exp
  mfma_fraction      contraction flops (2 passes x 2 d kpad per (k, n)) / kernel time / the 78.6 TF f64 MFMA peak
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

F64_MFMA_PEAK = 78.6e12


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _kernel_ms(eng, fn, reps):
    eng.profile(2)                           # (the totals accumulate: read them before and after)
    m0, n0 = eng.kernel_time("mixture_logpdf")
    l0, _ = eng.kernel_time("mixture_lse")
    for _ in range(reps):
        fn()
    m1, n1 = eng.kernel_time("mixture_logpdf")
    l1, _ = eng.kernel_time("mixture_lse")
    eng.profile(0)
    return (m1 - m0) / max(n1 - n0, 1), (l1 - l0) / max(n1 - n0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--dim", type=int, default=1000)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--N", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pfmi
    from scipy.special import logsumexp

    d, K, N = a.dim, a.K, a.N
    tg = pfmi.t_lowrank(d, r=8, seed=2)
    eng = pfmi.Engine(0)
    eng.set_target(tg)
    x0 = pfmi.HostRNG(11).rand(K * d).reshape(K, d) * 4 - 2
    eng.optimize_batch(x0, a.J, 200)
    eng.fit_batch(a.J)
    status = eng.fit_status()[0]
    pts = []
    for k in range(K):                                      # each run's last point with a usable fit
        ok = [p for p in range(int(eng.offsets[k]) + 1, int(eng.offsets[k + 1])) if status[p] == 0]
        pts.append(ok[-1] if ok else int(eng.offsets[k]))
    X = np.asfortranarray(np.random.default_rng(0).normal(size=(d, N)) * 2 + np.asarray(tg.mean)[:, None])
    Xt = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda:0").t()
    kpad = min(k for k in (4, 8, 12, 16, 20, 32, 64) if k >= 2 * a.J)     # the factor's column padding

    lse_host = eng.mixture_logpdf(pts, X)
    lse_dev = eng.mixture_logpdf(pts, Xt).cpu().numpy()
    loop = np.stack([eng.logpdf(p, X) for p in pts], axis=1)
    lse_loop = logsumexp(loop, axis=1)
    err = float(np.max(np.abs(lse_host - lse_loop) / (1 + np.abs(lse_loop))))

    kern, lse_k = _kernel_ms(eng, lambda: eng.mixture_logpdf(pts, Xt), a.reps)
    pfmi.lib().pfmi_debug_set(b"PFMI_MIXTURE_KERNEL", b"lane")
    try:
        lane, _ = _kernel_ms(eng, lambda: eng.mixture_logpdf(pts, Xt), max(2, a.reps // 3))
    finally:
        pfmi.lib().pfmi_debug_set(b"PFMI_MIXTURE_KERNEL", None)
    host = _median_ms(lambda: eng.mixture_logpdf(pts, X), a.reps)
    dev = _median_ms(lambda: eng.mixture_logpdf(pts, Xt), a.reps)
    loop_ms = _median_ms(lambda: logsumexp(np.stack([eng.logpdf(p, X) for p in pts], axis=1), axis=1), max(2, a.reps // 3))
    flops = 2.0 * 2.0 * d * kpad * K * N
    out = dict(K=K, d=d, J=a.J, kpad=kpad, N=N, kernel_ms=kern, lse_kernel_ms=lse_k, lane_kernel_ms=lane, host_ms=host, dev_ms=dev,
               loop_ms=loop_ms, dev_speedup_vs_loop=loop_ms / dev, host_speedup_vs_loop=loop_ms / host,
               contraction_flops=flops, mfma_fraction=flops / (kern * 1e-3) / F64_MFMA_PEAK,
               host_equals_dev=bool(np.array_equal(lse_host, lse_dev)), max_rel_err_vs_loop=err,
               fits_ok=int(sum(status[p] == 0 for p in pts)))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
