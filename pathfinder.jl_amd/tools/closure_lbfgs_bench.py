"""Device L-BFGS for user closures at config 3's shape (K = 64, d = 1000, J = 6, x0 from t_lowrank(1000, 8, 2)): wall time until the traces
are resident on the GPU for
  * closure_hip    the closure optimiser with the example HIP value-and-gradient closure (examples/device_logp)
  * closure_torch  the closure optimiser with TorchDeviceTarget(grad="autograd")
  * host           the host driver (pfmi/optimize.py) on the same target, then set_traces
  * builtin        the built-in pf_lbfgs_kernel (reference point)
with a host clock around work that ends in a synchronisation; rounds and closure columns of the closure runs.  One JSON line per optimiser.
Per-round kernel time comes from a separate `rocprofv3 --kernel-trace --stats` run of `--only closure_hip`."""
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
import pfmi  # noqa: E402


def hip_target(tg):
    pfmi.lib()
    L = C.CDLL(os.path.join(ROOT, "examples", "device_logp", "liblogp_demo.so"))
    dp = C.POINTER(C.c_double)
    L.pfx_gauss_create.restype = C.c_void_p
    L.pfx_gauss_create.argtypes = [C.c_int32, C.c_int32, dp, dp, dp, dp, C.c_double]
    h = L.pfx_gauss_create(tg.d, tg.r, tg.mean.ctypes.data_as(dp), tg.a.ctypes.data_as(dp), tg.Wd.ctypes.data_as(dp),
                           tg.G.ctypes.data_as(dp), tg.offset)
    return pfmi.DeviceCallbackTarget(tg.d, C.cast(L.pfx_gauss_logp, C.c_void_p).value, C.c_void_p(h), host=tg, keepalive=(L, h),
                                     grad_fn=C.cast(L.pfx_gauss_logp_grad, C.c_void_p).value)


def torch_target(tg):
    import torch
    m, a = torch.tensor(tg.mean, device="cuda"), torch.tensor(tg.a, device="cuda")
    wd, G = torch.tensor(tg.Wd, device="cuda"), torch.tensor(tg.G, device="cuda")

    def fn(X):
        e = X - m
        t = (e @ wd) @ G.T
        return tg.offset - 0.5 * ((a * e * e).sum(1) - (t * t).sum(1))
    return pfmi.TorchDeviceTarget(tg.d, fn, host=tg, grad="autograd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-paths", type=int, default=64, help="paths the host driver runs (its time is scaled to K)")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    tg = pfmi.t_lowrank(a.d, 8, 2)
    x0 = pfmi.HostRNG(11).rand(a.K * a.d).reshape(a.K, a.d) * 4 - 2
    eng = pfmi.Engine(0)
    runs = {"closure_hip": lambda: hip_target(tg), "closure_torch": lambda: torch_target(tg), "builtin": lambda: tg, "host": None}
    for name, make in runs.items():
        if a.only and name != a.only:
            continue
        if name == "host":
            kh = min(a.host_paths, a.K)
            t0 = time.perf_counter()
            trs = [pfmi.optimize_with_trace(tg, x0[k], a.J) for k in range(kh)]
            eng.set_traces([t.points for t in trs], [t.gradients for t in trs])
            eng.sync()
            ms = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"optimizer": name, "K": a.K, "d": a.d, "J": a.J, "paths_run": kh, "wall_ms": ms * a.K / kh,
                              "points": int(sum(len(t) for t in trs))}), flush=True)
            continue
        eng.set_target(make())
        eng.optimize_batch(x0, a.J)                                 # warm-up (allocation, code objects, torch)
        ts = []
        for _ in range(a.reps):
            eng.sync()
            t0 = time.perf_counter()
            npts = eng.optimize_batch(x0, a.J)
            eng.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        rounds, cols = eng.optimize_stats() if name != "builtin" else (0, 0)
        print(json.dumps({"optimizer": name, "K": a.K, "d": a.d, "J": a.J, "wall_ms": float(np.median(ts)), "wall_ms_all": ts,
                          "rounds": rounds, "closure_columns": cols, "points": int(npts.sum()), "max_points": int(npts.max())}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
