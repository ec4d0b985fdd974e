"""pfmi_chain_diagnostics(PFMI_CHAIN_SRC_HMC, PFMI_CHAIN_WITH_LP) on resident HMC chains -- d = 1000, K = 64, T = 200 and T = 1000, chains
of the example Gaussian closure of examples/device_logp set up as in tests/probes/hmc_probe.py -- against what the library offered
before: pfmi_hmc_get of the draws plus the numpy reference of tests/chain_diag_reference.py on the host.  Writes its table as markdown
to the path given as the first argument (default: profiles/chain_diagnostics.md).

  wall time     host clock around the call, profiling off, median of REPEATS after WARMUP warm-up calls
  kernel split  pfmi_kernel_time of the five stages under pfmi_profile mode 2, a call of its own
  baseline      host clock around hmc_get (draws and logp), plus the float64 reference on BASE_COORDS coordinates, scaled to d + 1
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "pathfinder.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np                                         # noqa: E402
import pfmi                                                # noqa: E402
import chain_diag_reference as R                           # noqa: E402
from helpers import demo_device_target, fit_seeds          # noqa: E402

D, J, K, LF = 1000, 6, 64, 8
SHAPES = (200, 1000)
WARMUP, REPEATS, BASE_COORDS = 2, 7, 24
CUS, GHZ = 256, 2.4
STAGES = ("chain_diag_transpose", "chain_diag_moments", "chain_diag_rank", "chain_diag_ess", "chain_diag_final")


def main(out_path):
    tg = pfmi.t_lowrank(D, r=8, seed=2, wscale=2.0 / np.sqrt(D))
    eng = pfmi.Engine(0)
    eng.set_target(demo_device_target(tg, grad=True))
    x0p = pfmi.HostRNG(2024).rand(4 * D).reshape(4, D) * 4 - 2
    eng.optimize_batch(x0p, J, 200)
    eng.fit_batch(J)
    status = eng.fit_status()[0]
    _, _, best = eng.elbo_batch(64, fit_seeds(eng.P, 3))
    p = int(eng.offsets[0]) + int(best[0])
    assert status[p] == 0
    th, _, _ = eng.get_trace(0)
    x0 = np.asfortranarray(th[int(best[0])][:, None] + eng.woodbury_apply(p, "unwhiten", np.random.default_rng(5).standard_normal((D, K))))
    seeds = np.asarray(pfmi.hostrng.rand_u64(99, np.arange(K, dtype=np.uint64), 9), dtype=np.uint64)
    pts = np.full(K, p, dtype=np.int64)
    rows = []
    for T in SHAPES:
        eng.hmc_enqueue(pts, x0, seeds, 0.6 * D ** -0.25, LF, T)
        eng.hmc_wait()
        for _ in range(WARMUP):
            out = eng.chain_diagnostics(with_lp=True)
        wall = []
        for _ in range(REPEATS):
            eng.sync()
            t0 = time.perf_counter()
            out = eng.chain_diagnostics(with_lp=True)
            wall.append(time.perf_counter() - t0)
        eng.profile(2)
        eng.chain_diagnostics(with_lp=True)
        split = {s: eng.kernel_time(s)[0] for s in STAGES}
        eng.profile(0)
        tiled = eng.kernel_time("chain_diag:count:tiled")[1] > 0
        # the baseline: download, then the float64 reference on a few coordinates and logp
        t0 = time.perf_counter()
        got = eng.hmc_get()
        t_get = time.perf_counter() - t0
        sub = np.concatenate([got["draws"][:BASE_COORDS - 1], got["logp"].T[None]])
        t0 = time.perf_counter()
        ref = R.diagnostics(sub)
        t_ref = (time.perf_counter() - t0) / BASE_COORDS * (D + 1)
        idx = list(range(BASE_COORDS - 1)) + [D]
        agree = max(float(np.max(np.abs(out[k][idx] - ref[k]) / (1 + np.abs(ref[k])))) for k in R.KEYS)
        Sp = 2 * K * (T // 2)
        rows.append(dict(T=T, Sp=Sp, wall=float(np.median(wall)), best=float(np.min(wall)), split=split, tiled=tiled, t_get=t_get, t_ref=t_ref,
                         agree=agree, acc=float(got["accept_prob"].mean()), rhat=float(np.nanmax(out["rhat"])),
                         bulk=float(np.nanmin(out["ess_bulk"])), tail=float(np.nanmin(out["ess_tail"])),
                         pairs=2.0 * (D + 1) * float(Sp) ** 2))
    eng.close()
    L = ["# Chain diagnostics on device: what a call costs", "",
         "Written by `tests/probes/chain_diag_probe.py` on an MI355X.  Chains: d = %d, K = %d static HMC chains (Lf = %d) on one fit of the" % (D, K, LF),
         "example Gaussian closure of `examples/device_logp`, set up as in `profiles/hmc.md`.  The call:",
         "`pfmi_chain_diagnostics(PFMI_CHAIN_SRC_HMC, PFMI_CHAIN_WITH_LP)`, d + 1 = %d series.  Wall times: host clock, profiling off, median of" % (D + 1),
         "%d after %d warm-up calls.  Kernel split: `pfmi_kernel_time` under profile mode 2, a call of its own." % (REPEATS, WARMUP), ""]
    L += ["| quantity | " + " | ".join("T = %d (S' = %d)" % (r["T"], r["Sp"]) for r in rows) + " |", "|---|" + "---|" * len(rows)]

    def line(name, f):
        L.append("| " + name + " | " + " | ".join(f(r) for r in rows) + " |")

    line("wall time of the call", lambda r: "median %.2f ms, best %.2f ms" % (1e3 * r["wall"], 1e3 * r["best"]))
    for s in STAGES:
        line("`%s`" % s, lambda r, s=s: "%.3f ms" % r["split"][s])
    line("counting plan", lambda r: "`chain_diag:count:%s`" % ("tiled" if r["tiled"] else "one"))
    line("pairs the definition compares, 2 (d + 1) S'^2", lambda r: "%.3g (%.3g per second of `chain_diag_rank`)" % (r["pairs"], r["pairs"] / (1e-3 * r["split"]["chain_diag_rank"])))
    line("baseline: `pfmi_hmc_get` (draws, logp)", lambda r: "%.1f ms" % (1e3 * r["t_get"]))
    line("baseline: numpy float64 reference, %d series timed, scaled to d + 1" % BASE_COORDS, lambda r: "%.1f s" % r["t_ref"])
    line("ratio baseline / device", lambda r: "%.0fx" % ((r["t_get"] + r["t_ref"]) / r["wall"]))
    line("device vs reference on the timed series (max relative)", lambda r: "%.1e" % r["agree"])
    line("the chains: acceptance, max rhat, min ess_bulk, min ess_tail", lambda r: "%.2f, %.4f, %.0f, %.0f" % (r["acc"], r["rhat"], r["bulk"], r["tail"]))
    L.append("")
    r = rows[-1]
    dev_ms = sum(r["split"].values())
    ntiles = (r["Sp"] + R.TILE - 1) // R.TILE
    reads = 2.0 * 2.0 * (D + 1) * r["Sp"] * ntiles * 12 / 64.0          # two transforms, two searches of 12 LDS reads, per wave of 64
    per_cu = CUS * GHZ * 1e9 * 1e-3 * r["split"]["chain_diag_rank"] / reads
    L += ["What the call costs at these shapes.  `chain_diag_rank` (two tile sorts and two counting passes) is %.0f %% of the device time at"
          % (100.0 * r["split"]["chain_diag_rank"] / dev_ms),
          "T = %d, `chain_diag_ess` %.0f %%; transpose, moments and the final kernel together stay below %.1f ms.  The counting pass does, per"
          % (r["T"], 100.0 * r["split"]["chain_diag_ess"] / dev_ms, r["split"]["chain_diag_transpose"] + r["split"]["chain_diag_moments"] + r["split"]["chain_diag_final"] + 0.05),
          "value and sorted tile of %d, two binary searches of 12 dependent LDS reads: %.3g wave-wide reads in all, one per %.0f clocks and"
          % (R.TILE, reads, per_cu),
          "compute unit (%d units at %.1f GHz).  The searches read scattered addresses, so their reads conflict on LDS banks, and each"
          % (CUS, GHZ),
          "waits for the one before it; which of the two -- bank conflicts or the latency of dependent reads between the two barriers of a",
          "tile -- bounds the stage was not separated: no counters were collected.  The row of pairs is the work the pairwise definition",
          "implies, not what is executed (the first version of the stage did execute it: 882 ms at T = 1000).  The autocovariance stage",
          "stops at Geyer's truncation point; its time depends on how fast the chains mix.",
          "The baseline is what the library offered before: download the records, then rank, transform and autocorrelate on the host in",
          "numpy, coordinate by coordinate (`tests/chain_diag_reference.py`, float64); the reference was timed on %d series and scaled." % BASE_COORDS,
          "Not measured: the stages under `rocprofv3`, hardware counters, other d or K, a multi-threaded host baseline.", ""]
    open(out_path, "w").write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chain_diagnostics.md"))
