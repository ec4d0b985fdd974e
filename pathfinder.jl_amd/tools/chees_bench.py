"""ChEES-HMC (pfmi_chees_enqueue) beside the device warm-up of static HMC and of NUTS, in one process on the same fit, starts and seeds.

Shape: d = 1000, K = 64 chains, J = 6, the example HIP closure of examples/device_logp on t_lowrank(1000, 8, 2) (tools/adapt_bench.py's
setup).  One JSON line:
  * step_us        stage time per step launch under pfmi_profile(2), [median, min, max] over --reps: the ChEES step kernel in a sampling
                   run (nwarmup = 0, tau_0 = 16 eps_0: 8.5 leapfrog steps on average) against the warm kernel of pfmi_hmc_adapt_enqueue
                   with nleapfrog = 8, measured TWICE per repetition (hmc_adapt, hmc_adapt_again): the gap between the two is the
                   run-to-run spread the ChEES figure is read against.  (The at most 4 idle launches a ChEES run issues ahead of its last
                   progress word are in its count.)
  * step_us_synchronised  the same under pfmi_profile(1), where every stage is host-synchronised and each launch runs on an empty queue
  * update_us      a warm-up run of nwarmup transitions: the "chees_update" stage (the update's three launches and the opening launch, issued
                   behind every round of the warm-up and doing nothing unless the round ended a transition) per warm-up transition,
                   beside the rest of a warm-up transition (its step launches and closure calls)
  * columns_per_ess  closure columns of a whole run (warm-up included) per unit of minimum bulk ESS over the coordinates
                   (pfmi_chain_diagnostics), ChEES against pfmi_nuts_adapt_enqueue; reported, not asserted
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pfmi  # noqa: E402
from closure_lbfgs_bench import hip_target  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--nwarmup", type=int, default=200)
    ap.add_argument("--max-leapfrog", type=int, default=64)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    K, d, W, T = a.K, a.d, a.nwarmup, a.T
    tg = pfmi.t_lowrank(d, 8, 2)
    eng = pfmi.Engine(0)
    eng.set_target(hip_target(tg))
    x0 = pfmi.HostRNG(3).rand(d).reshape(1, d) * 4 - 2
    npts = eng.optimize_batch(x0, a.J, 200, 1e-8)
    eng.fit_batch(a.J)
    _, _, best = eng.elbo_batch(64, pfmi.hostrng.rand_u64(5, np.arange(int(npts[0]), dtype=np.uint64), 9))
    p = int(best[0])
    th, _, _ = eng.get_trace(0)
    pts = np.full(K, p, dtype=np.int64)
    X0 = np.asfortranarray(np.repeat(th[p][:, None], K, axis=1))
    seeds = pfmi.HostRNG(17).rand_u64(K)
    eps0 = d ** -0.25

    def stages(names, fn):
        m0 = {n: eng.kernel_time(n) for n in names}
        fn()
        return {n: (eng.kernel_time(n)[0] - m0[n][0], eng.kernel_time(n)[1] - m0[n][1]) for n in names}

    def chees(w, t, tau0=0.0):
        eng.chees_enqueue(pts, X0, seeds, eps0, tau0, a.max_leapfrog, w, t)
        eng.chees_wait()

    def adapt(t):
        eng.hmc_adapt_enqueue(pts, X0, seeds, np.full(K, eps0), 8, 1, t)
        eng.hmc_wait()

    stat = lambda v: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]     # noqa: E731
    chees(W, 8); adapt(8)                                       # unmeasured
    eng.profile(2)
    N = 50
    s_ch, s_ad, s_ad2, upd, rest, Ls = [], [], [], [], [], []
    for _ in range(a.reps):
        r = stages(["hmc_adapt"], lambda: adapt(N))["hmc_adapt"]; s_ad.append(r[0] / r[1] * 1e3)
        r = stages(["chees"], lambda: chees(0, N, 16 * eps0))["chees"]; s_ch.append(r[0] / r[1] * 1e3)
        r = stages(["hmc_adapt"], lambda: adapt(N))["hmc_adapt"]; s_ad2.append(r[0] / r[1] * 1e3)
        r = stages(["chees", "chees_closure", "chees_update"], lambda: chees(W, 1))
        upd.append(r["chees_update"][0] / W * 1e3)
        rest.append((r["chees"][0] + r["chees_closure"][0]) / W * 1e3)
        Ls.append(float(eng.chees_get()["n_leapfrog"][:W].mean()))
    # the same three under pfmi_profile(1), every stage host-synchronised: each launch is timed on an empty queue, so what the pump's
    # bounded window does to a full queue is taken out and only the kernels differ
    eng.profile(1)
    y_ch, y_ad, y_ad2 = [], [], []
    for _ in range(a.reps):
        r = stages(["hmc_adapt"], lambda: adapt(N))["hmc_adapt"]; y_ad.append(r[0] / r[1] * 1e3)
        r = stages(["chees"], lambda: chees(0, N, 16 * eps0))["chees"]; y_ch.append(r[0] / r[1] * 1e3)
        r = stages(["hmc_adapt"], lambda: adapt(N))["hmc_adapt"]; y_ad2.append(r[0] / r[1] * 1e3)
    eng.profile(0)
    # closure columns per unit of minimum bulk ESS
    chees(W, T)
    ch = eng.chees_get()
    ess_c = float(np.min(eng.chain_diagnostics()["ess_bulk"]))
    col_c = eng.chees_stats()[1]
    acc_c = float(eng.hmc_get(draws=False)["accept_prob"].mean())
    eng.nuts_adapt_enqueue(pts, X0, seeds, np.full(K, eps0), a.max_depth, W, T)
    eng.nuts_wait()
    ess_n = float(np.min(eng.chain_diagnostics()["ess_bulk"]))
    col_n = eng.nuts_stats()[1]
    _, nl = eng.nuts_get_stats()
    print(json.dumps({"d": d, "K": K, "nwarmup": W, "T": T, "reps": a.reps,
                      "step_us": {"chees": stat(s_ch), "hmc_adapt": stat(s_ad), "hmc_adapt_again": stat(s_ad2)},
                      "step_us_synchronised": {"chees": stat(y_ch), "hmc_adapt": stat(y_ad), "hmc_adapt_again": stat(y_ad2)},
                      "update_us": {"chees_update_per_transition": stat(upd), "steps_and_closure_per_transition": stat(rest), "mean_warmup_L": stat(Ls)},
                      "columns_per_ess": {"chees": round(col_c / ess_c, 2), "nuts": round(col_n / ess_n, 2), "chees_columns": col_c, "nuts_columns": col_n,
                                          "chees_min_ess_bulk": round(ess_c, 1), "nuts_min_ess_bulk": round(ess_n, 1)},
                      "chees": {"step_size": round(ch["step_size"], 4), "traj_length": round(ch["traj_length"], 4), "status": ch["status"],
                                "mean_L": round(float(ch["n_leapfrog"][W:].mean()), 2), "accept": round(acc_c, 3)},
                      "nuts": {"mean_leapfrog": round(float(nl.mean()), 2)}}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
