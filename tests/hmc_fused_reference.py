"""Reference of the fused static-HMC kernel (pathfinder.jl_amd/csrc/hmc_fused_kernel.hip, hmc_target.h).  Not collected by pytest; used by
tests/test_gpu_hmc_fused.py / test_gpu_hmc_fused_steps.py and pinned on the CPU by tests/test_hmc_fused_reference_cpu.py.

The transition is hmc_reference's (mirror, check); what is new in the kernel is the target evaluation, and this file holds its
long-double reference: value AND gradient of both built-in targets with their absolute-value majorants (scan_reference.target_logp has
the value; the gradient is added here), and the case grids of the tests.

Bound on the target evaluation, in the style of hmc_reference's docstring: |value - ref| <= C eps S with eps = 2^-52 (two unit roundoffs
per counted step), S the same sums with every term replaced by its absolute value, and C counted from the kernel's reduction map
(hmc_target.h), never fitted to GPU output:
    C_target = ceil(d / 256)   rows a thread accumulates into its partial sums (one fma per row and sum)
             + 6               butterfly steps of the wave sum
             + 4               waves summed in wave order
             + 2 RPAD          the two triangular contractions gg = G we and h = G'gg, at most RPAD terms each
             + RPAD            the RPAD-term dot of a row of Wd with h
             + 16              the roundings of the inputs (e = x - mean, a e, exp(-tau), tau / 3, 2 tau / 9), the final multiply-adds,
                               corr = sum gg^2 and the last subtractions
Below the smallest normal double a result has lost its relative precision (e^-tau underflows for tau > 708 where long double does not):
every bound carries the absolute term TINY = 2^-1022.
  Gaussian family (e = x - mean, RPAD = 0, 8, 16 for r = 0, r <= 8, r <= 16):
    lp  = offset - (qa - corr) / 2          S_lp  = |offset| + (sum a e^2 + | |G| |Wd|'|e| |^2) / 2
    g_i = -(a_i e_i - Wd[i, :] h)            S_g,i = a_i |e_i| + |Wd[i, :]| (|G|'|G| |Wd|'|e|)
  Funnel (tau = x_0, ss = sum_{i >= 1} x_i^2):
    lp  = -((tau / 3)^2 + (d - 1) tau + e^-tau ss) / 2        S_lp  = ((tau / 3)^2 + (d - 1) |tau| + e^-tau ss) / 2
    g_0 = -(2 tau / 9 + (d - 1) - e^-tau ss) / 2              S_g,0 = (2 |tau| / 9 + (d - 1) + e^-tau ss) / 2
    g_i = -e^-tau x_i                                          S_g,i = e^-tau |x_i|
"""
import numpy as np

import hmc_reference as H
import scan_reference as sr

LD = sr.LD
EPS = sr.EPS64
TINY = 2.0 ** -1022               # the smallest normal double
ROUNDS_CAP = 1024                 # HM_FUSED_ROUNDS (pathfinder.jl_amd/csrc/hmc_rows.h)


def rpad_of(tg):
    r = getattr(tg, "r", 0)
    return 0 if (tg.kind == 1 or r == 0) else (8 if r <= 8 else 16)


def c_target(d, rpad):
    return -(-d // 256) + 6 + 4 + 2 * rpad + rpad + 16


def target_tag(tg):
    """the <f|g0|g8|g16> of the plan counter hmc_fused:<KPAD>:<res|stream>:<..>"""
    return "f" if tg.kind == 1 else "g%d" % rpad_of(tg)


def plan_name(tg, d, kpad):
    return "hmc_fused:%d:%s:%s" % (kpad, "res" if H.resident(d, kpad) else "stream", target_tag(tg))


def target_ld(tg, x, fault=None):
    """(lp, S_lp, g, S_g) in long double at the point x (d,).  fault (the CPU test: the checker must reject each): "lowrank_sign" adds the
    low-rank term of the gradient instead of subtracting it, "funnel_g0" drops the e^-tau ss term of g_0"""
    x = np.asarray(x, dtype=LD)
    d = len(x)
    if tg.kind == 1:
        tau = x[0]
        ee = np.exp(-tau)
        ss = np.sum(x[1:] ** 2)
        lp = ((tau / 3) ** 2 + (d - 1) * tau + ee * ss) / -2
        S = ((tau / 3) ** 2 + (d - 1) * abs(tau) + ee * ss) / 2
        g = -ee * x
        g[0] = -(2 * tau / 9 + (d - 1) - (0 if fault == "funnel_g0" else ee * ss)) / 2
        Sg = ee * np.abs(x)
        Sg[0] = (2 * abs(tau) / 9 + (d - 1) + ee * ss) / 2
        return lp, S, g, Sg
    mean, a = np.asarray(tg.mean, dtype=LD), np.asarray(tg.a, dtype=LD)
    e = x - mean
    ea = np.abs(e)
    q, Sq = np.sum(a * e * e), np.sum(a * ea * ea)
    g, Sg = a * e, a * ea
    corr = Sc = LD(0)
    if tg.r:
        Wd = np.asarray(tg.Wd, dtype=LD).reshape(d, -1)[:, :tg.r]
        G = np.tril(np.asarray(tg.G, dtype=LD).reshape(tg.r, tg.r))
        gg = G @ (Wd.T @ e)
        ga = np.abs(G) @ (np.abs(Wd).T @ ea)
        corr, Sc = np.sum(gg * gg), np.sum(ga * ga)
        low = Wd @ (G.T @ gg)
        g = g + low if fault == "lowrank_sign" else g - low
        Sg = Sg + np.abs(Wd) @ (np.abs(G).T @ ga)
    off = LD(tg.offset)
    return off - (q - corr) / 2, abs(off) + (Sq + Sc) / 2, -g, Sg


def target_ratios(tg, X, lp, g, fault=None):
    """largest |value - ref| / (C_target eps S) of recorded evaluations: X (n, d) points, lp (n,), g (n, d) -> (ratio of lp, ratio of g).
    Rows with a non-finite recorded value are left out (the transition's checker demands that they are divergent)."""
    d = X.shape[1]
    C = c_target(d, rpad_of(tg))
    rl = rg = 0.0
    for i in range(X.shape[0]):
        if not (np.isfinite(lp[i]) and np.all(np.isfinite(g[i]))):
            continue
        l, S, gr, Sg = target_ld(tg, X[i], fault)
        with np.errstate(all="ignore"):
            bl, bg = C * EPS * S + TINY, C * EPS * Sg + TINY
            el, eg = abs(LD(lp[i]) - l), np.abs(np.asarray(g[i], dtype=LD) - gr)
            rl = max(rl, float(el / bl) if bl > 0 else (np.inf if el > 0 else 0.0))
            rg = max(rg, float(np.max(np.where(bg > 0, eg / np.where(bg > 0, bg, 1), np.where(eg > 0, np.inf, 0)))))
    return rl, rg


# ---- the grid of tests/test_gpu_hmc_fused_steps.py (the CPU test runs the same cases on the mirror): (d, J, target name) -------------
GRID_T, GRID_LF, GRID_K = 4, 3, 3
GRID = ([(64, J, tn) for J in (2, 4, 6, 8, 10, 16, 32) for tn in ("gauss", "funnel")]            # all seven paddings
        + [(5, 10, tn) for tn in ("gauss", "funnel")]                                             # d < KPAD
        + [(257, 6, tn) for tn in ("diag", "lowrank12", "funnel")]                                # one row beyond a full sweep; RPAD 0 and 16
        + [(1600, 6, "funnel"), (1601, 6, "funnel")]                                              # the two sides of pf_hmc_resident at KPAD 12
        + [(320, 32, "gauss")])                                                                   # KPAD 64 streamed


def case_id(case):
    return "%s-d%d-J%d" % (case[2], case[0], case[1])


def grid_target(pfmi, tn, d):
    if tn == "diag":
        return pfmi.t_diag(d)
    if tn == "lowrank12":
        return pfmi.t_lowrank(d, r=12, seed=2, wscale=2.0 / np.sqrt(d))
    return H.grid_target(pfmi, tn, d)


def grid_path_x0(pfmi, tn, d):
    return H.grid_path_x0(pfmi, "funnel" if tn == "funnel" else "gauss", d)


def grid_plans(pfmi):
    return {plan_name(grid_target(pfmi, tn, d), d, H.kpad_for(J)) for d, J, tn in GRID}


# the two shapes of the bit-identity tests (K = 4, Lf = 5, T = 40; adaptive: W = 25, T = 15)
BIT_CASES = ((64, 6, "gauss"), (257, 6, "funnel"))
BIT_K, BIT_LF, BIT_T, BIT_W, BIT_TA = 4, 5, 40, 25, 15
BIT_CAPS = (None, 1, 7)           # the default cap, the rounds schedule, and a cap that does not divide 201 and cuts trajectories


# ---- what the GPU tests share --------------------------------------------------------------------------------------------------------
def set_round_cap(pfmi, cap):
    """the test hook PFMI_HMC_FUSED_ROUNDS (include/pfmi.h: pfmi_debug_set); None: the library's own cap"""
    L = pfmi._lib.lib()
    assert L.pfmi_debug_set(b"PFMI_HMC_FUSED_ROUNDS", None if cap is None else str(int(cap)).encode()) == 0


def setup_chains(pfmi, eng, case, K=GRID_K):
    """The chains of tests/test_gpu_hmc_steps.py on the built-in target itself: one path optimised by the device L-BFGS (which takes a
    history of at most 16: a longer one is fitted from the trace of 16), fitted with history_length J; the metrics are the fits of the
    path's first point (j_eff = 0), of an early point with 0 < j_eff < J and of the best fit (repeated beyond three chains); every
    chain starts at the best fit's trace point and steps by 0.4, 1, 2.2 (then 1) times d^(-1/4).  Returns (tg, pts, x0, eps, seeds, jeff)."""
    from helpers import fit_seeds
    d, J, tn = case
    tg = grid_target(pfmi, tn, d)
    eng.set_target(tg)
    npts = eng.optimize_batch(grid_path_x0(pfmi, tn, d), min(J, 16), 40, 1e-8)
    eng.fit_batch(J)
    status, jeff, _, _ = eng.fit_status()
    P = int(npts[0])
    _, _, best = eng.elbo_batch(32, fit_seeds(P, 5))
    p_best = int(best[0])
    early = [p for p in range(1, P) if status[p] == 0 and 0 < jeff[p] < J]
    assert status[0] == 0 and jeff[0] == 0 and early and status[p_best] == 0, (case_id(case), status[:4], jeff[:4], p_best)
    pts = np.array(([0, early[0], p_best] + [p_best] * K)[:K], dtype=np.int64)
    th, _, _ = eng.get_trace(0)
    x0 = np.asfortranarray(np.repeat(th[p_best][:, None], K, axis=1))
    eps = np.array((list(H.EPS_MULT) + [1.0] * K)[:K]) * d ** -0.25
    seeds = np.asarray(pfmi.hostrng.rand_u64(9000 + 7 * d + J, np.arange(K, dtype=np.uint64), 9), dtype=np.uint64)
    return tg, pts, x0, eps, seeds, jeff
