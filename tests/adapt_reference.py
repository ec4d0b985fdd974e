"""Reference of the device-resident warm-up (pathfinder.jl_amd/csrc/adapt.h; include/pfmi.h: pfmi_hmc_adapt_enqueue).  Not collected by
pytest; used by tests/test_adapt_reference_cpu.py and tests/test_gpu_adapt.py.

`replay_ld`     the update of include/pfmi.h in np.longdouble, from a sequence of acceptance statistics.
`replay_np`     pfmi.hmc.dual_averaging_update (the window route's float64 NumPy statement of the same rule) iterated on the sequence.
`floor`         a bound on the relative error of a float64 evaluation of the update, counted from its operations (below).
`bound`         what a float64 implementation may deviate from replay_ld, relatively: the larger of 8 x replay_np's own deviation on the same
                sequence (the project's rule for chain diagnostics: profiles/chain_diag_parity.md) and the floor.
`mirror`        a float64 statement of static HMC with the warm-up in front, built on hmc_reference's pieces.

The floor.  u = 2^-53, one rounding of relative size u per floating-point operation; m updates; g_m = sqrt(m) / gamma; S_m the recursion of
Hbar with every term replaced by its absolute value, S_m = (1 - 1/(m + t0)) S_{m-1} + |delta - a_t| / (m + t0), a majorant of |Hbar_m|.
  Hbar   A = 1 - 1/(m + t0) takes 2 roundings and its product 1; B = (delta - a)/(m + t0) takes 2 and the sum 1:
         E_m <= A E_{m-1} + 3 u S_m, and since every S_j A_{j+1} .. A_m <= S_m:  E_m <= 3 m u S_m
  mu     log(10 eps_0): one rounding of the product (an absolute u in the logarithm) and a logarithm good to one ulp: u + 2 u |mu|
  le     sqrt, the division by gamma, gamma's own representation and the product: 4 u g_m S_m; the subtraction: u |le|
         F_m = u (1 + 2 |mu| + |le_m| + g_m (3 m + 4) S_m)
  eps    exp is good to one ulp:  |eps_m / ref - 1| <= F_m + 2 u
  leb    w = 1 / (sqrt(m) sqrt(sqrt(m))) takes 4 roundings and acts on both terms, 1 - w one more, the two products and the sum 3; with
         Lmax_m = max_{j <= m} |le_j| >= |leb_j|:   G_m <= w F_m + (1 - w) G_{m-1} + 10 u Lmax_m,   |epsbar_m / ref - 1| <= G_m + 2 u
Nothing here is fitted to the code under test."""
import ctypes as C

import numpy as np

import hmc_reference as H

LD = H.LD
U = 2.0 ** -53
GAMMA, T0 = 0.05, 10.0
KEPT_STEP = 1                     # PFMI_ADAPT_KEPT_STEP


def replay_ld(eps0, delta, accept):
    """(eps [n + 1], eps_bar [n], le [n], S [n]) in long double: eps[0] = eps0, eps[m] = exp(le_m), eps_bar[m - 1] = exp(leb_m); S the
    absolute-value majorant of Hbar.  The keep-the-previous-step rule is NOT applied: the values are exact statements of the recursion."""
    a = np.asarray(accept, dtype=LD)
    n = len(a)
    mu = np.log(LD(10) * LD(eps0))
    hbar, leb, s = LD(0), LD(0), LD(0)
    eps, bar, les, ss = [LD(eps0)], [], [], []
    for t in range(n):
        m = LD(t + 1)
        q = m + LD(T0)
        hbar = (1 - 1 / q) * hbar + (LD(delta) - a[t]) / q
        s = (1 - 1 / q) * s + abs(LD(delta) - a[t]) / q
        sm = np.sqrt(m)
        le = mu - sm / (LD(5) / LD(100)) * hbar
        w = 1 / (sm * np.sqrt(sm))
        leb = w * le + (1 - w) * leb
        eps.append(np.exp(le)); bar.append(np.exp(leb)); les.append(le); ss.append(s)
    return np.array(eps, dtype=LD), np.array(bar, dtype=LD), np.array(les, dtype=LD), np.array(ss, dtype=LD)


def replay_np(eps0, delta, accept):
    """(eps [n + 1], eps_bar [n]) of pfmi.hmc.dual_averaging_update iterated in float64"""
    from pfmi.hmc import dual_averaging_init, dual_averaging_update
    st = dual_averaging_init(np.float64(eps0))
    eps, bar = [np.float64(eps0)], []
    with np.errstate(all="ignore"):
        for a in np.asarray(accept, dtype=np.float64):
            st, e, eb = dual_averaging_update(st, a, delta)
            eps.append(float(e)); bar.append(float(eb))
    return np.array(eps), np.array(bar)


def floor(eps0, delta, accept):
    """(floor of eps[1:], floor of eps_bar) as in the docstring"""
    _, _, le, S = replay_ld(eps0, delta, accept)
    n = len(le)
    mu = abs(float(np.log(LD(10) * LD(eps0))))
    fe, fb = np.zeros(n), np.zeros(n)
    G, Lmax = 0.0, 0.0
    for t in range(n):
        m = t + 1
        g = np.sqrt(m) / GAMMA
        F = U * (1 + 2 * mu + abs(float(le[t])) + g * (3 * m + 4) * float(S[t]))
        w = m ** -0.75
        Lmax = max(Lmax, abs(float(le[t])))
        G = w * F + (1 - w) * G + 10 * U * Lmax
        fe[t], fb[t] = F + 2 * U, G + 2 * U
    return fe, fb


def bound(eps0, delta, accept):
    """(bound of eps[1:], bound of eps_bar, the replay_ld values of both): relative deviations a float64 implementation may show"""
    re, rb, _, _ = replay_ld(eps0, delta, accept)
    ne, nb = replay_np(eps0, delta, accept)
    fe, fb = floor(eps0, delta, accept)
    with np.errstate(all="ignore"):
        de = np.abs(np.asarray(ne[1:], dtype=LD) / re[1:] - 1).astype(np.float64)
        db = np.abs(np.asarray(nb, dtype=LD) / rb - 1).astype(np.float64)
    return np.maximum(8 * de, fe), np.maximum(8 * db, fb), re, rb


def ratios(val_eps, val_bar, eps0, delta, accept, skip=None):
    """the largest |value / reference - 1| / bound over eps[1:] (entries where skip[m - 1] is set are left out) and over eps_bar (None: not
    looked at)"""
    be, bb, re, rb = bound(eps0, delta, accept)
    with np.errstate(all="ignore"):
        qe = (np.abs(np.asarray(val_eps, dtype=LD)[1:] / re[1:] - 1)).astype(np.float64) / be
        if skip is not None:
            qe = qe[~np.asarray(skip, dtype=bool)]
        out = [float(np.max(qe)) if len(qe) else 0.0]
        if val_bar is not None:
            out.append(float(np.max((np.abs(np.asarray(val_bar, dtype=LD) / rb - 1)).astype(np.float64) / bb)))
    return out


def host_dual_averaging(lib, eps0, delta, accept, rc=False):
    """pfmi_host_dual_averaging: (eps [n + 1], eps_bar [n]) (rc=True: only the return code)"""
    a = np.ascontiguousarray(accept, dtype=np.float64)
    n = len(a)
    eps, bar = np.full(n + 1, np.nan), np.full(n, np.nan)
    dp = C.POINTER(C.c_double)
    code = lib.pfmi_host_dual_averaging(C.c_int64(n), C.c_double(eps0), C.c_double(delta), a.ctypes.data_as(dp), eps.ctypes.data_as(dp),
                                        bar.ctypes.data_as(dp))
    if rc:
        return code
    assert code == 0, code
    return eps, bar


# ---- the float64 mirror of static HMC with the warm-up in front --------------------------------------------------------------------
def mirror(M, logp_and_grad, x0, seed, eps0, Lf, W, T, delta=0.8):
    """W warm-up transitions whose step size follows the update after every transition (float64, the keep-the-previous-step rule
    included), then T sampling transitions with exp(leb_W): the transition of hmc_reference.mirror, transition t using the momentum and
    the uniform of index t.  Returns {"draws" (T, d), "logp", "accept_prob", "divergent" (T,), "eps_trace", "accept_trace" (W,),
    "warm_divergent" (W,), "step_size", "status"}."""
    from pfmi.hmc import dual_averaging_init, dual_averaging_update
    d = M.d
    x = np.array(x0, dtype=np.float64)
    out = {k: [] for k in ("draws", "logp", "accept_prob", "divergent", "eps_trace", "accept_trace", "warm_divergent")}
    st = dual_averaging_init(np.float64(eps0))
    eps, status = float(eps0), 0
    with np.errstate(all="ignore"):
        lp, g = logp_and_grad(x)
        lp = float(lp)
        wg = M.R(np.asarray(g, dtype=np.float64))
        for t in range(W + T):
            v = H.momentum(seed, d, t)
            H0 = -lp + 0.5 * float(v @ v)
            v = v + 0.5 * eps * wg
            xt = x + eps * M.L(v)
            bad = False
            for i in range(1, Lf + 1):
                lpt, gt = logp_and_grad(xt)
                lpt, gt = float(lpt), np.asarray(gt, dtype=np.float64)
                wt = M.R(gt)
                bad = bad or not (np.isfinite(lpt) and np.all(np.isfinite(gt)))
                if i < Lf:
                    v = v + eps * wt
                    xt = xt + eps * M.L(v)
                else:
                    v = v + 0.5 * eps * wt
            H1 = -lpt + 0.5 * float(v @ v)
            dH = H1 - H0
            div = bad or not np.isfinite(H1) or dH > 1000.0
            a = 0.0 if div else min(1.0, float(np.exp(-dH)))
            if H.accept_uniform(seed, t) < a:
                x, lp, wg = xt.copy(), lpt, wt
            if t < W:
                out["eps_trace"].append(eps); out["accept_trace"].append(a); out["warm_divergent"].append(int(div))
                st, e1, ebar = dual_averaging_update(st, a, delta)
                cand = float(e1) if t + 1 < W else float(ebar)
                if cand > 0.0 and np.isfinite(cand):
                    eps = cand
                else:
                    status |= KEPT_STEP
            else:
                out["draws"].append(x.copy()); out["logp"].append(lp); out["accept_prob"].append(a); out["divergent"].append(int(div))
    res = {k: np.array(v) for k, v in out.items()}
    res["step_size"], res["status"] = eps, status
    return res


# ---- the cases of tests/test_gpu_adapt.py ------------------------------------------------------------------------------------------------
# bit equality with the plain calls: the shapes of hmc_reference.GRID that cover the column paddings 4, 12, 32, both targets and the
# streamed factor route, and the one padding that is no power of two (J = 10: KPAD 20) on the Gaussian; (d, J, target, W, T)
BIT_CASES = ([(d, J, tn, 12, 4) for d, J in ((5, 2), (64, 6), (257, 16)) for tn in ("gauss", "funnel")] + [(64, 10, "gauss", 12, 4)]
             + [(20000, 6, "gauss", 3, 1)])
BIT_LF, BIT_DEPTH = 3, 4
# the sampling case (hmc_reference.sampling_case): the warm-up the CPU test admits on the mirror, then the T of the plain sampling test
SAMPLING_W, SAMPLING_T = 150, H.SAMPLING_T


def bit_case_id(case):
    return "%s-d%d-J%d" % (case[2], case[0], case[1])
