"""Reference of ChEES-HMC (pathfinder.jl_amd/csrc/adapt.h: the rule; include/pfmi.h: pfmi_chees_enqueue).  Not collected by pytest; used
by tests/test_chees_reference_cpu.py and tests/test_gpu_chees.py.

`halton`, `leapfrog`   the jitter and the leapfrog count of transition t in float64: exact statements, compared with `==`.
`update_ld`            one cross-chain update in np.longdouble from (x, x', u', a), the state and h; also the error budget of a float64
                       evaluation of it (below).  `replay_ld` iterates it over a trace of recorded updates, the step-size part being
                       adapt_reference.replay_ld on the harmonic means.
`bound`                what a float64 implementation may deviate from replay_ld: per update the absolute bound of g and the relative
                       bounds of the next tau and eps, and those of the sampling values.
`mirror`               a float64 NumPy statement of a whole run of K chains (the transition of hmc_reference.mirror, the update of
                       `update_np`); `fault=` injects one wrong step into the update.

The bound.  u = 2^-53, one rounding of relative size u per operation.  A sum of n terms costs n roundings whatever its order (the device's
block sums and the host's sequential loop are both covered), so with S| | the same sum over absolute values:
  A, xbar      K adds and a division:                    |dA| <= K u A,   e_i = (K + 1) u sum_k |x_k,i| / K
  xbar'        K fused multiply-adds, A, a division:     e'_i = (2 K + 2) u sum_k a_k |x'_k,i| / A
  p, q, r      a difference dx_i = x_i - xbar_i carries delta_i = u |dx_i| + e_i; its square 2 |dx_i| delta_i + delta_i^2; the d-term sum
               (d + 2) u sum_i (|dx_i| + delta_i)^2.  q likewise with e'; r with (|dx'_i| + delta'_i) |u'_i|.
  S            = sum_k a_k (q_k - p_k) r_k: the errors of p, q, r propagated (their product included: p, q and r may all be 0 exactly),
               4 roundings per term and K for the sum
  g            = (h tau) S / A: |dg| <= |g| (rho_tau + (K + 4) u) + |h tau / A| dS, rho_tau the relative error tau carries
  hm           = K / sum_k 1 / a_k: (K + 3) u relative; the dual averaging is linear in its statistic with weights that sum to at most 1, so
               le carries (sqrt(m) / gamma) (K + 3) u on top of adapt_reference.bound
  s, b         s' = 0.95 s + 0.05 g^2: ds' = 0.95 ds + 0.1 |g| dg + dg^2 + 4 u s';  b' = 0.95 b: 2 u relative per update
  lt           the step 0.025 g / D, D = sqrt(s / (1 - b)) + 1e-8 >= 1e-8: |dstep| <= 0.05 dg / D + |step| (dD / D + 3 u);
               dlt = rho_tau + u |log tau| + dstep + u |lt|
  ltb          as leb in adapt_reference: dltb' = w dlt + (1 - w) dltb + 10 u max_j |lt_j|
  tau+         the clamp is 1-Lipschitz in the logarithms of its three arguments: rho_tau+ = max(dlt, rho_eps+) + 3 u
Nothing here is fitted to the code under test."""
import ctypes as C

import numpy as np

import adapt_reference as A
import hmc_reference as H

LD = H.LD
U = 2.0 ** -53
CLAMPED, KEPT_TRAJ = 8, 16
SEED_BASE = 777                   # the sampling case's seed base (profiles/chees.md records the mirror's worst ratio under it)


def halton(t, fault=None):
    """the base-2 radical inverse of t + 1, exactly (a dyadic rational with at most 32 bits); fault "halton_t": of t"""
    n, out, w = int(t) + (0 if fault == "halton_t" else 1), 0.0, 0.5
    assert 0 <= n < 2 ** 32
    while n:
        out += w * (n & 1)
        n >>= 1
        w *= 0.5
    return out


def leapfrog(t, tau, eps, Lmax, fault=None):
    """(L_t, clamped) in float64: n = ceil((h tau) / eps), one rounding each"""
    n = np.ceil((np.float64(halton(t, fault)) * np.float64(tau)) / np.float64(eps))
    clamped = bool(n > Lmax)
    if not n >= 1:
        return 1, clamped
    return (int(Lmax) if clamped else int(n)), clamped


def init_state(eps0, tau0, delta, dtype=LD):
    """the state before the first update; err: the error budget carried forward"""
    f = dtype
    return {"eps": f(eps0), "tau": f(tau0 if tau0 > 0 else eps0), "s": f(0), "b": f(1), "ltb": f(0), "m": 0, "status": 0,
            "err": {"tau": 0.0, "s": 0.0, "b": 0.0, "ltb": 0.0, "ltmax": 0.0}}


def _sums(x, xp, u, a, f):
    """A, xbar, xbar', p, q, r and (for f = LD) their error budgets"""
    K, d = x.shape
    x, a = np.asarray(x, dtype=f), np.asarray(a, dtype=f)
    live = np.asarray(a) != 0
    xl, ul, al = np.asarray(xp[live], dtype=f), np.asarray(u[live], dtype=f), a[live]
    Asum = al.sum() if live.any() else f(0)
    xb = x.sum(axis=0) / f(K)
    with np.errstate(all="ignore"):
        xbp = (al[:, None] * xl).sum(axis=0) / Asum
    dx = x - xb
    p = (dx * dx).sum(axis=1)
    q, r = np.zeros(K, dtype=f), np.zeros(K, dtype=f)
    dp = xl - xbp
    q[live], r[live] = (dp * dp).sum(axis=1), (dp * ul).sum(axis=1)
    e = (K + 1) * U * np.abs(x).sum(axis=0) / K
    with np.errstate(all="ignore"):
        ep = (2 * K + 2) * U * (al[:, None] * np.abs(xl)).sum(axis=0) / Asum
    dl, dlp = U * np.abs(dx) + e, U * np.abs(dp) + ep
    Ep = (2 * np.abs(dx) * dl + dl * dl + (d + 2) * U * (np.abs(dx) + dl) ** 2).sum(axis=1)
    Eq, Er = np.zeros(K, dtype=f), np.zeros(K, dtype=f)
    Eq[live] = (2 * np.abs(dp) * dlp + dlp * dlp + (d + 2) * U * (np.abs(dp) + dlp) ** 2).sum(axis=1)
    Er[live] = (dlp * np.abs(ul) + (d + 2) * U * (np.abs(dp) + dlp) * np.abs(ul)).sum(axis=1)
    return Asum, live, p, q, r, Ep, Eq, Er


def update_ld(st, x, xp, u, a, h, Lmax, eps_next, rho_eps, last=False):
    """One update in long double.  st: the state (init_state / the previous call's); eps_next, rho_eps: the step size after the update
    from the dual-averaging replay and its relative bound.  Returns (new state, {"g", "hm", "dg", "kept"}): dg the absolute bound of g,
    the new state's err the bounds carried forward."""
    K, d = np.shape(x)
    f = LD
    Asum, live, p, q, r, Ep, Eq, Er = _sums(np.asarray(x), np.asarray(xp), np.asarray(u), np.asarray(a), f)
    al = np.asarray(a, dtype=f)
    err = dict(st["err"])
    tau = st["tau"]
    with np.errstate(all="ignore"):
        terms = al * ((q - p) * r)
        S = terms[live].sum() if live.any() else f(0)
        g = (f(h) * tau) * S / Asum
        hm = f(0) if not live.all() else f(K) / (1 / al).sum()
        ES = (al * ((Eq + Ep) * (np.abs(r) + Er) + (np.abs(q) + np.abs(p)) * Er))[live].sum() + (K + 4) * U * (al * (np.abs(q) + np.abs(p)) * np.abs(r))[live].sum()
        dg = abs(g) * (err["tau"] + (K + 4) * U) + abs(f(h) * tau / Asum) * ES
    new = {"m": st["m"] + 1, "status": st["status"], "eps": f(eps_next)}
    lt = np.log(tau)
    dlt = err["tau"] + U * abs(float(lt))
    kept = not (Asum > 0 and np.isfinite(g))
    if kept:
        new["s"], new["b"] = st["s"], st["b"]
        new["status"] |= KEPT_TRAJ
        dg = 0.0
    else:
        dg = float(dg)
        new["s"] = f(95) / 100 * st["s"] + f(5) / 100 * g * g
        new["b"] = f(95) / 100 * st["b"]
        err["s"] = 0.95 * err["s"] + 0.1 * abs(float(g)) * dg + dg * dg + 4 * U * float(new["s"])
        err["b"] = err["b"] + 2 * U
        one_b = 1 - new["b"]
        rel_1b = (float(new["b"]) * err["b"] + U) / float(one_b)
        root = np.sqrt(new["s"] / one_b)
        D = root + f(1) / f(10 ** 8)
        dD = float(root) * (0.5 * ((err["s"] / float(new["s"]) if new["s"] > 0 else 0.0) + rel_1b + U) + U) + U * float(D)
        if new["s"] > 0 and err["s"] >= float(new["s"]):         # s itself is within its own error of 0: the root may be anything up to sqrt(2 ds / (1 - b))
            dD += float(np.sqrt(f(2 * err["s"]) / one_b))
        step = f(25) / 1000 * g / D
        dstep = 0.05 * dg / float(D) + abs(float(step)) * (dD / float(D) + 3 * U)
        lt = lt + step
        dlt += dstep + U * abs(float(lt))
    mm = f(new["m"])
    w = 1 / (np.sqrt(mm) * np.sqrt(np.sqrt(mm)))
    new["ltb"] = w * lt + (1 - w) * st["ltb"]
    err["ltmax"] = max(err["ltmax"], abs(float(lt)))
    err["ltb"] = float(w) * dlt + (1 - float(w)) * err["ltb"] + 10 * U * err["ltmax"]
    src, dsrc = (new["ltb"], err["ltb"]) if last else (lt, dlt)
    new["tau"] = min(max(np.exp(src), new["eps"]), f(Lmax) * new["eps"])
    err["tau"] = max(dsrc, rho_eps) + 3 * U
    new["err"] = err
    return new, {"g": g, "hm": hm, "dg": dg, "kept": kept, "dlt": dlt}


def harmonic_means(acc):
    """hm of every update of a trace acc (W, K), in long double"""
    out = []
    for a in np.asarray(acc):
        al = np.asarray(a, dtype=LD)
        out.append(LD(0) if np.any(a == 0) else LD(len(a)) / (1 / al).sum())
    return np.array(out, dtype=LD)


def eps_replay(eps0, delta, hms, K):
    """(eps after every update [W] with the sampling value last, their relative bounds): adapt_reference's replay and bound on the harmonic
    means, plus what the error of a float64 harmonic mean adds"""
    W = len(hms)
    be, bb, re, rb = A.bound(eps0, delta, hms)
    extra = np.sqrt(np.arange(1, W + 1)) / A.GAMMA * (K + 3) * U
    eps = [re[m + 1] for m in range(W - 1)] + [rb[W - 1]]
    rho = [be[m] + extra[m] for m in range(W - 1)] + [bb[W - 1] + extra[W - 1]]
    return eps, rho


def replay_ld(eps0, tau0, delta, Lmax, xs, xps, us, acc, t_first=0):
    """the updates after warm-up transitions t_first .. t_first + W - 1 (the last one ends the warm-up) from their recorded inputs
    xs, xps, us (W, K, d) and acc (W, K).  Returns a list of per-update dicts {"tau" (used), "g", "dg", "hm", "tau_next", "rho_tau",
    "eps_next", "rho_eps", "kept"}."""
    W, K = np.shape(acc)
    eps, rho = eps_replay(eps0, delta, harmonic_means(acc), K)
    st = init_state(eps0, tau0, delta)
    out = []
    for t in range(W):
        tau = st["tau"]
        st, o = update_ld(st, xs[t], xps[t], us[t], acc[t], halton(t_first + t), Lmax, eps[t], rho[t], last=t == W - 1)
        o.update(tau=tau, tau_next=st["tau"], rho_tau=st["err"]["tau"], eps_next=st["eps"], rho_eps=rho[t])
        out.append(o)
    return out


def ratios(rep, g, tau_next, eps_next):
    """the largest error / bound of g, of the next tau and of the next eps over the updates of replay_ld's `rep`"""
    qg = qt = qe = 0.0
    for t, o in enumerate(rep):
        if not o["kept"]:
            err = abs(float(LD(g[t]) - o["g"]))
            qg = max(qg, np.inf if not np.isfinite(err) else err / o["dg"] if o["dg"] > 0 else (np.inf if err > 0 else 0.0))
        qt = max(qt, abs(float(LD(tau_next[t]) / o["tau_next"] - 1)) / o["rho_tau"])
        qe = max(qe, abs(float(LD(eps_next[t]) / o["eps_next"] - 1)) / o["rho_eps"])
    return qg, qt, qe


def check_run(res, eps0, tau0, delta, Lmax):
    """A whole run's record (the mirror's, or the GPU's put into the mirror's keys) against the rule: returns (L trace exact, largest
    error / bound of g, of tau and of eps): the leapfrog counts are the rule applied in float64 to the recorded (tau, eps); from the
    recorded update inputs the long-double replay gives g, the tau and eps of every later transition and the sampling values."""
    W = len(res["tau_trace"])
    nl = np.asarray(res["n_leapfrog"])
    tau_t = list(res["tau_trace"]) + [res["traj_length"]] * (len(nl) - W)
    eps_t = list(res["eps_trace"]) + [res["step_size"]] * (len(nl) - W)
    l_ok = all(int(nl[t]) == leapfrog(t, tau_t[t], eps_t[t], Lmax)[0] for t in range(len(nl)))
    if W == 0:
        return l_ok, 0.0, 0.0, 0.0
    x, xp, u = res["updates"]
    rep = replay_ld(eps0, tau0, delta, Lmax, x, xp, u, res["accept_trace"])
    return (l_ok,) + ratios(rep, res["grad_trace"], tau_t[1:W + 1], eps_t[1:W + 1])


# ---- the float64 statement of the update and of a whole run ------------------------------------------------------------------------------
def update_np(st, x, xp, u, a, h, Lmax, last=False, fault=None):
    """one update in float64 NumPy on st = {"eps", "tau", "s", "b", "ltb", "da": adapt state of pfmi.hmc, "status"}; returns (g, hm)"""
    from pfmi.hmc import dual_averaging_update
    x, xp, u, a = (np.asarray(v, dtype=np.float64) for v in (x, xp, u, a))
    K, d = x.shape
    live = a != 0
    al = a[live]
    with np.errstate(all="ignore"):
        Asum = np.float64(al.sum() if live.any() else 0.0)
        xb = x.sum(axis=0) / K
        xbp = xp[live].sum(axis=0) / max(int(live.sum()), 1) if fault == "unweighted_mean" else (al[:, None] * xp[live]).sum(axis=0) / Asum
        p = ((x - xb) ** 2).sum(axis=1)
        dp = xp[live] - xbp
        q, r = (dp * dp).sum(axis=1), (dp * u[live]).sum(axis=1)
        S = np.float64((al * ((q - p[live]) * r)).sum() if live.any() else 0.0)
        g = ((1.0 if fault == "no_jitter" else h) * (1.0 if fault == "grad_wrt_tau" else st["tau"])) * S / Asum
        hm = a.mean() if fault == "arithmetic_mean" else (0.0 if not live.all() else K / (1.0 / al).sum())
        st["da"], e1, ebar = dual_averaging_update(st["da"], hm, st["delta"])
        cand = float(ebar if last else e1)
        if cand > 0 and np.isfinite(cand):
            st["eps"] = cand
        else:
            st["status"] |= A.KEPT_STEP
        lt = np.log(st["tau"])
        if Asum > 0 and np.isfinite(g):
            st["s"] = 0.95 * st["s"] + 0.05 * (g * g)
            st["b"] = 0.95 * st["b"]
            lt = lt + 0.025 * g / (np.sqrt(st["s"] / (1.0 - st["b"])) + 1e-8)
        else:
            st["status"] |= KEPT_TRAJ
        m = st["da"][0]
        w = 1.0 / (np.sqrt(m) * np.sqrt(np.sqrt(m)))
        st["ltb"] = w * lt + (1.0 - w) * st["ltb"]
        te = float(np.exp(st["ltb"] if last else lt))
        if te > 0 and np.isfinite(te):
            st["tau"] = min(max(te, st["eps"]), Lmax * st["eps"])
        else:
            st["status"] |= KEPT_TRAJ
    return float(g), float(hm)


def np_state(eps0, tau0, delta):
    from pfmi.hmc import dual_averaging_init
    return {"eps": float(eps0), "tau": float(tau0 if tau0 > 0 else eps0), "s": 0.0, "b": 1.0, "ltb": 0.0, "da": dual_averaging_init(np.float64(eps0)),
            "delta": delta, "status": 0}


def mirror(Ms, logp_and_grad, x0, seeds, eps0, tau0, Lmax, W, T, delta=0.651, fault=None):
    """K chains (metrics Ms[k], starts x0 (d, K), seeds) through W warm-up and T sampling transitions: the transition of
    hmc_reference.mirror with the shared eps and L_t, the update of update_np.  Returns {"draws" (T, K, d), "accept_prob", "divergent" (T, K),
    "eps_trace", "tau_trace", "grad_trace", "hmean_trace" (W,), "accept_trace" (W, K), "n_leapfrog" (W + T,), "step_size", "traj_length",
    "status", "updates": (x, xp, u) (W, K, d)}."""
    K = len(seeds)
    d = Ms[0].d
    x = [np.array(x0[:, k], dtype=np.float64) for k in range(K)]
    st = np_state(eps0, tau0, delta)
    out = {k: [] for k in ("draws", "accept_prob", "divergent", "eps_trace", "tau_trace", "grad_trace", "hmean_trace", "accept_trace", "n_leapfrog")}
    ux, uxp, uu = [], [], []
    with np.errstate(all="ignore"):
        lp, wg = [0.0] * K, [None] * K
        for k in range(K):
            l, g = logp_and_grad(x[k])
            lp[k], wg[k] = float(l), Ms[k].R(np.asarray(g, dtype=np.float64))
        for t in range(W + T):
            eps = st["eps"]
            Lf, cl = leapfrog(t, st["tau"], eps, Lmax, fault)
            if cl:
                st["status"] |= CLAMPED
            out["n_leapfrog"].append(Lf)
            xs, xps, us, acc, divs = [], [], [], [], []
            for k in range(K):
                M = Ms[k]
                v = H.momentum(seeds[k], d, t)
                H0 = -lp[k] + 0.5 * float(v @ v)
                v = v + 0.5 * eps * wg[k]
                xt = x[k] + eps * M.L(v)
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
                xs.append(x[k].copy()); xps.append(xt.copy()); us.append(M.L(v)); acc.append(a); divs.append(int(div))
                if H.accept_uniform(seeds[k], t) < a:
                    x[k], lp[k], wg[k] = xt.copy(), lpt, wt
            if t < W:
                out["eps_trace"].append(eps); out["tau_trace"].append(st["tau"]); out["accept_trace"].append(acc)
                ux.append(xs); uxp.append(xps); uu.append(us)
                g, hm = update_np(st, xs, xps, us, acc, halton(t, fault), Lmax, last=t == W - 1, fault=fault)
                out["grad_trace"].append(g); out["hmean_trace"].append(hm)
            else:
                out["draws"].append(np.array(x)); out["accept_prob"].append(acc); out["divergent"].append(divs)
    res = {k: np.array(v) for k, v in out.items()}
    res.update(step_size=st["eps"], traj_length=st["tau"], status=st["status"], updates=(np.array(ux), np.array(uxp), np.array(uu)))
    return res


# ---- the host build ------------------------------------------------------------------------------------------------------------------------
def host_state(eps0, tau0, delta):
    from pfmi._lib import CheesState
    return CheesState(step_size=eps0, traj_length=tau0 if tau0 > 0 else eps0, s=0.0, b=1.0, ltb=0.0, hbar=0.0, leb=0.0, mu=float(np.log(10.0 * eps0)),
                      delta=delta, m=0, status=0, grad=0.0, hmean=0.0)


def host_update(lib, st, x, xp, u, a, h, Lmax, last=False):
    """pfmi_host_chees_update on the CheesState st (updated in place); returns its code"""
    dp = C.POINTER(C.c_double)
    arr = [np.ascontiguousarray(v, dtype=np.float64) for v in (x, xp, u, a)]
    K, d = arr[0].shape
    return lib.pfmi_host_chees_update(K, d, *[v.ctypes.data_as(dp) for v in arr], C.c_double(h), int(Lmax), 1 if last else 0, C.byref(st))


def host_leapfrog(lib, t, tau, eps, Lmax):
    cl = C.c_int32(0)
    L = lib.pfmi_host_chees_leapfrog(int(t), float(tau), float(eps), int(Lmax), C.byref(cl))
    return L, bool(cl.value)


# ---- the cases of tests/test_gpu_chees.py --------------------------------------------------------------------------------------------------
# (d, J, target, W, T): the shapes of adapt_reference.BIT_CASES
BIT_CASES = [(d, J, tn, 12, 4) for d, J in ((5, 2), (64, 6), (257, 16)) for tn in ("gauss", "funnel")] + [(20000, 6, "gauss", 3, 1)]
BIT_LMAX = 16
SAMPLING_W, SAMPLING_T, SAMPLING_LMAX, SAMPLING_K = 150, H.SAMPLING_T, 64, H.SAMPLING_K
DELTA = 0.651


def sampling_seeds(pfmi):
    return np.asarray(pfmi.hostrng.rand_u64(SEED_BASE, np.arange(SAMPLING_K, dtype=np.uint64), 9), dtype=np.uint64)


def bit_case_id(case):
    return "%s-d%d-J%d" % (case[2], case[0], case[1])
