"""Reference of the NUTS step kernel (pathfinder.jl_amd/csrc/nuts_kernel.hip).  Not collected by pytest; used by tests/test_gpu_nuts_steps.py
and tests/test_gpu_nuts.py and pinned on the CPU by tests/test_nuts_reference_cpu.py.

`mirror`     a float64 NumPy statement of the transition of include/pfmi.h (pfmi_nuts_enqueue): multinomial NUTS with the ITERATIVE tree
             builder (checkpoints), with the kernel's consumption of random numbers.  It returns what the kernel records: per round the
             closure's input X, its output (lp, g), the synchronised momentum v of the leaf the round finished and the event record; per
             transition x, lp, accept_prob, energy_error, divergent, tree_depth and n_leapfrog.  `fault=` injects one wrong step.
`recursive`  the textbook recursive builder of ONE transition (Hoffman & Gelman 2014 Algorithm 3 with Betancourt's generalised criterion):
             depth, leaf count and stop reason only -- what the checkpoint rule must reproduce.
`check`      a np.longdouble checker of a recording (the kernel's or the mirror's), TEACHER-FORCED: every round is replayed from the
             recording's own previous v, X and closure output; every decision is recomputed and compared exactly unless its margin is
             inside its bound (BORDERLINE: counted, the recording's decision is followed).

Bounds (eps = 2^-52: two unit roundoffs per counted step; C_apply, C_sum: hmc_reference's counts from the kernel's reduction map, which
nuts_kernel.hip shares pass for pass):
  v     a leaf's momentum is the previous leaf's (or the tree end's) recorded one plus two half kicks with wt = R g of the two rounds:
        |v - v_ref| <= C_apply eps S_v,  S_v = |v_prev| + (e/2) (S_R(|g_prev|) + S_R(|g|))
  X     X_next = base + dir e L(v + dir (e/2) wt): the half kick's error passes through L, then L's own roundings:
        |X - X_ref| <= 2 C_apply eps S_X,  S_X = |base| + e S_L(|v| + (e/2) S_R(|g|))
  H     |H - H_ref| <= C_sum eps (|lp| + |v|^2 / 2) =: b_H;  B_H of a leaf = b_H(root) + b_H(leaf) bounds lw = H0 - H
  logW  logaddexp is 1-Lipschitz in the sup norm of its inputs and each evaluation rounds by a few ulp of 1 + |value|:
        |logW - ref| <= max B_H + 8 eps m (1 + max |logW|) after m evaluations; a selection u < exp(a - b) is borderline when
        |log u - (a - b)| <= 2 max B_H + 16 eps (m + 1) (1 + |a| + |b|)
  dots  rho_sub . v and rho . v: the momentum sums carry at most one rounding per summand, each at most u S_i with S_i the sum of the
        summands' absolute values, and the dot product C_sum roundings:  |dot - ref| <= eps (C_sum + m + 2) sum_i S_i |v_i| with m the
        number of summands; a turn test is borderline inside that bound.
"""
import numpy as np

import hmc_reference as H

LD = H.LD
EPS = H.EPS
DIR_STREAM, TREE_STREAM, LEAF_STREAM = 4, 5, 6    # PF_RNG_STREAM_NUTS_* (pathfinder.jl_amd/csrc/pfmi_common.h)
DBL_MAX = H.DBL_MAX
MAXD = 10
EV_DIV, EV_SUB_TURN, EV_LEAF, EV_SUB_DONE, EV_TREE, EV_TREE_TURN, EV_MAX_DEPTH, EV_END = 1, 2, 4, 8, 16, 32, 64, 128
EVENT = np.dtype([("t", np.int32), ("j", np.int32), ("n", np.int32), ("dir", np.int32), ("leaf", np.int32), ("flags", np.int32),
                  ("H_leaf", np.float64), ("logW_s", np.float64), ("logW", np.float64), ("H0", np.float64)])


def _u64(seed, ctr, stream):
    import pfmi
    return int(np.asarray(pfmi.hostrng.rand_u64(int(seed), np.array([ctr], dtype=np.uint64), stream))[0])


def uniform(seed, ctr, stream):
    return (_u64(seed, ctr, stream) >> 11) * 2.0 ** -53


def direction(seed, t, j):
    return 1 if _u64(seed, 16 * t + j, DIR_STREAM) >> 63 else -1


def logaddexp(a, b):
    if a == -np.inf:
        return b
    if b == -np.inf:
        return a
    return max(a, b) + np.log1p(np.exp(-abs(a - b)))


def popcount(n):
    return bin(n).count("1")


def trailing_ones(n):
    c = 0
    while n & 1:
        n >>= 1
        c += 1
    return c


def pos(x):
    """the kernel's `x > 0` (a NaN is a turn)"""
    return bool(x > 0)


# ---- the float64 mirror ----------------------------------------------------------------------------------------------------------
def mirror(M, logp_and_grad, x0, seed, eps, max_depth, T, fault=None, momenta=None, directions=None):
    """T transitions of one chain from x0.  momenta / directions (test hooks): callables (t) -> v0 and (t, j) -> +-1 replacing the
    chain's generator.  Returns a recording (see `check`)."""
    d = M.d
    x = np.array(x0, dtype=np.float64)
    rec = {"x0": x.copy(), "X": [], "lp": [], "g": [], "v": [], "ev": [], "draws": [], "logp": [], "accept_prob": [], "energy_error": [],
           "divergent": [], "tree_depth": [], "n_leapfrog": [], "stop": []}

    def evaluate(xt):
        with np.errstate(all="ignore"):
            l, g = logp_and_grad(xt)
        rec["X"].append(np.array(xt)); rec["lp"].append(float(l)); rec["g"].append(np.array(g, dtype=np.float64))
        return float(l), np.asarray(g, dtype=np.float64)

    def event(t, j, n, dr, leaf, flags, Hl, lws, lw_, H0):
        e = np.zeros((), dtype=EVENT)
        e["t"], e["j"], e["n"], e["dir"], e["leaf"], e["flags"] = t, j, n, dr, leaf, flags
        e["H_leaf"], e["logW_s"], e["logW"], e["H0"] = Hl, lws, lw_, H0
        return e

    with np.errstate(all="ignore"):
        lp, g = evaluate(x)
        wg = M.R(g)
        rec["v"].append(np.zeros(d)); rec["ev"].append(event(-1, -1, -1, 0, 0, 0, 0.0, 0.0, 0.0, 0.0))
        for t in range(T):
            v0 = momenta(t) if momenta else H.momentum(seed, d, t)
            H0 = -lp + 0.5 * float(v0 @ v0)
            xe, ve, we = [x.copy(), x.copy()], [v0.copy(), v0.copy()], [wg.copy(), wg.copy()]
            xc, wc, lpc, Hc = x.copy(), wg.copy(), lp, H0
            rho, logW = v0.copy(), 0.0
            nleaf, sacc, stop, div = 0, 0.0, None, False
            j = 0
            while stop is None:
                dr = directions(t, j) if directions else direction(seed, t, j)
                if fault == "flip_dir":
                    dr = -dr
                e = 1 if dr > 0 else 0
                hk = 0.5 * dr * eps
                v = ve[e] + hk * we[e]
                X = xe[e] + dr * eps * M.L(v)
                rhos, logWs = np.zeros(d), -np.inf
                xs = ws = None
                lps = Hs = 0.0
                vck, rck = [None] * (MAXD + 1), [None] * (MAXD + 1)
                for n in range(1 << j):
                    lpt, gt = evaluate(X)
                    wt = M.R(gt)
                    vl = v + hk * wt
                    rhos = rhos + vl
                    imax, nchk = popcount(n >> 1), trailing_ones(n)
                    last = n == (1 << j) - 1
                    if n % 2 == 0:
                        at = imax - 1 if fault == "ck_index" and imax >= 1 else imax
                        vck[at], rck[at] = vl.copy(), rhos.copy()
                    Hl = -lpt + 0.5 * float(vl @ vl)
                    dH = Hl - H0
                    lw = dH if fault == "weight_sign" else -dH
                    bad = not (np.isfinite(lpt) and np.all(np.isfinite(gt)))
                    div = bool(bad or not np.isfinite(Hl) or dH > 1000.0)
                    sacc += 0.0 if div else min(1.0, float(np.exp(-dH)))
                    leaf = nleaf
                    nleaf += 1
                    flags = 0
                    turn = complete = False
                    if not div:
                        lws_new = logaddexp(logWs, lw)
                        sel = uniform(seed, 1024 * t + leaf, LEAF_STREAM) < np.exp(lw - lws_new)
                        logWs = lws_new
                        if sel:
                            xs, ws, lps, Hs = X.copy(), wt.copy(), lpt, Hl
                            flags |= EV_LEAF
                        for c in range(nchk):
                            if fault == "skip_check" and c > 0:
                                break
                            i = imax - c
                            if vck[i] is None:             # (only a faulty index rule reads a checkpoint that was never stored)
                                continue
                            rsub = (rhos - rck[i]) + vck[i]
                            if not pos(float(rsub @ vck[i])) or not pos(float(rsub @ vl)):
                                turn = True
                        if not turn and last:
                            complete = True
                            flags |= EV_SUB_DONE
                            if fault == "uniform_top":
                                tsel = uniform(seed, 16 * t + j, TREE_STREAM) < np.exp(logWs - logaddexp(logW, logWs))
                            else:
                                tsel = uniform(seed, 16 * t + j, TREE_STREAM) < np.exp(logWs - logW)
                            logW = logaddexp(logW, logWs)
                            if tsel:
                                xc, wc, lpc, Hc = xs.copy(), ws.copy(), lps, Hs
                                flags |= EV_TREE
                            rn = rho + rhos
                            fturn = not pos(float(rn @ vl)) or not pos(float(rn @ ve[1 - e]))
                            if fault != "stale_rho":
                                rho = rn
                            xe[e], ve[e], we[e] = X.copy(), vl.copy(), wt.copy()
                            if fturn:
                                flags |= EV_TREE_TURN
                                stop = "tree_turn"
                            if j + 1 >= max_depth:
                                flags |= EV_MAX_DEPTH
                                stop = stop or "max_depth"
                    if div:
                        flags |= EV_DIV
                        stop = "divergent"
                    elif turn:
                        flags |= EV_SUB_TURN
                        stop = "subtree_turn"
                    if stop:
                        flags |= EV_END
                    rec["v"].append(vl.copy())
                    rec["ev"].append(event(t, j, n, dr, leaf, flags, Hl, logWs, logW, H0))
                    if stop or complete:
                        break
                    v = vl + hk * wt
                    X = X + dr * eps * M.L(v)
                if stop is None:
                    j += 1
            x, wg, lp = xc, wc, lpc
            de = Hc - H0
            rec["draws"].append(x.copy()); rec["logp"].append(lp); rec["accept_prob"].append(sacc / nleaf)
            rec["energy_error"].append(de if np.isfinite(de) else DBL_MAX); rec["divergent"].append(int(div))
            rec["tree_depth"].append(j + 1); rec["n_leapfrog"].append(nleaf); rec["stop"].append(stop)
    for k_ in ("X", "g", "v", "draws"):
        rec[k_] = np.array(rec[k_])
    for k_ in ("lp", "logp", "accept_prob", "energy_error"):
        rec[k_] = np.array(rec[k_], dtype=np.float64)
    for k_ in ("divergent", "tree_depth", "n_leapfrog"):
        rec[k_] = np.array(rec[k_], dtype=np.int32)
    rec["ev"] = np.array(rec["ev"], dtype=EVENT)
    return rec


# ---- the textbook recursive builder ------------------------------------------------------------------------------------------------
def recursive(M, logp_and_grad, x, lp, wg, v0, eps, max_depth, directions):
    """one transition from (x, lp, wg = R grad) with momentum v0 and directions(j): (tree_depth, n_leapfrog, stop reason)"""
    H0 = -lp + 0.5 * float(v0 @ v0)
    count = [0]

    def leapfrog(s, dr):
        xs, vs, ws = s
        vh = vs + 0.5 * dr * eps * ws
        xn = xs + dr * eps * M.L(vh)
        with np.errstate(all="ignore"):
            l, g = logp_and_grad(xn)
        wn = M.R(np.asarray(g, dtype=np.float64))
        vn = vh + 0.5 * dr * eps * wn
        count[0] += 1
        Hn = -float(l) + 0.5 * float(vn @ vn)
        bad = not (np.isfinite(l) and np.all(np.isfinite(g)) and np.isfinite(Hn)) or Hn - H0 > 1000.0
        return (xn, vn, wn), bad

    def build(s, dr, depth):
        """(first state, last state, sum of momenta, stop reason or None) of 2^depth leaves grown from s"""
        if depth == 0:
            s1, bad = leapfrog(s, dr)
            return s1, s1, s1[1].copy(), ("divergent" if bad else None)
        f1, l1, r1, stop = build(s, dr, depth - 1)
        if stop:
            return f1, l1, r1, stop
        f2, l2, r2, stop = build(l1, dr, depth - 1)
        r = r1 + r2
        if stop:
            return f1, l2, r, stop
        if not pos(float(r @ f1[1])) or not pos(float(r @ l2[1])):
            return f1, l2, r, "subtree_turn"
        return f1, l2, r, None

    with np.errstate(all="ignore"):
        ends = [(x, v0, wg), (x, v0, wg)]
        rho = v0.copy()
        for j in range(max_depth):
            dr = directions(j)
            e = 1 if dr > 0 else 0
            _, last, r, stop = build(ends[e], dr, j)
            if stop:
                return j + 1, count[0], stop
            ends[e] = last
            rho = rho + r
            if not pos(float(rho @ ends[0][1])) or not pos(float(rho @ ends[1][1])):
                return j + 1, count[0], "tree_turn"
        return max_depth, count[0], "max_depth"


def gpu_recording(x0, path, got, stats, k, rounds=None):
    """chain k's recording from Engine.nuts_path(), Engine.hmc_get() and Engine.nuts_get_stats(): the rounds the chain was running in"""
    X, lp, g, v, ev = path
    n = int(np.sum(stats[1][k])) + 1 if rounds is None else rounds
    return {"x0": np.asarray(x0, dtype=np.float64), "X": X[:, k, :n].T, "lp": lp[k, :n], "g": g[:, k, :n].T, "v": v[:, k, :n].T, "ev": ev[:n, k],
            "draws": got["draws"][:, :, k].T, "logp": got["logp"][k], "accept_prob": got["accept_prob"][k],
            "energy_error": got["energy_error"][k], "divergent": got["divergent"][k], "tree_depth": stats[0][k], "n_leapfrog": stats[1][k]}


# ---- the long-double checker -------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def check(M, rec, seed, eps, max_depth, kpad, label=""):
    """teacher-forced long-double check of a recording of T transitions that started at transition 0.  Returns {"borderline", "decisions",
    "seen": set of what occurred, "margins": {quantity: max err / bound}}; raises Mismatch."""
    ML = M.astype(LD)
    d = M.d
    T = len(rec["logp"])
    Ca, Cs = H.c_apply(d, kpad), H.c_sum(d)
    e = LD(eps)
    marg = {"v": 0.0, "X": 0.0, "H": 0.0, "logW": 0.0, "a": 0.0}
    out = {"borderline": 0, "decisions": 0, "seen": set(), "margins": marg}
    Xr, gr, vr, lpr, ev = rec["X"], rec["g"], rec["v"], rec["lp"], rec["ev"]

    def need(cond, *what):
        if not cond:
            raise Mismatch((label,) + what)

    def close(q, val, ref, S, C, *what):
        err = np.abs(np.asarray(val, dtype=LD) - ref)
        bound = C * EPS * np.asarray(S, dtype=LD)
        with np.errstate(all="ignore"):
            m = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
        marg[q] = max(marg[q], m)
        need(m <= 1.0, q, m, *what)

    def decide(dev, ref, margin, bound, *what):
        """a decision of the recording against the reference's; inside the bound it is borderline and the recording's is followed"""
        out["decisions"] += 1
        if abs(float(margin)) <= float(bound):
            out["borderline"] += 1
            return bool(dev)
        need(bool(dev) == bool(ref), "decision", *what, float(margin), float(bound))
        return bool(ref)

    need(np.array_equal(Xr[0], rec["x0"]), "round 0 did not evaluate x0")
    need(len(lpr) == 1 + int(np.sum(rec["n_leapfrog"])), "rounds", len(lpr), int(np.sum(rec["n_leapfrog"])))
    x = np.asarray(rec["x0"], dtype=np.float64)
    lp = float(lpr[0])
    need(np.isfinite(lp) and np.all(np.isfinite(gr[0])), "non-finite start")
    wg, Swg = ML.R(gr[0]), ML.R_abs(np.abs(gr[0]))
    r = 0                                                   # the last round consumed
    for t in range(T):
        z = np.asarray(H.momentum(seed, d, t), dtype=LD)
        H0 = -LD(lp) + np.sum(z * z) / 2
        bH0 = Cs * EPS * (abs(LD(lp)) + np.sum(z * z) / 2)
        # both ends: (x, v, wt, S_wt) with x and v the recording's float64 values
        ends = [(x, z, wg, Swg), (x, z, wg, Swg)]
        cand = (x, lp, None, wg, Swg)                        # (x, lp, H of the device or None for the root, wt, S_wt)
        rho, Srho, mrho = z.copy(), np.abs(z), 1
        logW, nlse, BHmax, maxlw = LD(0), 0, LD(0), LD(0)
        nleaf, sacc, Bacc, stop, div_t = 0, LD(0), LD(0), False, 0
        j = 0
        while not stop:
            dr = direction(seed, t, j)
            out["seen"].add("dir+" if dr > 0 else "dir-")
            en = 1 if dr > 0 else 0
            xb, vb, wb, Swb = ends[en]                       # the state the next leapfrog step starts from
            rhos, Srhos, logWs = np.zeros(d, dtype=LD), np.zeros(d, dtype=LD), -LD(np.inf)
            scand = None
            ck = {}
            complete = False
            for n in range(1 << j):
                r += 1
                need(r < len(lpr), "the recording ends inside a tree", t, j, n)
                E = ev[r]
                need((int(E["t"]), int(E["j"]), int(E["n"]), int(E["dir"]), int(E["leaf"])) == (t, j, n, dr, nleaf), "event", r,
                     (int(E["t"]), int(E["j"]), int(E["n"]), int(E["dir"]), int(E["leaf"])), (t, j, n, dr, nleaf))
                fl = int(E["flags"])
                # ---- the drift that produced X[r], from the base state
                vh = np.asarray(vb, dtype=LD) + dr * e / 2 * wb
                close("X", Xr[r], np.asarray(xb, dtype=LD) + dr * e * ML.L(vh), np.abs(xb) + e * ML.L_abs(np.abs(vb) + e / 2 * Swb), 2 * Ca,
                      "round", r)
                g, lpt = gr[r], float(lpr[r])
                bad = not (np.isfinite(lpt) and np.all(np.isfinite(g)) and np.all(np.isfinite(Xr[r])))
                nleaf += 1
                if bad:
                    need(fl & EV_DIV and fl & EV_END, "a non-finite leaf must be divergent and end the transition", r)
                    out["seen"].add("divergent")
                    div_t, stop = 1, True
                    break
                wt, Swt = ML.R(g), ML.R_abs(np.abs(g))
                close("v", vr[r], vh + dr * e / 2 * wt, np.abs(vb) + e / 2 * (Swb + Swt), Ca, "round", r)
                vl = np.asarray(vr[r], dtype=LD)
                Hl = -LD(lpt) + np.sum(vl * vl) / 2
                bHl = Cs * EPS * (abs(LD(lpt)) + np.sum(vl * vl) / 2)
                close("H", E["H_leaf"], Hl, bHl / EPS, 1.0, "H_leaf", r)
                close("H", E["H0"], H0, bH0 / EPS, 1.0, "H0", r)
                dH, BH = Hl - H0, bH0 + bHl
                BHmax = max(BHmax, BH)
                if not np.isfinite(float(dH)):
                    need(fl & EV_DIV and fl & EV_END, "a non-finite energy must be divergent", r)
                    div = True
                else:
                    div = decide(fl & EV_DIV, dH > 1000, dH - 1000, BH, "divergent", r)
                if div:
                    need(fl & EV_END and not fl & (EV_LEAF | EV_SUB_DONE | EV_TREE | EV_SUB_TURN | EV_TREE_TURN | EV_MAX_DEPTH), "flags of a divergent leaf", r, fl)
                    out["seen"].add("divergent")
                    div_t, stop = 1, True
                    break
                a_ref = min(LD(1), np.exp(-dH))
                sacc += a_ref
                Bacc += a_ref * (BH + 8 * EPS * (1 + abs(dH))) + EPS
                lw = -dH
                maxlw = max(maxlw, abs(lw))
                rhos, Srhos = rhos + vl, Srhos + np.abs(vl)
                logWs_new = lw if logWs == -np.inf else max(logWs, lw) + np.log1p(np.exp(-abs(logWs - lw)))
                nlse += 1
                Blse = BHmax + 8 * EPS * nlse * (1 + maxlw + abs(logWs_new))
                Bsel = 2 * BHmax + 16 * EPS * (nlse + 1) * (1 + maxlw + abs(logWs_new))
                close("logW", E["logW_s"], logWs_new, Blse / EPS, 1.0, "logW_s", r)
                u = uniform(seed, 1024 * t + (nleaf - 1), LEAF_STREAM)
                a = lw - logWs_new
                sel = decide(fl & EV_LEAF, u < np.exp(a), (np.log(LD(u)) - a) if u > 0 else -np.inf, Bsel if u > 0 else 0, "leaf selection", r)
                logWs = logWs_new
                if sel:
                    scand = (np.asarray(Xr[r], dtype=np.float64), lpt, float(E["H_leaf"]), wt, Swt)
                # ---- the checkpoints
                imax, nchk = popcount(n >> 1), trailing_ones(n)
                m = n + 1
                if n % 2 == 0:
                    ck[imax] = (vl, rhos.copy())
                turn_ref, tmargin, tbound = False, LD(np.inf), LD(0)
                for c in range(nchk):
                    vc, rc = ck[imax - c]
                    rsub = rhos - rc + vc
                    for w_ in (vc, vl):
                        dot = np.sum(rsub * w_)
                        B = EPS * (Cs + m + 2) * np.sum(Srhos * np.abs(w_))
                        turn_ref = turn_ref or not dot > 0
                        if abs(dot) - B < tmargin - tbound:
                            tmargin, tbound = abs(dot), B
                turn = decide(fl & EV_SUB_TURN, turn_ref, tmargin, tbound, "sub-tree turn", r) if nchk else False
                need(nchk or not fl & EV_SUB_TURN, "a turn without a check", r)
                if turn:
                    need(fl & EV_END and not fl & (EV_SUB_DONE | EV_TREE | EV_TREE_TURN | EV_MAX_DEPTH), "flags of a turned sub-tree", r, fl)
                    out["seen"].add("subtree_turn")
                    stop = True
                    break
                if n == (1 << j) - 1:
                    complete = True
                    need(fl & EV_SUB_DONE, "a completed sub-tree is not merged", r, fl)
                    u = uniform(seed, 16 * t + j, TREE_STREAM)
                    a = logWs - logW
                    tsel = decide(fl & EV_TREE, u < np.exp(a), (np.log(LD(u)) - a) if u > 0 else -np.inf, Bsel + Blse if u > 0 else 0, "tree selection", r)
                    out["seen"].add("candidate_replaced" if tsel else "candidate_kept")
                    if tsel:
                        cand = scand
                    logW = max(logW, logWs) + np.log1p(np.exp(-abs(logW - logWs)))
                    nlse += 1
                    close("logW", E["logW"], logW, (Blse + 8 * EPS * (1 + abs(logW))) / EPS, 1.0, "logW", r)
                    rho, Srho, mrho = rho + rhos, Srho + Srhos, mrho + m
                    ends[en] = (np.asarray(Xr[r], dtype=np.float64), vl, wt, Swt)
                    fturn_ref, tmargin, tbound = False, LD(np.inf), LD(0)
                    for w_ in (np.asarray(ends[0][1], dtype=LD), np.asarray(ends[1][1], dtype=LD)):
                        dot = np.sum(rho * w_)
                        B = EPS * (Cs + mrho + 2) * np.sum(Srho * np.abs(w_))
                        fturn_ref = fturn_ref or not dot > 0
                        if abs(dot) - B < tmargin - tbound:
                            tmargin, tbound = abs(dot), B
                    fturn = decide(fl & EV_TREE_TURN, fturn_ref, tmargin, tbound, "tree turn", r)
                    mstop = j + 1 >= max_depth
                    need(bool(fl & EV_MAX_DEPTH) == mstop, "max_depth flag", r, fl)
                    if fturn:
                        out["seen"].add("tree_turn")
                    if mstop:
                        out["seen"].add("max_depth")
                    stop = fturn or mstop
                    need(bool(fl & EV_END) == stop, "end flag", r, fl)
                    break
                need(not fl & (EV_END | EV_SUB_DONE | EV_TREE | EV_TREE_TURN | EV_MAX_DEPTH), "flags of an inner leaf", r, fl)
                xb, vb, wb, Swb = np.asarray(Xr[r], dtype=np.float64), vl, wt, Swt
            if not stop:
                need(complete, "a sub-tree neither ended nor completed", t, j)
                j += 1
        # ---- row t
        xsel, lpsel, Hsel, wsel, Swsel = cand
        need(np.array_equal(rec["draws"][t], xsel), "row is not the tree's candidate", t)
        need(float(rec["logp"][t]) == lpsel, "recorded logp is not the candidate's", t)
        de_dev = 0.0 if Hsel is None else Hsel - float(ev[r]["H0"])
        need(float(rec["energy_error"][t]) == de_dev, "energy_error", t, float(rec["energy_error"][t]), de_dev)
        need(int(rec["divergent"][t]) == div_t, "divergent flag of the row", t)
        need(int(rec["tree_depth"][t]) == j + 1 and int(rec["n_leapfrog"][t]) == nleaf, "tree statistics", t,
             (int(rec["tree_depth"][t]), int(rec["n_leapfrog"][t])), (j + 1, nleaf))
        close("a", rec["accept_prob"][t], sacc / nleaf, (Bacc / nleaf + 4 * EPS) / EPS, 1.0, "accept_prob", t)
        x, lp, wg, Swg = xsel, lpsel, wsel, Swsel
    need(r == len(lpr) - 1, "rounds left over", r, len(lpr))
    return out


# ---- the grid of tests/test_gpu_nuts_steps.py (the fits, targets, seeds and step sizes of tests/test_gpu_hmc_steps.py) ---------------------
GRID_DEPTH, GRID_T, GRID_K = 5, 3, 3
GRID = ([(d, J, tn, GRID_DEPTH, GRID_T) for d in (5, 64, 257, 1000) for J in (2, 6, 16, 32) for tn in ("gauss", "funnel")]
        + [(d, J, tn, GRID_DEPTH, GRID_T) for d, J in H.GRID_MID for tn in ("gauss", "funnel")] + [(20000, 6, "gauss", 3, 1)])


def case_id(case):
    return "%s-d%d-J%d" % (case[2], case[0], case[1])
