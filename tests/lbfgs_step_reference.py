"""Teacher-forced check of an L-BFGS trace: every recorded step against an extended-precision replay.  Plain NumPy, no GPU.

The optimisers of this repository (pfmi/optimize.py, the oracle's pfo_optimize_trace, lbfgs_kernels.hip, lbfgs_closure_kernel.hip) store
s = x_{l+1} - x_l and y = g_{l+1} - g_l formed from exactly the values they record (trace row l: x_l and grad logp = -g_l).  The ring
that produced step l can therefore be rebuilt bit for bit from the trace, and what the step from the recorded x_l MUST be is computed
for each l separately: errors do not accumulate, step 60 is held as tightly as step 1.

`check_trace` returns one record per step l -> l + 1 and a summary.  Per step:

  (a) direction, never exempt.  p = -H g by the two-loop recursion of pfmi/optimize.py in np.longdouble (gamma from the newest pair
      of the ring; p = -g and an empty ring when g'p >= 0).  With a_fit = (dx.p) / (p.p), dx = x_{l+1} - x_l:
          |dx_i - a_fit p_i| <= 2^-52 (|x_l,i| + |x_l+1,i|) + tau_l |a_fit| |p|_inf            elementwise.
      The first term covers the rounding of x + a p (one rounding with fma, two without: 2^-53 |a p_i| + 2^-53 |x_l+1,i| and
      |a p_i| <= |x_l,i| + |x_l+1,i|).  tau_l = 8 max(dev64_l, 2^-50), where dev64_l is the larger relative deviation (in |.|_inf) from
      the long-double p of fp64 evaluations of the SAME step made here: the two-loop recursion, the Byrd-Nocedal-Schnabel compact
      form the kernels use, and the two-loop recursion with every inner product summed left to right (NumPy sums pairwise; the scalar C
      oracle sums 20 000 terms in order and missed 8 x the spread of the first two by a factor 1.5 there, the only miss of the CPU grid).
      It measures the conditioning of this step and is never taken from the implementation under test; the factor 8 is the allowance
      for another summation order (block reductions, padded rows, lane-order sums).
      The bound is evaluated at the best step length within a_fit's own rounding error, rho = 2^-53 sum |x_l+1,j p_j| / sum p_j^2
      (`_direction_ratio`): at a_fit itself a CORRECT fp64 driver misses it by factors of 20 to 190 late in a trace, where |a p| << |x|
      and the least-squares a carries more error than a coordinate with |x_i| << |x|_inf is allowed.
  (b) step length.  The strong-Wolfe search of pfmi/optimize.py is replayed from (x_l, p, f_l, g_l) with `fg`, the target's fp64
      logp_and_grad, and a0 = 1 (ring not empty) or min(1, 1 / max(|g|_2, 1e-300)); it gives a_replay, a dyadic multiple of a0, and
          |a_fit - a_replay| <= |a_replay| (tau_l + 2^-52 |x|_inf / |a p|_inf).
      A step is BORDERLINE when a comparison the replayed search made had its two sides within 1e-9 (1 + |f0|) of each other: another
      correct implementation may then branch the other way.  A borderline step that misses the bound is EXEMPT from (b) if it still
      satisfies strong Wolfe (c1 = 1e-4, c2 = 0.9) from the recorded f_{l+1}, g_{l+1}, or if the replay hit its 25 + 30 evaluation
      cap.  (Near convergence |a g0| falls below 1e-9 and a third to a half of a trace's steps are borderline: the bound is therefore
      asserted on borderline steps as well, and only a step that NEEDS the exemption counts against the cap.)  Without `fg`, (b) is the Wolfe check from the recorded values plus "a_fit / a0 is a dyadic rational, denominator <= 2^30".
      (Slack of the Wolfe check: the implementation compared ITS f and ITS g'p; f is recorded, so the first condition gets the rounding
      of f0 + c1 a g0 and tau_l on g0; the second gets tau_l (|g0| + sum |g_l+1,i p_i|), p and the sum's order being its own.)
  (c) curvature.  The pair of step l enters the ring when y's > 1e-10 y'y and the `reject_every` hook does not drop it.  When y's is
      within 1e-6 relative of the threshold both continuations are tried at the next step, either is accepted, and that step counts
      as exempt.
  (d) stop rules.  No recorded point before the last has |g|_inf <= g_tol or a non-finite value; the last point is `converged`,
      `maxiters` (npts == maxiters + 1), `not moved` or `non-finite`; anything else is a failure (`none`).

Cap: exempt steps are at most 10 % of a trace's steps and none of the first J + 2 is exempt (`assert_trace`).

`variant` alters the REFERENCE -- the same as checking a wrong implementation against the right one -- for the mutation tests:
  gamma_oldest, gamma_one, ring_Jm1 (ring of J - 1), evict_newest (a full ring replaces its newest pair), flip_gYt (sign of the
  gamma Y t term of the compact form), a0_one (a0 = 1 with an empty ring), skip_slot_6 / _4 / _2 (the fused reductions walk the ring in
  batches of CH = 6, 4 or 2 slots: the last slot, J - 1, of a ragged last batch is left out once the ring is full, J % CH != 0).
"""
import numpy as np

LD = np.longdouble
HAVE_LONGDOUBLE = np.finfo(LD).nmant >= 63
SKIP_REASON = "np.longdouble carries fewer than 63 mantissa bits here: no extended-precision reference"
EPS = 2.0 ** -52
TAU_FLOOR = 2.0 ** -50
TAU_FACTOR = 8.0
C1, C2, AMAX = 1e-4, 0.9, 1e10
VARIANTS = ("gamma_oldest", "gamma_one", "ring_Jm1", "evict_newest", "flip_gYt", "a0_one", "skip_slot_6", "skip_slot_4", "skip_slot_2")


# ---- directions ------------------------------------------------------------------------------------------------------------------
def _serial_dot(a, b):
    """left-to-right sum, as a scalar loop forms it (np.cumsum adds in order; `@` sums pairwise or in SIMD lanes)"""
    return np.cumsum(a * b)[-1]


def two_loop(g, S, Y, gam, dt, dot=np.dot):
    """H g by the two-loop recursion of pfmi/optimize.py (pairs oldest first) in dtype dt; gam None: s'y / y'y of the newest pair"""
    q = np.array(g, dtype=dt)
    S = [np.asarray(s, dtype=dt) for s in S]
    Y = [np.asarray(y, dtype=dt) for y in Y]
    al = []
    for s, y in zip(reversed(S), reversed(Y)):
        a = dot(s, q) / dot(y, s)
        al.append(a)
        q = q - a * y
    if S:
        q = q * (dt(gam) if gam is not None else dot(S[-1], Y[-1]) / dot(Y[-1], Y[-1]))
    for (s, y), a in zip(zip(S, Y), reversed(al)):
        b = dot(y, q) / dot(y, s)
        q = q + (a - b) * s
    return q


def compact(g, S, Y, gam, dt, sign=1):
    """H g in the compact form of Byrd, Nocedal & Schnabel (1994) the kernels use: t = R^-1 S'g, a = R^-T ((D + gam Y'Y) t - gam Y'g),
    H g = gam g + S a - gam Y t, R = triu(S'Y), D = diag(R).  sign = -1: the mutation `flip_gYt`."""
    g = np.asarray(g, dtype=dt)
    Sm = np.array(S, dtype=dt)
    Ym = np.array(Y, dtype=dt)
    h = len(S)
    gam = dt(gam) if gam is not None else (Sm[-1] @ Ym[-1]) / (Ym[-1] @ Ym[-1])
    SY, YY, u, w = Sm @ Ym.T, Ym @ Ym.T, Sm @ g, Ym @ g
    t = np.zeros(h, dtype=dt)
    for j in range(h - 1, -1, -1):
        t[j] = (u[j] - SY[j, j + 1:] @ t[j + 1:]) / SY[j, j]
    z = np.diag(SY) * t + gam * (YY @ t - w)
    a = np.zeros(h, dtype=dt)
    for j in range(h):
        a[j] = (z[j] - SY[:j, j] @ a[:j]) / SY[j, j]
    return gam * g + Sm.T @ a - dt(sign) * gam * (Ym.T @ t)


# ---- the ring, as the kernels keep it ----------------------------------------------------------------------------------------------
class _Ring:
    """pairs oldest first; head = physical slot of the oldest pair (kernel: slot of age i is (head + i) mod J)"""
    def __init__(self, J, pairs=(), head=0, evictions=0):
        self.J, self.pairs, self.head, self.evictions = J, list(pairs), head, evictions

    def copy(self):
        return _Ring(self.J, self.pairs, self.head, self.evictions)

    def clear(self):
        self.pairs, self.head, self.evictions = [], 0, 0

    def push(self, s, y, variant):
        cap = self.J - 1 if variant == "ring_Jm1" else self.J
        if cap <= 0:
            return
        if len(self.pairs) >= cap:
            if variant == "evict_newest":
                self.pairs[-1] = (s, y)
            else:
                self.pairs.pop(0)
                self.pairs.append((s, y))
            self.head = (self.head + 1) % cap
            self.evictions += 1
        else:
            self.pairs.append((s, y))

    def used(self, variant):
        """(S, Y, gam) the direction is built from; gam None = from the newest pair"""
        S, Y = [p[0] for p in self.pairs], [p[1] for p in self.pairs]
        gam = None
        if not S:
            return S, Y, gam
        if variant == "gamma_one":
            gam = 1.0
        elif variant == "gamma_oldest":
            gam = float((LD(1) * S[0].astype(LD)) @ Y[0].astype(LD) / (Y[0].astype(LD) @ Y[0].astype(LD)))
        elif variant and variant.startswith("skip_slot_"):
            ch = int(variant.rsplit("_", 1)[1])
            if len(S) == self.J and self.J % ch != 0:
                s, y = S[-1].astype(LD), Y[-1].astype(LD)
                gam = float((s @ y) / (y @ y))                       # (the kernels keep gam apart from the ring)
                age = (self.J - 1 - self.head) % self.J
                S, Y = S[:age] + S[age + 1:], Y[:age] + Y[age + 1:]
        return S, Y, gam


# ---- the line search of pfmi/optimize.py, replayed with every comparison watched -----------------------------------------------------
def replay_search(fg, x, f0, g, p, a0):
    """-> (a of the last evaluation, borderline, hit_cap).  fg(x) -> (f, grad f)."""
    g0 = float(g @ p)
    tol = 1e-9 * (1.0 + abs(f0))
    st = {"border": False}

    def near(lhs, rhs):
        if not (abs(lhs - rhs) > tol):
            st["border"] = True

    def phi(a):
        f, gv = fg(x + a * p)
        return float(f), float(gv @ p)

    a_prev, f_prev, a = 0.0, f0, a0
    lo = hi = f_lo = 0.0
    zoom = False
    for it in range(25):
        f, gd = phi(a)
        a_eval = a
        if not np.isfinite(f):
            a = 0.5 * (a_prev + a)
            continue
        near(f, f0 + C1 * a * g0)
        armijo_fails = f > f0 + C1 * a * g0
        if not armijo_fails and it > 0:
            near(f, f_prev)
        if armijo_fails or (it > 0 and f >= f_prev):
            zoom, lo, hi, f_lo = True, a_prev, a, f_prev
            break
        near(abs(gd), -C2 * g0)
        if abs(gd) <= -C2 * g0:
            return a, st["border"], False
        near(gd, 0.0)
        if gd >= 0:
            zoom, lo, hi, f_lo = True, a, a_prev, f
            break
        a_prev, f_prev = a, f
        a = min(2 * a, AMAX)
    if not zoom:
        return a_eval, st["border"], True
    for _ in range(30):
        a = 0.5 * (lo + hi)
        f, gd = phi(a)
        near(f, f0 + C1 * a * g0)
        hi_moves = f > f0 + C1 * a * g0
        if not hi_moves:
            near(f, f_lo)
        if hi_moves or f >= f_lo:
            hi = a
        else:
            near(abs(gd), -C2 * g0)
            if abs(gd) <= -C2 * g0:
                return a, st["border"], False
            near(gd * (hi - lo), 0.0)
            if gd * (hi - lo) >= 0:
                hi = lo
            lo, f_lo = a, f
    return a, st["border"], True


def _is_dyadic(q, tau):
    """q = m / 2^k with k <= 30, to relative tau"""
    if not np.isfinite(q) or q <= 0:
        return False
    m = q * 2.0 ** 30
    return abs(m - round(m)) <= max(tau * m, 0.0) and round(m) >= 1


def _direction_ratio(dx, p, a_fit, allow, x1):
    """max_i |dx_i - a p_i| / allow_i at the step length a that suits it best among those the trace cannot tell from a_fit: the
    least-squares a_fit = (dx.p) / (p.p) inherits from the rounding of x_{l+1} (|e_i| <= 2^-53 |x_l+1,i|) an error of at most
    rho = 2^-53 sum |x_l+1,j p_j| / sum p_j^2, which at a coordinate with |x_i| << |x|_inf is far above that coordinate's own
    allowance (measured on the host driver: x_l + p == x_l+1 bit for bit, residual 20 to 190 allowances at a_fit).  So the bound is
    taken at the best a in [a_fit - rho, a_fit + rho] (a convex problem in one unknown: ternary search); a_fit itself is among them."""
    pp = float(p @ p)
    if not pp > 0:
        r = np.abs(dx).astype(np.float64)
        return (float(np.max(np.where(r > 0, r / np.where(allow > 0, allow, 1e-300), 0.0))) if len(r) else 0.0), a_fit, r
    r0 = (dx - LD(a_fit) * p).astype(np.float64)
    p64 = p.astype(np.float64)
    w = np.where(allow > 0, allow, 1e-300)
    rho = 2.0 ** -53 * float(np.abs(x1) @ np.abs(p64)) / pp

    def worst(dl):
        return float(np.max(np.abs(r0 - dl * p64) / w))

    lo, hi = -rho, rho
    for _ in range(60):
        m1, m2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        if worst(m1) <= worst(m2):
            hi = m2
        else:
            lo = m1
    dl = 0.5 * (lo + hi)
    best = min((worst(0.0), 0.0), (worst(dl), dl))
    return best[0], a_fit + best[1], r0 - best[1] * p64


# ---- one step from one ring ----------------------------------------------------------------------------------------------------------
def _step(l, th, lp, gr, ring, fg, variant):
    ring = ring.copy()
    x, x1 = th[l], th[l + 1]
    g, f = -gr[l], -float(lp[l])
    gL = g.astype(LD)
    h_in, head_in, ev_in = len(ring.pairs), ring.head, ring.evictions
    S, Y, gam = ring.used(variant)
    restart = False
    dev = 0.0
    if S:
        if variant == "flip_gYt":
            p = -compact(g, S, Y, gam, LD, sign=-1)
        else:
            p = -two_loop(g, S, Y, gam, LD)
        if not (gL @ p < 0):
            restart = True
            ring.clear()
            p = -gL
        else:
            pn = float(np.max(np.abs(p)))
            if variant == "flip_gYt":                         # (dev64 is the spread of the SAME formula's fp64 evaluations)
                forms = (-compact(g, S, Y, gam, np.float64, sign=-1),)
            else:
                forms = (-two_loop(g, S, Y, gam, np.float64), -compact(g, S, Y, gam, np.float64),
                         -two_loop(g, S, Y, gam, np.float64, dot=_serial_dot))
            dev = max(float(np.max(np.abs(q_ - p))) for q_ in forms) / pn
    else:
        p = -gL
    tau = TAU_FACTOR * max(dev, TAU_FLOOR)
    dx = x1.astype(LD) - x.astype(LD)
    pp = p @ p
    a_fit = float((dx @ p) / pp) if pp > 0 else 0.0
    pinf = float(np.max(np.abs(p)))
    allow = EPS * (np.abs(x) + np.abs(x1)) + tau * abs(a_fit) * pinf
    ratio_a, a_dir, res = _direction_ratio(dx, p, a_fit, allow, x1)
    # (informational) the factor in front of max(dev64, 2^-50) this step needed once the rounding term is used up: 8 is what (a) grants
    rnd = EPS * (np.abs(x) + np.abs(x1))
    unit = abs(a_fit) * pinf * max(dev, TAU_FLOOR)
    ratio_rnd = float(np.max(np.maximum(np.abs(res) - rnd, 0.0))) / unit if unit > 0 and len(res) else 0.0
    if not np.all(np.isfinite(x1)):
        ratio_a = float("inf")

    # (b) step length
    a0 = 1.0 if (ring.pairs or variant == "a0_one") else min(1.0, 1.0 / max(float(np.sqrt(g @ g)), 1e-300))
    p64 = p.astype(np.float64)
    g0 = float(gL @ p)
    f1, g1 = -float(lp[l + 1]), -gr[l + 1]
    ap_inf = abs(a_fit) * pinf
    with np.errstate(invalid="ignore", over="ignore"):
        sum_gp = float(np.abs(g1) @ np.abs(p64))
        wolfe = bool(np.isfinite(f1) and f1 <= f + C1 * a_fit * g0 + EPS * (abs(f) + abs(f1)) + tau * C1 * abs(a_fit * g0)
                     and abs(float(g1 @ p64)) <= -C2 * g0 + tau * (abs(g0) + sum_gp))
    rec_b = {"a_replay": None, "ratio_b": 0.0, "borderline": False, "cap": False}
    ok_b, exempt_b = True, False
    nonfinite_next = not (np.isfinite(f1) and np.all(np.isfinite(g1)))
    if nonfinite_next:
        pass                                                  # the offending point is recorded and the run stops: (d) judges it
    elif fg is not None:
        a_rep, border, cap = replay_search(fg, x, f, g, p64, a0)
        tol_b = abs(a_rep) * (tau + (EPS * float(np.max(np.abs(x))) / ap_inf if ap_inf > 0 else 0.0))
        rb = abs(a_fit - a_rep) / tol_b if tol_b > 0 else (0.0 if a_fit == a_rep else float("inf"))
        rec_b = {"a_replay": a_rep, "ratio_b": rb, "borderline": border, "cap": cap}
        if rb > 1.0:
            if border and (wolfe or cap):
                exempt_b = True
            else:
                ok_b = False
    else:
        ok_b = wolfe and _is_dyadic(a_fit / a0, tau + (EPS * float(np.max(np.abs(x))) / ap_inf if ap_inf > 0 else 0.0))
        rec_b["ratio_b"] = 0.0 if ok_b else float("inf")
    rec = {"l": l, "h": h_in, "head": head_in, "evictions": ev_in, "restart": restart, "dev64": dev, "tau": tau, "a_fit": a_fit, "a0": a0,
           "ratio_a": ratio_a, "tau_factor": ratio_rnd, "a_dir": a_dir, "wolfe": wolfe, "ok_a": ratio_a <= 1.0, "ok_b": ok_b, "exempt_b": exempt_b, "exempt_c": False, **rec_b}
    return rec, ring


def check_trace(points, logps, grads, J, maxiters, g_tol, fg=None, reject_every=0, variant=None):
    """points (n, d), logps (n,), grads (n, d) = grad logp, as Engine.get_trace / OptimizationTrace / po.optimize_trace give them.
    fg: the target's logp_and_grad (x -> (logp, grad logp)) or None.  Returns (records, summary)."""
    th = np.ascontiguousarray(points, dtype=np.float64)
    gr = np.ascontiguousarray(grads, dtype=np.float64)
    lp = np.ascontiguousarray(logps, dtype=np.float64)
    n = len(th)
    assert variant is None or variant in VARIANTS, variant
    nfg = None
    if fg is not None:
        def nfg(x):
            v, gv = fg(x)
            return -v, -np.asarray(gv)
    rings = [_Ring(J)]
    recs = []
    rejected = 0
    for l in range(n - 1):
        cands = [_step(l, th, lp, gr, r, nfg, variant) for r in rings]
        rec, ring = min(cands, key=lambda c: (not (c[0]["ok_a"] and c[0]["ok_b"]), c[0]["ratio_a"]))
        if len(cands) > 1:
            rec["exempt_c"] = True
        recs.append(rec)
        # the pair of this step: s and y in fp64, exactly what the optimisers store
        s = th[l + 1] - th[l]
        y = -(gr[l + 1] - gr[l])
        rings = [ring]
        if np.all(np.isfinite(s)) and np.all(np.isfinite(y)):
            sL, yL = s.astype(LD), y.astype(LD)
            sy, yy = float(sL @ yL), float(yL @ yL)
            hook = bool(reject_every and (l + 1) % reject_every == 0)
            take = sy > 1e-10 * yy and not hook
            rec["sy"], rec["yy"], rec["take"] = sy, yy, take
            if not hook and abs(sy - 1e-10 * yy) <= 1e-6 * 1e-10 * yy and yy > 0:
                with_pair = ring.copy()
                with_pair.push(s, y, variant)
                rings = [with_pair, ring] if take else [ring, with_pair]
            elif take:
                ring.push(s, y, variant)
            if not take:
                rejected += 1

    # (d) stop rules
    gmax = np.max(np.abs(gr), axis=1)
    fin = np.isfinite(lp) & np.all(np.isfinite(gr), axis=1) & np.all(np.isfinite(th), axis=1)
    with np.errstate(invalid="ignore"):
        early = [int(l) for l in range(n - 1) if not fin[l] or gmax[l] <= g_tol]
    if not fin[-1]:
        stop = "non-finite"
    elif gmax[-1] <= g_tol:
        stop = "converged"
    elif n == maxiters + 1:
        stop = "maxiters"
    elif n >= 2 and np.array_equal(th[-1], th[-2]):
        stop = "not moved"
    else:
        stop = "none"
    fails = [(r["l"], "a", r["ratio_a"]) for r in recs if not r["ok_a"]] + [(r["l"], "b", r["ratio_b"]) for r in recs if not r["ok_b"]]
    fails.sort()
    exempt = [r["l"] for r in recs if r["exempt_b"] or r["exempt_c"]]
    full = [r["l"] for r in recs if r["h"] >= (J - 1 if variant == "ring_Jm1" else J)]
    wrapped = [r["l"] for r in recs if r["head"] != 0]
    checked_b = [r["ratio_b"] for r in recs if r["ok_b"] and not r["exempt_b"] and np.isfinite(r["ratio_b"])]
    summary = {
        "steps": len(recs), "max_h": max([r["h"] for r in recs], default=0), "wrapped": len(wrapped), "rejected": rejected,
        "restarts": sum(r["restart"] for r in recs), "exempt": len(exempt), "exempt_steps": exempt,
        "borderline": sum(bool(r["borderline"]) for r in recs), "evicted": sum(r["evictions"] > 0 for r in recs),
        "first_full": full[0] if full else None, "first_wrapped": wrapped[0] if wrapped else None,
        "turns": _turns(recs, J),
        "max_ratio_a": max([r["ratio_a"] for r in recs], default=0.0),
        "max_tau_factor": max([r["tau_factor"] for r in recs], default=0.0), "max_ratio_b": max(checked_b, default=0.0),
        "max_dev64": max([r["dev64"] for r in recs], default=0.0),
        "stop": stop, "early_stop_points": early, "failures": fails, "first_failure": fails[0] if fails else None,
    }
    return recs, summary


def _turns(recs, J):
    """full turns of the ring: evictions since the last restart, over J (head is back at its start after J of them)"""
    return max([r["evictions"] for r in recs], default=0) // J if J > 0 else 0


def assert_trace(case, recs, summary, J, impl="gpu"):
    """the assertions every test makes on a checked trace: (a) and (b) through margins.check under the config `lbfgs step <case>`, the
    stop rules, the exemption cap"""
    import margins as mg
    cfg = f"lbfgs step {case}"
    assert summary["stop"] != "none" and not summary["early_stop_points"], (case, summary["stop"], summary["early_stop_points"])
    bad = [r for r in recs if not r["ok_a"]]
    mg.check(cfg, f"direction residual / allowance @{impl}", [r["ratio_a"] for r in recs] or [0.0], 1.0,
             ctx=[(r["l"], r["h"], r["head"], r["ratio_a"]) for r in bad[:3]])
    mg.record(cfg, f"factor on max(dev64, 2^-50) needed beyond rounding @{impl}", [r["tau_factor"] for r in recs if np.isfinite(r["tau_factor"])] or [0.0],
              TAU_FACTOR, why="informational: what (a) asserts with the factor 8, as the factor each step needed")
    badb = [r for r in recs if not r["ok_b"]]
    mg.check(cfg, f"step length |a_fit - a_replay| / allowance @{impl}",
             [r["ratio_b"] for r in recs if not r["exempt_b"]] or [0.0], 1.0,
             ctx=[(r["l"], r["h"], r["head"], r["a_fit"], r["a_replay"], r["borderline"], r["wolfe"]) for r in badb[:3]])
    assert not summary["failures"], (case, summary["failures"][:5])
    assert summary["exempt"] <= 0.10 * summary["steps"], (case, "exempt steps above 10 %", summary["exempt_steps"], summary["steps"])
    assert all(l >= J + 2 for l in summary["exempt_steps"]), (case, "an exempt step among the first J + 2", summary["exempt_steps"])


# ---- the case grid shared by the CPU calibration (test_lbfgs_step_cpu.py) and the GPU test (test_gpu_lbfgs_steps.py) -------------------
# (id, target, d, J, maxiters, reject_every, x0 scale).  target: diag | lr8 | lr11 | lr16 | funnel (pfmi.t_diag(d, 1), t_lowrank(d, r, r - 6),
# t_funnel(d)).  K = 2 paths from HostRNG(17).
GRID = [
    # one wave (EPT 4, NT 64), ring in LDS
    ("w64-diag-J1", "diag", 40, 1, 120, 0, 2.0), ("w64-lr8-J6", "lr8", 40, 6, 120, 0, 2.0), ("w64-lr11-J16", "lr11", 40, 16, 120, 0, 2.0),
    ("w64-lr16-J6", "lr16", 40, 6, 120, 0, 2.0), ("w64-diag-J16", "diag", 40, 16, 120, 0, 2.0), ("w64-funnel-J6", "funnel", 40, 6, 120, 0, 10.0),
    ("w64-lr8-J6-rej", "lr8", 40, 6, 120, 3, 2.0),
    # 256 threads (4, 256), ring in LDS
    ("w256-diag-J6", "diag", 700, 6, 60, 0, 2.0), ("w256-lr8-J6", "lr8", 700, 6, 60, 0, 2.0), ("w256-lr16-J6", "lr16", 700, 6, 60, 0, 2.0),
    ("w256-funnel-J6", "funnel", 700, 6, 60, 0, 10.0), ("w256-diag-J6-rej", "diag", 700, 6, 60, 3, 2.0),
    # 256 threads, ring in global memory (ragged last batch of 6)
    ("w256g-diag-J10", "diag", 700, 10, 60, 0, 2.0), ("w256g-lr8-J16", "lr8", 700, 16, 60, 0, 2.0), ("w256g-lr11-J10", "lr11", 700, 10, 60, 0, 2.0),
    ("w256g-lr16-J16", "lr16", 700, 16, 60, 0, 2.0), ("w256g-lr8-J10-rej", "lr8", 700, 10, 60, 3, 2.0),
    # 20 x 512
    ("w512-diag-J2", "diag", 1500, 2, 40, 0, 2.0), ("w512-lr8-J6", "lr8", 1500, 6, 40, 0, 2.0), ("w512-lr16-J16", "lr16", 1500, 16, 40, 0, 2.0),
    ("w512-lr11-J6", "lr11", 1500, 6, 40, 0, 2.0), ("w512-diag-J6-rej", "diag", 1500, 6, 40, 3, 2.0),
    # 32 x 512
    ("w512x-diag-J6", "diag", 10300, 6, 20, 0, 2.0), ("w512x-lr8-J6", "lr8", 10300, 6, 20, 0, 2.0), ("w512x-lr16-J6", "lr16", 10300, 6, 20, 0, 2.0),
    ("w512x-diag-J6-rej", "diag", 10300, 6, 24, 3, 2.0),
]
# the closure kernel (LC_NT = 256 threads, batches of 4 slots, J up to 32)
CLOSURE_GRID = [
    ("clo-lr8-J6", "lr8", 50, 6, 120, 0, 2.0), ("clo-lr8-J24", "lr8", 50, 24, 120, 0, 2.0), ("clo-lr8-J32", "lr8", 50, 32, 120, 0, 2.0),
    ("clo-diag-J6", "diag", 20000, 6, 20, 0, 2.0), ("clo-lr8-J6-rej", "lr8", 50, 6, 120, 3, 2.0),
]
GRID_K, GRID_SEED, G_TOL = 2, 17, 1e-8


def grid_target(pfmi, name, d):
    if name == "diag":
        return pfmi.t_diag(d, 1)
    if name == "funnel":
        return pfmi.t_funnel(d)
    r = int(name[2:])
    return pfmi.t_lowrank(d, r, r - 6)


def grid_x0(pfmi, d, scale):
    return pfmi.HostRNG(GRID_SEED).rand(GRID_K * d).reshape(GRID_K, d) * 2 * scale - scale


def coverage_ok(summary, J):
    """the coverage condition of a grid case: at least 4 steps with a wrapped ring (head != 0); J <= 6: at least one full turn.  A ring
    of one pair has head == 0 always: there the steps behind an eviction count (every one of them reuses the slot)."""
    wrapped = summary["wrapped"] if J > 1 else summary["evicted"]
    return wrapped >= 4 and (J > 6 or summary["turns"] >= 1)
