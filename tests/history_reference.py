"""Teacher-forced check of the history walk: every step of every path against a long-double replay, a bound counted from the
kernel's operations, and a Python mirror of the dispatch.  Not collected by pytest; used by tests/test_gpu_history_steps.py and pinned
on the CPU by tests/test_history_reference_cpu.py.

  pf_history_kernel<EPT, NT>     register sets of rows, 1 / alpha carried in registers   (pathfinder.jl_amd/csrc/fit_kernels.hip)
  pf_history_lean_kernel<EPT>    1024 threads, 1 / alpha carried in LDS
  pf_history_mem_kernel          1024 threads, nothing carried: alpha re-read, the reference's divisions

All three walk a trace (theta_l, grad_l), l = 0 .. L (lbfgs_inverse_hessians, reference src/inverse_hessian.jl:25-66).  Step l forms
    s = fl(theta_l - theta_{l-1}),  y = fl(grad_{l-1} - grad_l)                      one rounding each: INPUTS of the step
    b = y's   q = y'y   a = y'diag(alpha)y   c = s'diag(1 / alpha)s                  alpha = alpha_{l-1}
    accepted  <=>  b > eps q                                                         (:47)
    alpha_l,i = b / x_i,  x_i = a / alpha_i + y_i^2 - (a / c)(s_i / alpha_i)^2        gilbert_init (:5-10), when accepted
    alpha_l   = fill(b / q)                                                          hinit = nocedal_wright, when accepted
    alpha_l   = alpha_{l-1}                                                          when rejected
and the ring of a point is the last min(#accepted, J) accepted steps, oldest first (:49-52, :105).

`Replay` restates one path in np.longdouble.  The decisions, the ring, j_eff and n_rejected depend on s and y only, so they are
replayed once, from the inputs.  alpha is TEACHER-FORCED: `Replay.step(l, alpha_prev)` takes the walk's own float64 alpha of point
l - 1 and returns what alpha_l must be, so errors do not accumulate and step 60 is held as tightly as step 1.

The bound (u = 2^-53; g(n) = n u / (1 - n u)).  Counted from the kernels, not measured.  A sum of the walk is formed as
    n_ser serial terms per thread (v += term; EPT in the register and lean kernels, ceil(d / 1024) in the memory-resident one),
    6 butterfly levels inside a wave (two permlane swaps, four row shifts: pf_block_sum_mv),
    NT / 64 - 1 additions across the waves, in wave order,
so its longest path has A = n_ser + 6 + NT / 64 - 1 additions (`chain`), and
    |fl(sum) - sum| <= g(A + r) sum |term|,     r = roundings inside one term:
    b: r = 1 (y s)      q: r = 1 (y y)      a: r = 2 ((y alpha) y)      c: r = 2 + rcp ((s ial) s resp. (s s) / alpha)
rcp = the roundings by which the kernel's 1 / alpha differs from the exact reciprocal of the stored alpha: the register and the lean
kernels CARRY ial = fl(x fl(1 / b)) while they store alpha = fl(b / x): ial = (1 / alpha)(1 + d1)(1 + d2)(1 + d3), rcp = 3 (this also
covers fl(1 / fl(b / q)) of nocedal_wright, the exact 1 of the first point and the carried state a resumed launch restores).  The
memory-resident kernel divides by the stored alpha: rcp = 0.  The oracle sums row after row (A = d) and multiplies by fl(1 / alpha): rcp = 1.
With E_b = g(A + 1) sum|y_i s_i| / |b|, E_q = g(A + 1), E_a = g(A + 2), E_c = g(A + 2 + rcp) (a, c, q are sums of non-negative terms):
    T1 = a / alpha_i         rel. error E_a + (1 + rcp) u          (one product or quotient, the reciprocal's roundings)
    T2 = y_i^2               u
    T3 = (a / c)(s_i / alpha_i)^2     E_a + E_c + u (the quotient a / c) + 2 (1 + rcp) u (s ial, twice) + 2 u (two products)
    x  = fl(fl(T1 + T2) - T3)         two more roundings, each at most u (|T1| + |T2| + |T3|): 2 u on every term
    dx_i = |T1| (E_a + (3 + rcp) u) + |T2| 3 u + |T3| (E_a + E_c + (7 + 2 rcp) u),      delta_i = dx_i / |x_i|  (the REFERENCE's x_i)
    |alpha_l,i - ref_i| <= |ref_i| (E_b + delta_i / (1 - delta_i) + u) (1 + 2^-20)       gilbert_init
    |alpha_l,i - ref_i| <= |ref_i| (E_b + E_q + u) (1 + 2^-20)                           nocedal_wright
(the last factor covers the products of two of the small terms, each below 2^-40 of the bound).  Fused multiply-adds only remove
roundings from this count.  There is no conditioning gate and no excluded coordinate: cancellation in x_i enters through the division
by |x_i| and nowhere else.  `x_cond` reports min_i |x_i| / (|T1| + |T2| + |T3|); the CPU test asserts it stays >= 0.5 on the grid, which
keeps delta_i within twice the counted constant.  (d = 1 is the exception BY IDENTITY: there a / alpha = (a / c)(s / alpha)^2 = y^2,
x = y^2 + y^2 - y^2 and the quotient is exactly 1 / 3; it is asserted as such.)

Decisions are not teacher-forced and get no borderline exemption.  The kernel compares fl(b) with fl(eps fl(q)):
    |(fl(b) - fl(eps fl(q))) - (b - eps q)| <= g(A + 2) (sum|y_i s_i| + eps q)
and `margin` = |b - eps q| / (sum|y_i s_i| + eps q) of every step must be at least 1000 g(A + 2) (`decision_bound`): the grid's eps
sits between two neighbouring order statistics of b / q, so no step is borderline.  A step whose y is not finite is rejected by every
implementation (a comparison with NaN is false) and has no margin.

`mirror_walk` is a free-running float64 NumPy walk in the summation order of the plan it is given (thread -> element map tid + NT e,
butterfly, wave order), carrying the reciprocal as the register kernels do or dividing as the memory-resident kernel and the oracle do.
Its `mut` argument applies one fault to the otherwise correct walk (`MUTATIONS`); `check_path` must reject each.
"""
import collections

import numpy as np

import fit_reference as fr
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON   # noqa: F401  (one long-double skip convention for the suite)

LD = np.longdouble
U = LD(2.0) ** -53
SLACK = 1 + LD(2.0) ** -20
MARGIN_FACTOR = 1000
X_COND_MIN = 0.5
J = 3
LENGTHS = (13, 1, 12, 2, 15, 14)                               # 1 point, 2 points, four consecutive lengths from 2 J + 6: L mod 3 and L mod 4 take every value


# ---- Python mirror of the dispatch (pf_launch_history) ---------------------------------------------------------------------------------
def plan_for(d, force=None):
    """the plan ONE history launch takes at dimension d; force = PFMI_HISTORY_KERNEL ("mem", "prefetch") or None"""
    f = force[0] if force else ""
    if d > 16 * 1024 or f == "m":
        return "hist:mem"
    if d <= 1024:
        ept, nt = (1, 64) if d <= 64 else (2, 64) if d <= 128 else (4, 64) if d <= 256 else (2, 256) if d <= 512 else (4, 256)
        return f"hist:reg:{ept},{nt}"
    ept = -(-d // 1024)
    if ept <= 2:
        return "hist:reg:2,1024"
    if ept <= 10:
        e = 4 if ept <= 4 else 6 if ept <= 6 else 8 if ept <= 8 else 10
        return f"hist:reg:{e},1024" if f == "p" else f"hist:lean:{e}"
    return "hist:reg:12,1024" if ept <= 12 else "hist:reg:16,1024"


REG_DEFAULT = ((1, 64), (2, 64), (4, 64), (2, 256), (4, 256), (2, 1024), (12, 1024), (16, 1024))
ALL_PLANS = ([f"hist:reg:{e},{nt}" for e, nt in REG_DEFAULT] + [f"hist:lean:{e}" for e in (4, 6, 8, 10)]
             + [f"hist:reg:{e},1024" for e in (4, 6, 8, 10)] + ["hist:mem"])
REACHABLE = list(ALL_PLANS)                                    # the four prefetch instances through PFMI_HISTORY_KERNEL=prefetch
RANGES = ((1, 64), (65, 128), (129, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 4096), (4097, 6144), (6145, 8192), (8193, 10240),
          (10241, 12288), (12289, 16384))


def geometry(plan, d):
    """(kind, serial terms per thread, threads) of a plan; "oracle": one serial sum over d"""
    if plan == "oracle":
        return "oracle", d, 1
    parts = plan.split(":")
    if parts[1] == "mem":
        return "mem", -(-d // 1024), 1024
    if parts[1] == "lean":
        return "lean", int(parts[2]), 1024
    ept, nt = (int(v) for v in parts[2].split(","))
    return "reg", ept, nt


def chain(plan, d):
    """A: additions on the longest path of one of the walk's sums"""
    kind, nser, nt = geometry(plan, d)
    return nser if kind == "oracle" else nser + 6 + nt // 64 - 1


def rcp_roundings(plan):
    kind = geometry(plan, 1)[0]
    return {"reg": 3, "lean": 3, "mem": 0, "oracle": 1}[kind]


def _g(n):
    return n * U / (1 - n * U)


def decision_bound(plan, d):
    """the counted relative error of b - eps q in units of sum|y s| + eps q"""
    return float(_g(chain(plan, d) + 2))


# ---- the replay ----------------------------------------------------------------------------------------------------------------------------
class Replay:
    """one path (theta, grad: (n, d) float64) in long double: decisions, ring, j_eff, n_rejected from the inputs; alpha teacher-forced"""

    def __init__(self, theta, grad, J, eps, hinit="gilbert"):
        theta, grad = np.asarray(theta, dtype=np.float64), np.asarray(grad, dtype=np.float64)
        self.theta, self.grad, self.J, self.eps, self.hinit = theta, grad, J, eps, hinit
        self.n, self.d = theta.shape
        L = self.n - 1
        self.s = (theta[1:] - theta[:-1]).astype(LD)           # float64 differences: one rounding each, as the kernels form them
        with np.errstate(invalid="ignore"):
            self.y = (grad[:-1] - grad[1:]).astype(LD)
            self.b = np.sum(self.y * self.s, axis=1)
            self.ab = np.sum(np.abs(self.y * self.s), axis=1)
            self.q = np.sum(self.y * self.y, axis=1)
            e = LD(eps)
            self.accept = np.array([bool(self.b[l] > e * self.q[l]) for l in range(L)], dtype=bool)
            self.finite = np.isfinite(self.b) & np.isfinite(self.q)
            self.margin = np.full(L, np.inf)
            ok = self.finite & (self.ab + e * self.q > 0)
            self.margin[ok] = (np.abs(self.b[ok] - e * self.q[ok]) / (self.ab[ok] + e * self.q[ok])).astype(np.float64)
        acc, self.ring, self.jeff = [], [[]], np.zeros(self.n, dtype=np.int32)
        for l in range(1, self.n):
            if self.accept[l - 1]:
                acc.append(l - 1)
            self.ring.append(acc[-J:] if J > 0 else [])
            self.jeff[l] = len(self.ring[l])
        self.n_rejected = int(L - len(acc))

    def ratios(self):
        """b / q of the finite steps (float64): what eps is chosen from"""
        return (self.b[self.finite] / self.q[self.finite]).astype(np.float64)

    def step(self, l, alpha_prev, plan):
        """(alpha_l in long double, its per-coordinate absolute bound, x_cond) of ACCEPTED step l from the walk's own alpha of point l - 1"""
        A, rcp = chain(plan, self.d), rcp_roundings(plan)
        s, y, b, q = self.s[l - 1], self.y[l - 1], self.b[l - 1], self.q[l - 1]
        E_b = _g(A + 1) * self.ab[l - 1] / np.abs(b)
        if self.hinit == "nocedal_wright":
            ref = np.full(self.d, b / q, dtype=LD)
            return ref, np.abs(ref) * (E_b + _g(A + 1) + U) * SLACK, 1.0
        al = np.asarray(alpha_prev, dtype=np.float64).astype(LD)
        ia = 1 / al
        a, c = np.sum(y * y * al), np.sum(s * s * ia)
        E_a, E_c = _g(A + 2), _g(A + 2 + rcp)
        T1, T2, T3 = a * ia, y * y, (a / c) * (s * ia) ** 2
        x = T1 + T2 - T3
        ref = b / x
        tot = np.abs(T1) + np.abs(T2) + np.abs(T3)
        dx = np.abs(T1) * (E_a + (3 + rcp) * U) + np.abs(T2) * 3 * U + np.abs(T3) * (E_a + E_c + (7 + 2 * rcp) * U)
        delta = dx / np.abs(x)
        rel = np.where(delta < 0.5, E_b + delta / (1 - np.minimum(delta, LD(0.5))) + U, LD(0))    # (delta >= 1 / 2: the first-order count does not hold; a zero bound fails the step)
        return ref, np.abs(ref) * rel * SLACK, float(np.min(np.abs(x) / tot))


def check_path(rep, plan, alpha, jeff, n_rej, sblock=None):
    """one path of a walk (alpha (n, d) float64, jeff (n,), n_rej, sblock(l) -> the (d, j_eff[l]) S block of point l's fit or None) against
    its Replay.  Returns (report, failures): report = {"ratio": largest error / bound over the accepted steps, "x_cond": smallest,
    "accepted", "rejected"}; failures is a list of (what, l, detail) and is empty for a correct walk."""
    n, d = rep.n, rep.d
    alpha = np.asarray(alpha, dtype=np.float64)
    fails, worst, xc = [], 0.0, np.inf
    if alpha.shape != (n, d):
        return {"ratio": np.inf, "x_cond": 0.0}, [("alpha_shape", -1, alpha.shape)]
    if not (np.all(alpha[0] == 1.0) and int(jeff[0]) == 0):
        fails.append(("first_point", 0, (float(alpha[0].min()), float(alpha[0].max()), int(jeff[0]))))
    if not np.array_equal(np.asarray(jeff, dtype=np.int64), rep.jeff.astype(np.int64)):
        fails.append(("j_eff", int(np.argmax(np.asarray(jeff) != rep.jeff)), (list(map(int, jeff)), list(map(int, rep.jeff)))))
    if int(n_rej) != rep.n_rejected:
        fails.append(("n_rejected", -1, (int(n_rej), rep.n_rejected)))
    for l in range(1, n):
        if not rep.accept[l - 1]:
            if alpha[l].tobytes() != alpha[l - 1].tobytes():
                fails.append(("rejected_step_moved_alpha", l, int(np.sum(alpha[l] != alpha[l - 1]))))
        else:
            ref, bound, cond = rep.step(l, alpha[l - 1], plan)
            xc = min(xc, cond)
            err = np.abs(alpha[l].astype(LD) - ref)
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.where(err == 0, LD(0), err / bound).astype(np.float64)
            r[~np.isfinite(alpha[l])] = np.inf
            r[np.isnan(r)] = np.inf
            i = int(np.argmax(r))
            worst = max(worst, float(r[i]))
            if not r[i] <= 1.0:
                fails.append(("alpha", l, (i, float(alpha[l, i]), float(ref[i]), float(r[i]))))
            if rep.hinit == "nocedal_wright" and not np.all(alpha[l] == alpha[l, 0]):
                fails.append(("nocedal_wright_not_constant", l, int(np.sum(alpha[l] != alpha[l, 0]))))
        if sblock is not None:
            S = sblock(l)
            want = fr.history_columns(rep.theta, rep.grad, rep.ring[l])[0]
            if S.shape != want.shape or np.asarray(S, dtype=np.float64).tobytes() != np.ascontiguousarray(want).tobytes():
                fails.append(("ring_sources", l, rep.ring[l]))
    rejected = int(np.sum(~rep.accept))
    return {"ratio": worst, "x_cond": float(xc), "accepted": int(np.sum(rep.accept)), "rejected": rejected}, fails


# ---- float64 mirrors of the walk in the kernels' summation orders ---------------------------------------------------------------------------
def _block_sum(x, plan, fill=0.0):
    """the sum of x (d,) as the plan forms it, in x's dtype: serial per thread over tid + NT e, butterfly, waves in order.  fill: the term
    of the slots past d (0: masked, as the kernels do)"""
    kind, nser, nt = geometry(plan, len(x))
    if kind == "oracle":
        return np.cumsum(x)[-1]
    pad = np.full(nser * nt, fill, dtype=x.dtype)
    pad[:len(x)] = x
    X = pad.reshape(nser, nt)
    acc = np.zeros(nt, dtype=x.dtype)
    for e in range(nser):
        acc = acc + X[e]
    w = acc.reshape(nt // 64, 4, 16)                            # rows of 16 lanes: (c, c + 32) and (c + 16, c + 48), then their sum
    p = (w[:, 0] + w[:, 2]) + (w[:, 1] + w[:, 3])
    while p.shape[1] > 1:                                       # row_shr 1, 2, 4, 8: the pairwise tree that ends in lane 15
        p = p[:, 1::2] + p[:, 0::2]
    tot = p[0, 0]
    for k in range(1, p.shape[0]):
        tot = tot + p[k, 0]
    return tot


# three ways to break pf_history_kernel itself, restated on the mirror: the remainder of the NS-times unrolled loop dropped (the last L mod NS
# steps never run), a step reading the register set one ahead (point l + 1, clamped at L, in place of point l) and the `in` mask skipped
# (the slots past d repeat coordinate d - 1, which is what the clamped loads deliver)
KERNEL_BREAKS = ("tail_dropped", "wrong_register_set", "padding_not_masked")
MUTATIONS = ("drop_last_coordinate", "alpha_two_points_back", "stale_reciprocal", "c_replaced_by_a", "rejected_step_applied",
             "last_step_not_applied", "ring_source_off_by_one")


def mirror_walk(theta, grad, J, eps, hinit, plan, mut=None):
    """(alpha_all, hist_len, hist_src, n_rejected) of one path as a float64 walk in `plan`'s summation order and reciprocal form;
    mut: one of MUTATIONS, a fault in the otherwise correct walk"""
    assert mut is None or mut in MUTATIONS + KERNEL_BREAKS, mut
    theta, grad = np.asarray(theta, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    n, d = theta.shape
    divide = geometry(plan, d)[0] in ("mem", "oracle")
    ns = 4 if geometry(plan, d)[1] <= 6 else 3                 # register sets of pf_history_kernel
    alpha_all = np.empty((n, d))
    hist_len, hist_src = np.zeros(n, dtype=np.int32), np.full((n, J), -1, dtype=np.int32)
    al, ial = np.ones(d), np.ones(d)
    al_old, ial_old = al, ial                                  # the state one accepted step earlier
    alpha_all[0] = 1.0
    acc, nacc_at, applied_reject = [], [0], False
    for l in range(1, n):
        with np.errstate(invalid="ignore"):
            l1 = min(l + 1, n - 1) if mut == "wrong_register_set" else l
            s, y = theta[l1] - theta[l - 1], grad[l - 1] - grad[l1]
            ta = y * al * y
            if mut == "drop_last_coordinate":
                ta = ta.copy()
                ta[d - 1] = 0.0
            tc = s * s / al if divide else s * ial * s
            terms = (y * s, y * y, ta, tc)
            v = [_block_sum(t, plan, t[d - 1] if mut == "padding_not_masked" else 0.0) for t in terms]
            accept = bool(v[0] > eps * v[1])
        if mut == "rejected_step_applied" and not accept and not applied_reject and np.isfinite(v[0]):
            accept = applied_reject = True
        if (mut == "last_step_not_applied" and l == n - 1) or (mut == "tail_dropped" and l > (n - 1) - (n - 1) % ns):
            accept = False
        if accept:
            if hinit == "nocedal_wright":
                an = v[0] / v[1]
                new_al, new_ial = np.full(d, an), np.full(d, 1.0 / an)
            else:
                a, b, c = v[2], v[0], v[3]
                if mut == "c_replaced_by_a":
                    c = a
                ual, uial = al, ial
                if mut == "alpha_two_points_back" and l >= 2:
                    ual = alpha_all[l - 2]
                    uial = 1.0 / ual
                if mut == "stale_reciprocal":
                    uial = ial_old
                aoc = a / c
                if divide:
                    sa = s / ual
                    x = a / ual + y * y - aoc * sa * sa
                    new_al, new_ial = b / x, None
                else:
                    sa = s * uial
                    x = a * uial + y * y - aoc * sa * sa
                    new_al, new_ial = b / x, x * (1.0 / b)
            al_old, ial_old = al, ial
            al = new_al
            ial = 1.0 / al if new_ial is None else new_ial
            acc.append(l - 1)
        alpha_all[l] = al
        nacc_at.append(len(acc))
    for l in range(1, n):
        na = nacc_at[l]
        re = min(na, J)
        hist_len[l] = re
        lo = na - re
        if mut == "ring_source_off_by_one" and na > J:
            lo -= 1
        hist_src[l, :re] = acc[lo:lo + re]
    return alpha_all, hist_len, hist_src, (n - 1) - len(acc)


def sblock_of(theta, grad, hist_len, hist_src):
    """the S block a fit of point l would hold, from a walk's own ring sources"""
    return lambda l: fr.history_columns(theta, grad, hist_src[l, :int(hist_len[l])])[0]


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------------
# eps: "third" = between two neighbouring order statistics of b / q at the one-third quantile of the case's steps; "all" / "none": every
# step accepted / rejected (d = 1: b / q is the same number at every step); "default": 1e-12
Case = collections.namedtuple("Case", "d force regime seed eps hinit bad", defaults=("third", "gilbert", None))
FAMILY_CASES = {"reg<=256": (300, None), "reg1024": (11000, None), "lean": (5000, None), "mem": (700, "mem")}


def _grid():
    out, names = [], tuple(fr.REGIMES)
    rot = 0

    def add(d, force=None, **kw):
        nonlocal rot
        out.append(Case(d, force, names[rot % len(names)], 700 + len(out), **kw))
        rot += 1

    for lo, hi in RANGES:
        for d in (lo, hi):
            if d == 1:
                add(1, eps="all")
                add(1, eps="none")
            else:
                add(d)
            if 2048 < d <= 10240:
                add(d, "prefetch")
    add(16385)
    add(1, "mem", eps="all")
    add(1, "mem", eps="none")
    add(1023, "mem")
    add(2049, "mem")
    for d, force in FAMILY_CASES.values():
        add(d, force, eps="default")
        add(d, force, hinit="nocedal_wright")
        add(d, force, bad=(5, d - 1, float("nan")))
    return out


GRID = _grid()


def case_id(c):
    return (f"d{c.d}-{c.regime}" + (f"-{c.force}" if c.force else "") + ("" if c.eps == "third" else f"-eps_{c.eps}")
            + ("-nw" if c.hinit != "gilbert" else "") + ("-nan" if c.bad else ""))


def case_plan(c):
    return plan_for(c.d, c.force)


def case_traces(c):
    cond, dep = fr.REGIMES[c.regime]
    return fr.quad_history(c.d, LENGTHS, cond, dep, c.seed, c.bad)


def case_eps(c, th, gr):
    """the case's eps from its own steps (long double ratios b / q, pooled over the paths)"""
    if c.eps == "default":
        return 1e-12
    r = np.sort(np.concatenate([Replay(t, g, J, 0.0).ratios() for t, g in zip(th, gr)]))
    assert len(r) and r[0] > 0, "quad_history: every step has s'y > 0"
    if c.eps == "all":
        return float(r[0]) / 2
    if c.eps == "none":
        return float(r[-1]) * 2
    k = len(r) // 3
    return float(np.sqrt(r[k - 1] * r[k]))


def case_replays(c, th, gr):
    eps = case_eps(c, th, gr)
    return eps, [Replay(t, g, J, eps, c.hinit) for t, g in zip(th, gr)]
