"""Reference of the Woodbury operator surface (pathfinder.jl_amd/csrc/woodbury_kernels.hip: pfmi_woodbury_apply with its eight ops and
pfmi_woodbury_diag).  Not collected by pytest; used by tests/test_gpu_woodbury.py (and, for C_lane, tests/test_gpu_hmc_steps.py) and
pinned on the CPU by tests/test_woodbury_reference_cpu.py.

The factor is hmc_reference.Metric -- L and R are stated there and nowhere else:
    L v = s . Q [V'v_1; v_2]            (unwhiten, mode 0)        R g = [V y_1; y_2], y = Q'(s . g)       (rmul, mode 2)
    Q = I - Vh T Vh', k = min(d, 2 j) reflectors.  `Ops` adds what the other modes and the two-pass ops compute from the same arrays:
    Linv x = [V'^-1 u_1; u_2], u = Q'(x / s)   (whiten, mode 1: a FORWARD substitution with V')
    Rinv x = Q [V^-1 x_1; x_2] / s              (invunwhiten, mode 3: a BACK substitution with V)
    mul = L R, solve = Rinv Linv, quad = |R x|^2, invquad = |Linv x|^2 per column,
    diag_i = alpha_i + sum_ac B_ia D_ac B_ic with B = [alpha . Y, S] rebuilt from the trace (the kernel recomputes b from theta and grad)
    and D the fit's own.
Linv and Rinv use Q' and Q as the kernel does: they are the inverses of L and R only as far as Q is orthogonal.

`mirror` / `mirror_diag` restate the lane kernels in float64: one column, the rows walked in order, T zero-padded and V identity-padded
to KPAD, the head block i < KPAD with its i < d guards, then the tail loop.  `fault=` injects one wrong step (FAULTS).

Bounds.  eps = 2^-52 (two unit roundoffs per counted step); every scale is the same sum with each term in absolute value, formed in
long double; every constant is counted from the kernel's loops, none is fitted to GPU output; every check is recorded with bound 1.
  C_lane = d + 3 KPAD + 16     one lane sums all d rows of w = Vh'z (one fma per row); three contractions of at most KPAD terms (the head
                               transform with V, tv = T w or T'w, and Vh[i, :] tv); 16: the roundings of the inputs (s . x, x / s), the
                               final multiply-adds and slack for the order of the last adds
  C_solve = C_lane + KPAD      the substitution with V or V': at most KPAD terms per row
  unwhiten, rmul     |out - ref| <= C_lane eps S,  S = L_abs(|x|) or R_abs(|x|)
  whiten             |L(y) - x| <= C_solve eps L_abs(|y|) + |s . (Q Q' - I)(x / s)|                       y the kernel's output, no
  invunwhiten        |R(y) - x| <= C_solve eps R_abs(|y|) + |[V e_1; e_2]|, e = (Q'Q - I)[V^-1 x_1; x_2]  conditioning gate
                     The second term is what the factor's own non-orthogonality contributes: Q Q' - I = Vh (T Vh'Vh T' - T - T') Vh'
                     (Q'Q - I likewise with T' Vh'Vh T), formed in long double from that fit's reflectors and T and applied to the vector
                     (tests/fit_reference.py bounds |Q_k'Q_k - I| itself).
  whiten_fwd,        |y - ref| <= C_solve eps S_inv, the scaled forward bound: the error of u = Q'(x / s) passes through |V'^-1|, and the
  invunwhiten_fwd    substitution is backward stable, (V' + dV') y_1 = u_1 with |dV| <= KPAD eps |V|, so
                         S_Linv(x) = [|V'^-1| (Qt_abs(|x| / s)_1 + |V'| |ref_1|); Qt_abs(|x| / s)_2]
                         S_Rinv(x) = Q_abs([|V^-1| |V| |w_1|; |w_2|]) / s,  w = [V^-1 x_1; x_2]
                     with Q_abs(z) = z + |Vh| |T| |Vh|'z and Qt_abs with |T|'.  The scale carries |V^-1| |V|, as S_D does in fit_reference.
  mul                two passes: |out - L R x| <= 2 C_lane eps L_abs(R_abs(|x|)): the second pass's own error on an input bounded by the
                     first pass's majorant, and the first pass's error C_lane eps R_abs(|x|) pushed through L_abs
  solve              |out - Rinv Linv x| <= C_solve eps (S_Rinv(Linv x) + Rinv_abs(S_Linv(x))),  Rinv_abs(e) = Q_abs([|V^-1| e_1; e_2]) / s
  quad               |out - sum r_i^2| <= 2 sum_i |r_i| (C_lane eps R_abs(|x|)_i) + (d + 4) eps sum r_i^2,  r = R x: the column sum of
                     squares is one lane summing d terms
  invquad            the same with r = Linv x, C_solve and S_Linv(x): a forward quantity, hence the scaled forward form
  diag               |out_i - ref_i| <= (2 KPAD + 8) eps (alpha_i + |b_i|'|D| |b_i|): two contractions of KPAD terms; 8: the roundings
                     of b (alpha . (g - g'), theta' - theta) and the last add
"""
import numpy as np

import fit_reference as fr
import hmc_reference as H

LD = H.LD
EPS = H.EPS
KPADS = H.KPADS
OPS = ("unwhiten", "whiten", "rmul", "invunwhiten", "mul", "solve", "quad", "invquad")
# the modes of pf_woodbury_kernel an op launches, in order (pfmi_woodbury_apply)
LAUNCHES = {"unwhiten": (0,), "whiten": (1,), "rmul": (2,), "invunwhiten": (3,), "mul": (2, 0), "solve": (1, 3), "quad": (2,), "invquad": (1,)}
# the quantities recorded per op: the primitives' solves are checked in both forms
CHECKS = ("unwhiten", "rmul", "whiten", "whiten_fwd", "invunwhiten", "invunwhiten_fwd", "mul", "solve", "quad", "invquad", "diag")
FAULTS = ("T_for_Tt", "V_for_Vt", "fwd_for_back", "no_sqrt_alpha", "sqrt_alpha_wrong_side", "head_guard_dropped", "tail_from_kpad_plus_1",
          "diag_offdiag_dropped")


def c_lane(d, kpad):
    return d + 3 * kpad + 16


def c_solve(d, kpad):
    return c_lane(d, kpad) + kpad


def c_diag(kpad):
    return 2 * kpad + 8


def plan_names():
    """the 28 + 7 launch counters of the surface (pfmi_kernel_time)"""
    return ["woodbury:%d:%d" % (kp, m) for kp in KPADS for m in range(4)] + ["woodbury_diag:%d" % kp for kp in KPADS]


# ---- the operators in long double ------------------------------------------------------------------------------------------------------
class Ops:
    """everything the surface computes from one fit's factor M (an hmc_reference.Metric), in long double; X is (d, N)"""

    def __init__(self, M):
        self.M = M = M.astype(LD)
        self.d, self.k = M.d, M.k
        k = self.k
        self.Vi = fr._triu_inv(M.V) if k else np.zeros((0, 0), dtype=LD)
        G = M.Vh.T @ M.Vh
        self.G_qqt = M.T @ G @ M.T.T - M.T - M.T.T             # Q Q' - I = Vh G_qqt Vh'
        self.G_qtq = M.T.T @ G @ M.T - M.T - M.T.T             # Q'Q - I = Vh G_qtq Vh'

    # column-wise forms of Metric.L / Metric.R (one statement of L and R: hmc_reference.Metric)
    def _cols(self, f, X):
        X = np.asarray(X, dtype=LD)
        return np.stack([f(X[:, n]) for n in range(X.shape[1])], axis=1) if X.shape[1] else X.copy()

    def L(self, X):
        return self._cols(self.M.L, X)

    def R(self, X):
        return self._cols(self.M.R, X)

    def L_abs(self, Xa):
        return self._cols(self.M.L_abs, Xa)

    def R_abs(self, Xa):
        return self._cols(self.M.R_abs, Xa)

    def _q_abs(self, Z, transposed):
        M = self.M
        Ta = np.abs(M.T).T if transposed else np.abs(M.T)
        return Z + np.abs(M.Vh) @ (Ta @ (np.abs(M.Vh).T @ Z))

    def Linv(self, X):
        M, k = self.M, self.k
        Z = np.asarray(X, dtype=LD) / M.s[:, None]
        U = Z - M.Vh @ (M.T.T @ (M.Vh.T @ Z))
        U[:k] = self.Vi.T @ U[:k]
        return U

    def Rinv(self, X):
        M, k = self.M, self.k
        W = np.array(X, dtype=LD)
        W[:k] = self.Vi @ W[:k]
        return (W - M.Vh @ (M.T @ (M.Vh.T @ W))) / M.s[:, None]

    def S_Linv(self, X, ref=None):
        M, k = self.M, self.k
        ref = self.Linv(X) if ref is None else ref
        S = self._q_abs(np.abs(np.asarray(X, dtype=LD)) / M.s[:, None], True)
        S[:k] = np.abs(self.Vi).T @ (S[:k] + np.abs(M.V).T @ np.abs(ref[:k]))
        return S

    def Rinv_abs(self, E):
        E = np.array(E, dtype=LD)
        E[:self.k] = np.abs(self.Vi) @ E[:self.k]
        return self._q_abs(E, False) / self.M.s[:, None]

    def S_Rinv(self, X):
        M, k = self.M, self.k
        W = np.array(X, dtype=LD)
        W[:k] = self.Vi @ W[:k]
        Wa = np.abs(W)
        Wa[:k] = np.abs(M.V) @ Wa[:k]
        return self.Rinv_abs(Wa)

    def nonorth_L(self, X):
        """|s . (Q Q' - I)(x / s)|: what L(Linv x) - x is in exact arithmetic"""
        M = self.M
        Z = np.asarray(X, dtype=LD) / M.s[:, None]
        return np.abs(M.s[:, None] * (M.Vh @ (self.G_qqt @ (M.Vh.T @ Z))))

    def nonorth_R(self, X):
        """|[V e_1; e_2]|, e = (Q'Q - I)[V^-1 x_1; x_2]: what R(Rinv x) - x is in exact arithmetic"""
        M, k = self.M, self.k
        W = np.array(X, dtype=LD)
        W[:k] = self.Vi @ W[:k]
        E = M.Vh @ (self.G_qtq @ (M.Vh.T @ W))
        E[:k] = M.V @ E[:k]
        return np.abs(E)

    def apply(self, op, X):
        X = np.asarray(X, dtype=LD)
        if op == "unwhiten":
            return self.L(X)
        if op == "rmul":
            return self.R(X)
        if op == "whiten":
            return self.Linv(X)
        if op == "invunwhiten":
            return self.Rinv(X)
        if op == "mul":
            return self.L(self.R(X))
        if op == "solve":
            return self.Rinv(self.Linv(X))
        r = self.R(X) if op == "quad" else self.Linv(X)
        assert op in ("quad", "invquad"), op
        return np.sum(r * r, axis=0)


def diag_parts(alpha, S, Y, D):
    """(diag W, its scale) in long double: alpha_i + b_i'D b_i and alpha_i + |b_i|'|D| |b_i|, B = [alpha . Y, S] from the trace's columns"""
    a = np.asarray(alpha, dtype=LD)
    B = np.hstack([a[:, None] * np.asarray(Y, dtype=LD), np.asarray(S, dtype=LD)])
    D = np.asarray(D, dtype=LD).reshape(B.shape[1], B.shape[1])
    return a + np.sum((B @ D) * B, axis=1), np.abs(a) + np.sum((np.abs(B) @ np.abs(D)) * np.abs(B), axis=1)


# ---- the checks --------------------------------------------------------------------------------------------------------------------------
def _ratio(dev, bound):
    """max of dev / bound as a float; where the bound is zero the value must be exact; a NaN deviation is inf"""
    return float(np.max(fr._ratio(dev, np.asarray(bound, dtype=LD) / EPS), initial=0.0))


def op_ratios(ops, kpad, op, X, out):
    """{check name: largest |deviation| / bound} of `out`, the surface's result of `op` on the columns of X (d, N), on the factor `ops`"""
    d = ops.d
    Cl, Cs = c_lane(d, kpad), c_solve(d, kpad)
    X = np.asarray(X, dtype=LD)
    Xa = np.abs(X)
    O = np.asarray(out, dtype=LD)
    if op in ("unwhiten", "rmul"):
        S = ops.L_abs(Xa) if op == "unwhiten" else ops.R_abs(Xa)
        return {op: _ratio(np.abs(O - ops.apply(op, X)), Cl * EPS * S)}
    if op == "whiten":
        ref = ops.Linv(X)
        return {"whiten": _ratio(np.abs(ops.L(O) - X), Cs * EPS * ops.L_abs(np.abs(O)) + ops.nonorth_L(X)),
                "whiten_fwd": _ratio(np.abs(O - ref), Cs * EPS * ops.S_Linv(X, ref))}
    if op == "invunwhiten":
        return {"invunwhiten": _ratio(np.abs(ops.R(O) - X), Cs * EPS * ops.R_abs(np.abs(O)) + ops.nonorth_R(X)),
                "invunwhiten_fwd": _ratio(np.abs(O - ops.Rinv(X)), Cs * EPS * ops.S_Rinv(X))}
    if op == "mul":
        return {op: _ratio(np.abs(O - ops.apply(op, X)), 2 * Cl * EPS * ops.L_abs(ops.R_abs(Xa)))}
    if op == "solve":
        t = ops.Linv(X)
        return {op: _ratio(np.abs(O - ops.Rinv(t)), Cs * EPS * (ops.S_Rinv(t) + ops.Rinv_abs(ops.S_Linv(X, t))))}
    assert op in ("quad", "invquad"), op
    r = ops.R(X) if op == "quad" else ops.Linv(X)
    S, C = (ops.R_abs(Xa), Cl) if op == "quad" else (ops.S_Linv(X, r), Cs)
    q = np.sum(r * r, axis=0)
    return {op: _ratio(np.abs(O - q), 2 * np.sum(np.abs(r) * (C * EPS * S), axis=0) + (d + 4) * EPS * q)}


def diag_ratio(kpad, out, alpha, S, Y, D):
    ref, scale = diag_parts(alpha, S, Y, D)
    return {"diag": _ratio(np.abs(np.asarray(out, dtype=LD) - ref), c_diag(kpad) * EPS * scale)}


# ---- the float64 mirror of pf_woodbury_kernel<KPAD, MODE> ---------------------------------------------------------------------------------
STALE = 0.37                      # what a dropped i < d guard reads past the column and past the factor's rows in the mirror


def mirror(M, kpad, mode, x, fault=None):
    """one column x (d,) through mode 0 .. 3 of the lane kernel on the float64 factor M, padded to kpad"""
    d, k = M.d, M.k
    assert k <= kpad and M.dt == np.float64
    T, V = np.zeros((kpad, kpad)), np.eye(kpad)
    T[:k, :k], V[:k, :k] = M.T, M.V
    nrow = max(d, kpad)
    Vh = np.full((nrow, kpad), STALE)
    Vh[:d] = 0.0
    Vh[:d, :k] = M.Vh
    x = np.concatenate([np.asarray(x, dtype=np.float64), np.full(nrow - d, STALE)])
    s = np.concatenate([M.s, np.ones(nrow - d)])
    rows = kpad if fault == "head_guard_dropped" else min(d, kpad)          # the head rows the guards let through
    pre = {1: lambda v, i: v / s[i], 2: lambda v, i: v * s[i]}.get(mode, lambda v, i: v)
    post = {0: lambda v, i: v * s[i], 3: lambda v, i: v / s[i]}.get(mode, lambda v, i: v)
    if fault == "no_sqrt_alpha":
        pre = post = lambda v, i: v
    elif fault == "sqrt_alpha_wrong_side":
        pre, post = post, pre
    fam_a = mode in (0, 3)
    if fault == "T_for_Tt":
        fam_a = not fam_a
    zh = np.zeros(kpad)
    for i in range(rows):
        zh[i] = pre(x[i], i)
    def head_Vt():                                              # head <- V'head, in place from the last row
        for a in range(kpad - 1, -1, -1):
            zh[a] = _dot(V[:a + 1, a], zh[:a + 1])

    def head_V():                                               # head <- V head, in place from the first row
        for a in range(kpad):
            zh[a] = _dot(V[a, a:], zh[a:])

    if fault == "V_for_Vt":
        head_V, head_Vt = head_Vt, head_V
    if mode == 0:                                               # z_head = V'x_head
        head_Vt()
    elif mode == 3:                                             # z_head = V^-1 x_head (back substitution)
        if fault == "fwd_for_back":
            for a in range(kpad):
                zh[a] = (zh[a] - _dot(V[a, :a], zh[:a])) / V[a, a]
        else:
            for a in range(kpad - 1, -1, -1):
                zh[a] = (zh[a] - _dot(V[a, a + 1:], zh[a + 1:])) / V[a, a]
    t0 = kpad + 1 if fault == "tail_from_kpad_plus_1" else kpad
    w = np.zeros(kpad)
    for i in range(rows):
        w += Vh[i] * zh[i]
    for i in range(t0, d):
        w += Vh[i] * pre(x[i], i)
    tv = np.array([_dot(T[a, a:], w[a:]) if fam_a else _dot(T[:a + 1, a], w[:a + 1]) for a in range(kpad)])
    for i in range(kpad):
        zh[i] = _sub_dot(zh[i], Vh[i], tv) if i < rows else 0.0
    if mode == 1:                                               # head <- V'^-1 head (forward substitution)
        for a in range(kpad):
            zh[a] = (zh[a] - _dot(V[:a, a], zh[:a])) / V[a, a]
    elif mode == 2:                                             # head <- V head
        head_V()
    out = np.zeros(d)
    for i in range(min(d, kpad)):
        out[i] = post(zh[i], i)
    for i in range(t0, d):
        out[i] = post(_sub_dot(pre(x[i], i), Vh[i], tv), i)
    return out


def _dot(a, b):
    s = 0.0
    for u, v in zip(a, b):
        s += u * v
    return s


def _sub_dot(v, row, tv):
    for u, t in zip(row, tv):
        v -= u * t
    return v


def mirror_op(M, kpad, op, x, fault=None):
    """one column through one of the eight ops as pfmi_woodbury_apply composes them from the four modes"""
    y = np.asarray(x, dtype=np.float64)
    for mode in LAUNCHES[op]:
        y = mirror(M, kpad, mode, y, fault)
    if op in ("quad", "invquad"):
        s = 0.0
        for v in y:
            s += v * v
        return s
    return y


def mirror_diag(kpad, alpha, theta, grad, src, D, fault=None):
    """pf_woodbury_diag_kernel<KPAD> in float64: b from the trace (theta, grad: (length, d); src: hist_src[:j]), D (2j x 2j) padded"""
    alpha = np.asarray(alpha, dtype=np.float64)
    d, j = len(alpha), len(src)
    Dp = np.zeros((kpad, kpad))
    Dp[:2 * j, :2 * j] = np.asarray(D, dtype=np.float64).reshape(2 * j, 2 * j)
    if fault == "diag_offdiag_dropped":
        Dp[:j, j:] = 0.0
        Dp[j:, :j] = 0.0
    out = np.empty(d)
    for i in range(d):
        b = np.zeros(kpad)
        for c, q in enumerate(src):
            b[c] = alpha[i] * (grad[q, i] - grad[q + 1, i])
            b[j + c] = theta[q + 1, i] - theta[q, i]
        q = 0.0
        for a in range(kpad):
            q += b[a] * _dot(Dp[a], b)
        out[i] = alpha[i] + q
    return out


# ---- the grid of tests/test_gpu_woodbury.py --------------------------------------------------------------------------------------------------
GRID_J = (2, 4, 6, 8, 10, 16, 32)                               # every KPAD: 4, 8, 12, 16, 20, 32, 64
GRID_N = 9
D_TAIL = 300


def grid_dims(kpad):
    return (2, kpad - 1, kpad, kpad + 1, D_TAIL)


def _grid():
    out = []
    for J in GRID_J:
        kp = H.kpad_for(J)
        for regime in ("plain",) + (("scaled", "dep") if kp in (12, 32) else ()):
            for d in grid_dims(kp):
                out.append((d, J, regime))
    return out


GRID = _grid()


def case_id(case):
    return "d%d-J%d-%s" % case


def grid_case(case):
    """the fit_reference.Case of a grid entry: two traces of J + 4 and J + 2 points"""
    d, J, regime = case
    return fr.make_case(d, J, regime, 700 + 13 * d + J)


def grid_points(case, lengths):
    """(trace, point in trace) of the fits a case checks: every fit at d <= KPAD + 1; at d = D_TAIL the points 0, 1, J // 2, J, last"""
    d, J, _ = case
    if d <= H.kpad_for(J) + 1:
        return [(k, l) for k, n in enumerate(lengths) for l in range(n)]
    return [(k, l) for k, n in enumerate(lengths) for l in sorted({0, 1, J // 2, J, n - 1})]


def grid_needs(case):
    """the kinds of fit a case must contain and check, as predicates on j_eff"""
    d, J, _ = case
    needs = {"j_eff == 0": lambda j: j == 0, "0 < j_eff < J": lambda j: 0 < j < J, "j_eff == J": lambda j: j == J}
    if d < 2 * J:
        needs["2 j_eff > d"] = lambda j: 2 * j > d
    return needs


def grid_X(case, p):
    """(d, GRID_N) Gaussian entries with log-normal magnitudes"""
    d, J, _ = case
    rng = np.random.default_rng(1000 * J + 7 * d + p)
    return np.asfortranarray(rng.standard_normal((d, GRID_N)) * np.exp(2.0 * rng.standard_normal((d, GRID_N))))
