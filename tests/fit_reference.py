"""Extended-precision reference of the fit stage, a conditioning-free backward-error check of its factor, and a Python mirror of its
dispatch.  Not collected by pytest; used by tests/test_gpu_fit_reference.py and pinned on the CPU by tests/test_fit_reference_cpu.py.

  pf_fit_reg_kernel<KPAD, RPT, 256>     the register-resident kernel          (pathfinder.jl_amd/csrc/fit_kernels.hip)
  pf_fit_kernel<KPAD>                   the general column-by-column kernel   (pathfinder.jl_amd/csrc/fit_kernels.hip)
  pf_fit_tsqr_kernel<MC, RC>            TSQR + Householder reconstruction     (pathfinder.jl_amd/csrc/fit_tsqr_kernel.hip)
  pf_fit_panel_kernel<NT16, RPT, PW>    the left-looking panel kernel         (pathfinder.jl_amd/csrc/fit_panel_kernel.hip)

All four perform the same operation on one trace point (src/inverse_hessian.jl:98-133, src/woodbury.jl:201-207).  With alpha (d), the
history S, Y (d x j, oldest first), theta and g = grad logp(theta):
    B = [alpha . Y, S]              R = triu(S'Y)       D = [0, -R^-1; -R^-T, R^-T (diag R + Y' alpha Y) R^-1]
    s = sqrt(alpha)                 B~ = B / s          B~ = Q R_qr (Householder, k = min(d, 2 j) reflectors Vh, compact-WY T)
    C = I + R_qr D R_qr' = V'V      logdet = 2 sum log s + 2 sum log V_cc          mu = theta + s . W~ (s . g),  W~ = I + B~ D B~'
FitRef restates, in np.longdouble and from the kernel's own inputs (alpha as the history walk left it, S and Y in the order of
hist_src), B, D, B~ D B~', logdet (through the m x m identity det(I + B~ D B~') = det(I_m + D B~'B~), an LU in long double: no QR, no
Cholesky) and mu.  check_fit compares one fit (a pfmi_get_fit dictionary) with it.

What is asserted (eps = 2^-52, i.e. TWO unit roundoffs per counted step; L = the length of the kernel's longest accumulation chain
over the d rows, `chain(plan, d)` below):
  B      |B - B_ref| <= C_B eps |B_ref|, C_B = 1: alpha_i (g - g') is two roundings, theta' - theta one; B.shape == (d, 2 j).
  D      |D - D_ref| <= C_D eps S_D, C_D = 2 L + 4 j + 16.  S_D is the standard forward bound of a triangular inverse carried through
         the three blocks: with |R|_a = triu(|S|'|Y|) (the sum S'Y with every term in absolute value: its rounding error is L eps of
         that), P = |R^-1| |R|_a |R^-1| bounds the error of R^-1, so S_D12 = P, S_D21 = P', S_D22 = P' M_a |R^-1| + |R^-1|' M_a P
         + |R^-1|' M_a |R^-1| with M_a = |diag R| + |Y|' alpha |Y|; S_D11 = 0 and S_D is zero below the diagonal of D12: those
         entries are exact zeros.  This is the only check that grows with cond(R), and the scale carries it.  2 L: the chains of S'Y
         and Y' alpha Y; 4 j: the back substitution and the two products of D22, j terms each; 16: input roundings.
  W      |Q_k (V'V - I) Q_k' - B~ D B~'|_ij <= C_W eps sqrt(S_ii S_jj),  S = I + |B~| |D| |B~|',  C_W = m (L + 6) + 16, m = 2 j.
         Both sides in long double from the fit's OWN arrays: Q_k = (I - Vh T Vh') E_k from its reflectors and its T, V its Cholesky
         factor, B~ = B / sqrt(alpha) and D its own.  This is the columnwise backward error of Householder QR (a column passes through
         at most m reflectors; each costs one d-long dot product, L steps, and an update, 3 steps) followed by R D R' (two m-term
         contractions) and a Cholesky factorisation (m terms): m (L + 3) + 3 m + 16.  It holds whatever the conditioning of B~: a
         Householder QR is backward stable at a rank-deficient block too, and so is the Householder reconstruction of the TSQR kernel.
         There is no conditioning gate and no cond(D) allowance.  The error is row-normwise (Q mixes the rows), hence sqrt(S_ii S_jj)
         and not the elementwise (|B~| |D| |B~|')_ij.
  Q      |Q_k'Q_k - I| <= C_Q eps,  C_Q = m (L + 6) + 16: the same reflectors; T from Vh'Vh (L steps) and an m-term recursion.
  logdet |logdet - ref| <= C_l eps (1 + 2 sum |log s_i| + 2 sum |log V_cc|),  C_l = C_W + L + 2 k + 16: the chain of sum log s (L), the
         k logarithms and their sum, and the factor's backward error, which reaches logdet through tr(C^-1 Q_k' dW Q_k).
  mu     |mu - ref|_i <= C_m eps (|theta_i| + s_i sqrt(S_ii) sum_j sqrt(S_jj) s_j |g_j|),  C_m = C_W + C_D + 2 L + 16: the factor's
         backward error applied to s . g row-normwise, the two d-long contractions of the mean (Q'(s . g) and the sum over j), and the
         kernel's D against the reference's.
  status, j_eff, n_rejected: array-equal with the oracle's history walk.
The chains, as read from the kernels (pf_block_sum / pf_block_sum_pp / pf_block_sum_mv of pfmi_common.h: 6 adds inside a wave, then
one add per further wave):
  reg    L = RPT + 10           a thread owns rows tid + 256 i, i < RPT (one fma per row), 6 + 3 adds across the 4 waves
  gen    L = ceil(d / 256) + 10 the same with the rows in global memory
  panel  L = ceil(d / 512) + 14 512 threads: 6 + 7 adds across the 8 waves
  tsqr   L = RC + ceil(d / 512) + 28: a chunk's QR sums RC rows per thread and 8 waves (14), the stack of the chunks' R factors is one
         more QR over at most one row per thread (14), the mean and logdet sum ceil(d / 512) rows per thread
  oracle L = d                  oracle/pf_oracle.c sums row after row
"""
import collections

import numpy as np

import scan_reference as sr
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON   # noqa: F401  (one long-double skip convention for the suite)
from oracle import pf_oracle as po

LD = sr.LD
EPS = sr.EPS64
KPADS = (4, 8, 12, 16, 20, 32, 64)
FP_NT = 512                                                    # fit_panel_kernel.hip
TS_NT, TS_STACK = 512, 512                                     # fit_tsqr_kernel.hip
TS_RC = {8: 8, 12: 5, 16: 4, 20: 3, 32: 2}                     # pf_launch_fit_tsqr: rows per thread of a chunk


def kpad_for(J):
    return next(o for o in KPADS if 2 * J <= o)


# ---- synthetic histories -----------------------------------------------------------------------------------------------------------
def quad_history(d, lengths, cond, dep, seed, bad=None):
    """K = len(lengths) traces of random-walk steps on the quadratic logp = -theta'H theta / 2, H = diag(h) + A A' (rank <= 2):
    theta[l + 1] = theta[l] + s_l, grad = -H theta, so y = H s and every s'y > 0.  h is log-uniform with max / min <= cond (scaled
    rows); dep: s_l = s_{l - 1} + dep . noise (a nearly rank-deficient block), None: independent steps.  bad = (l, i, value) plants
    a non-finite value in gradient component i of point l of the first trace.  Returns (thetas, grads), lists of (length, d)."""
    rng = np.random.default_rng(seed)
    h = np.exp((rng.uniform(size=d) - 0.5) * np.log(cond))
    r = min(2, d)
    A = 0.5 * np.sqrt(h)[:, None] * rng.normal(size=(d, r)) / np.sqrt(d)
    thetas, grads = [], []
    for n in lengths:
        th = np.empty((n, d))
        th[0] = rng.normal(size=d)
        s = 0.1 * rng.normal(size=d)
        for l in range(1, n):
            if l > 1:
                s = s + dep * 0.1 * rng.normal(size=d) if dep else 0.1 * rng.normal(size=d)
            th[l] = th[l - 1] + s
        gr = -(h[None, :] * th + (th @ A) @ A.T)
        thetas.append(th)
        grads.append(gr)
    if bad is not None:
        l, i, v = bad
        grads[0][l, i] = v
    return thetas, grads


def history_columns(theta, grad, src):
    """S, Y (d x j) of one fit: the pairs `src` (hist_src[l, :j], oldest first) of a trace (theta, grad: (length, d))"""
    d = theta.shape[1]
    if len(src) == 0:
        return np.zeros((d, 0)), np.zeros((d, 0))
    S = np.stack([theta[s + 1] - theta[s] for s in src], axis=1)
    Y = np.stack([grad[s] - grad[s + 1] for s in src], axis=1)
    return S, Y


# ---- small long-double linear algebra ----------------------------------------------------------------------------------------------
def _triu_inv(R):
    """inverse of an upper-triangular matrix by back substitution, in its own dtype"""
    n = R.shape[0]
    X = np.zeros_like(R)
    for c in range(n):
        X[c, c] = 1 / R[c, c]
        for a in range(c - 1, -1, -1):
            X[a, c] = -(R[a, a + 1:c + 1] @ X[a + 1:c + 1, c]) / R[a, a]
    return X


def _logdet_lu(A):
    """(log |det A|, sign) by Gaussian elimination with partial pivoting, in A's dtype"""
    A = A.copy()
    n = A.shape[0]
    ld, sign = A.dtype.type(0), 1
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]] = A[[p, c]]
            sign = -sign
        piv = A[c, c]
        if piv == 0:
            return A.dtype.type(-np.inf), 0
        if piv < 0:
            sign = -sign
        ld += np.log(np.abs(piv))
        if c + 1 < n:
            A[c + 1:, c + 1:] -= np.outer(A[c + 1:, c] / piv, A[c, c + 1:])
    return ld, sign


class FitRef:
    """the long-double reference of one fit from the kernel's inputs: alpha (d), S, Y (d x j), theta, g (d)"""

    def __init__(self, alpha, S, Y, theta, g):
        a = np.asarray(alpha, dtype=LD)
        S, Y = np.asarray(S, dtype=LD), np.asarray(Y, dtype=LD)
        d, j = S.shape
        self.d, self.j, self.m = d, j, 2 * j
        self.s = np.sqrt(a)
        self.theta, self.g = np.asarray(theta, dtype=LD), np.asarray(g, dtype=LD)
        self.B = np.hstack([a[:, None] * Y, S])
        m = 2 * j
        D, SD = np.zeros((m, m), dtype=LD), np.zeros((m, m), dtype=LD)
        if j:
            R = np.triu(S.T @ Y)
            Ra = np.triu(np.abs(S).T @ np.abs(Y))
            Ri = _triu_inv(R)
            Ria = np.abs(Ri)
            M = np.diag(np.diag(R)) + Y.T @ (a[:, None] * Y)
            Ma = np.diag(np.abs(np.diag(R))) + np.abs(Y).T @ (a[:, None] * np.abs(Y))
            P = Ria @ Ra @ Ria
            D[:j, j:], D[j:, :j], D[j:, j:] = -Ri, -Ri.T, Ri.T @ M @ Ri
            SD[:j, j:], SD[j:, :j] = P, P.T
            SD[j:, j:] = P.T @ Ma @ Ria + Ria.T @ Ma @ P + Ria.T @ Ma @ Ria
            self.R = R
        self.D, self.S_D = D, SD
        Bt = self.B / self.s[:, None]
        ld, sign = _logdet_lu(np.eye(m, dtype=LD) + D @ (Bt.T @ Bt)) if m else (LD(0), 1)
        self.sign = sign
        self.logdet = 2 * np.sum(np.log(self.s)) + ld
        with np.errstate(invalid="ignore"):                    # a non-finite gradient gives a non-finite reference mean
            self.mu = self.theta + a * self.g + self.B @ (D @ (self.B.T @ self.g))


# ---- the rows of the factor check ------------------------------------------------------------------------------------------------------
EDGE_ROWS = (0, 63, 64, 255, 256, 257, 511, 512, 513, 767, 768)


def check_rows(d, plan, seed=0):
    """d <= 256: every row.  Larger d: the edges of every tid + NT i slot of the register kernel, 16 seeded rows and, above 1024, the
    rows either side of the chunk boundaries of the plan that ran (TSQR: 512 RC rows a chunk; panel: FP_NT rows a slot)."""
    if d <= 256:
        return np.arange(d)
    rows = {r for r in EDGE_ROWS if r < d} | {d - 1}
    rows |= {int(r) for r in np.random.default_rng(seed + d).choice(d, 16, replace=False)}
    if d > 1024 and plan:
        fam, inst = plan.split(":")[1], plan.split(":")[2].split(",")
        step = TS_NT * TS_RC[int(inst[0])] if fam == "tsqr" else FP_NT if fam == "panel" else 256
        for b in list(range(step, d, step))[:8] + [((d - 1) // step) * step]:
            rows |= {r for r in (b - 1, b, b + 1) if 0 <= r < d}
    return np.array(sorted(rows), dtype=np.int64)


# ---- chains and constants ---------------------------------------------------------------------------------------------------------------
def chain(plan, d):
    """L: the longest accumulation chain over the d rows of the kernel `plan` names ("oracle": row after row)"""
    if plan == "oracle":
        return d
    fam, inst = plan.split(":")[1], [int(v) for v in plan.split(":")[2].split(",")]
    if fam == "reg":
        return inst[1] + 10
    if fam == "gen":
        return -(-d // 256) + 10
    if fam == "panel":
        return -(-d // FP_NT) + 14
    assert fam == "tsqr", plan
    return TS_RC[inst[0]] + -(-d // TS_NT) + 28


def constants(plan, d, j):
    L, m = chain(plan, d), 2 * j
    k = min(d, m)
    c_w = m * (L + 6) + 16
    c_d = 2 * L + 4 * j + 16
    return {"B": 1, "D": c_d, "W": c_w, "Q": c_w, "logdet": c_w + L + 2 * k + 16, "mu": c_w + c_d + 2 * L + 16}


def _ratio(dev, scale):
    """dev / (eps scale) elementwise as float64; where the scale is zero the entry must be exact (ratio 0 or inf)"""
    dev, scale = np.asarray(dev, dtype=LD), np.asarray(scale, dtype=LD)
    out = np.zeros(dev.shape)
    nz = scale > 0
    out[nz] = (dev[nz] / (EPS * scale[nz])).astype(np.float64)
    out[~nz & (dev != 0)] = np.inf
    out[np.isnan(dev)] = np.inf
    return out


def factor_parts(f):
    """(s, Vh, T, V, Bt, D) of a pfmi_get_fit dictionary in long double; k = min(d, 2 j)"""
    d = len(f["alpha"])
    m = f["B"].shape[1]
    k = min(d, m)
    s = np.sqrt(np.asarray(f["alpha"], dtype=np.float64)).astype(LD)          # the kernels' sqrt is correctly rounded
    Vh = np.zeros((d, k), dtype=LD)
    for c in range(k):
        Vh[c, c] = 1
        Vh[c + 1:, c] = np.asarray(f["qr_factors"][c + 1:, c], dtype=LD)
    T = np.triu(np.asarray(f["T"], dtype=LD)[:k, :k])
    V = np.triu(np.asarray(f["V"], dtype=LD)[:k, :k])
    Bt = np.asarray(f["B"], dtype=LD) / s[:, None]
    return s, Vh, T, V, Bt, np.asarray(f["D"], dtype=LD)


def qr_ratio(f):
    """min / max |diag R_qr| of the fit's own QR (1 when there is no history): how close to rank deficient the block is"""
    d, m = f["qr_factors"].shape if f["B"].shape[1] else (len(f["alpha"]), 0)
    k = min(d, m)
    if not k:
        return 1.0
    dg = np.abs(np.diag(f["qr_factors"])[:k])
    return float(dg.min() / dg.max()) if dg.max() > 0 else 0.0


def fit_ratios(f, ref, rows):
    """the six deviations of fit f (a pfmi_get_fit dictionary) in units of eps x scale: {name: (largest ratio, its index)}.  ref: the
    FitRef of the same inputs; rows: the rows of the factor check."""
    d, m = ref.d, ref.m
    k = min(d, m)
    assert f["B"].shape == (d, m) and f["D"].shape == (m, m), (f["B"].shape, f["D"].shape, d, m)
    s, Vh, T, V, Bt, D = factor_parts(f)
    out = {}

    def put(name, r):
        r = np.atleast_1d(r)
        i = int(np.argmax(r)) if r.size else 0
        out[name] = (float(r.reshape(-1)[i]) if r.size else 0.0, tuple(int(v) for v in np.unravel_index(i, r.shape)) if r.size else ())

    put("B", _ratio(np.abs(np.asarray(f["B"], dtype=LD) - ref.B), np.abs(ref.B)))
    put("D", _ratio(np.abs(D - ref.D), ref.S_D))
    Sd = 1 + np.sum((np.abs(Bt) @ np.abs(D)) * np.abs(Bt), axis=1)                       # diag of I + |B~| |D| |B~|'
    if k:
        Qk = -Vh @ (T @ Vh[:k].T)
        Qk[np.arange(k), np.arange(k)] += 1
        Cf = V.T @ V - np.eye(k, dtype=LD)
        dW = (Qk[rows] @ Cf) @ Qk.T - (Bt[rows] @ D) @ Bt.T
        put("W", _ratio(np.abs(dW), np.sqrt(Sd[rows][:, None] * Sd[None, :])))
        put("Q", _ratio(np.abs(Qk.T @ Qk - np.eye(k, dtype=LD)), np.ones((k, k))))
    else:
        put("W", np.zeros(1))
        put("Q", np.zeros(1))
    ldscale = 1 + 2 * np.sum(np.abs(np.log(s))) + (2 * np.sum(np.abs(np.log(np.abs(np.diag(V))))) if k else 0)
    put("logdet", _ratio(np.abs(LD(float(f["logdet"])) - ref.logdet), ldscale))
    sg = np.sum(np.sqrt(Sd) * s * np.abs(ref.g))
    put("mu", _ratio(np.abs(np.asarray(f["mu"], dtype=LD) - ref.mu), np.abs(ref.theta) + s * np.sqrt(Sd) * sg))
    return out


def fit_report(f, ref, plan, rows=None):
    """(ratios, bad) of one fit: {name: (largest deviation / (eps scale), C)} and the subset that exceeds its C.  At a point whose own
    gradient is not finite the mean is not finite either (reported under "mu_finite" when it is) and every other quantity, none of
    which reads that gradient, is reported as usual."""
    rows = check_rows(ref.d, plan) if rows is None else rows
    C = constants(plan, ref.d, ref.j)
    r = fit_ratios(f, ref, rows)
    bad = {}
    if not np.all(np.isfinite(np.asarray(ref.g, dtype=np.float64))):
        C.pop("mu")
        if np.all(np.isfinite(f["mu"])):
            bad["mu_finite"] = "finite mean from a non-finite gradient"
    rep = {nm: (r[nm][0], C[nm]) for nm in C}
    bad.update({nm: (r[nm], C[nm]) for nm in C if not r[nm][0] <= C[nm]})
    return rep, bad


def check_fit(f, ref, plan, rows=None, ctx=None):
    """assert every bound on one fit; returns {name: ratio / C}"""
    rep, bad = fit_report(f, ref, plan, rows)
    assert not bad, (plan, ctx, bad)
    return {nm: v / c for nm, (v, c) in rep.items()}


# ---- the double oracle in pfmi_get_fit's conventions ---------------------------------------------------------------------------------------
def oracle_fit(alpha, S, Y, theta, g):
    """the fit of oracle/pf_oracle.c as a pfmi_get_fit dictionary (T: LAPACK's dlarft from its reflectors and tau in long double, rounded
    to double, as tests/draw_reference.py forms it) and its status"""
    B, D = po.lbfgs_inverse_hessian(alpha, S, Y)
    F = po.Factor(alpha, B, D)
    mu = F.fit_mean(theta, g) if F.status == 0 else np.full(F.d, np.nan)
    k, m = F.k, F.m
    T = sr.LDFactor(F, mu).Tw.astype(np.float64)
    return dict(alpha=np.array(alpha, dtype=np.float64), B=np.asfortranarray(F.B), D=np.asfortranarray(F.D),
                qr_factors=np.asfortranarray(F.QR[:, :m]), T=np.asfortranarray(T), V=np.asfortranarray(F.V[:k, :k]), mu=np.array(mu),
                logdet=F.logdet, j=m // 2), F.status


# ---- mutations: wrong fits the bounds must catch ---------------------------------------------------------------------------------------------
# name -> the bound it must break
MUTATIONS = {"vh_rows_scaled": "W", "t_offdiag_zero": "Q", "v_transposed": "W", "logdet_row_dropped": "logdet", "mu_alpha_for_sqrt": "mu",
             "b_s_columns_swapped": "B", "d22_without_diag_r": "D", "mu_head_dropped": "mu"}


def mutate(f, ref, name):
    """a copy of the double fit f (d > 256, j >= 2) with one slip of the kind an RPT > 1 kernel could make"""
    g = {k: (np.array(v, order="F") if isinstance(v, np.ndarray) else v) for k, v in f.items()}
    d, j = ref.d, ref.j
    s = np.sqrt(g["alpha"])
    if name == "vh_rows_scaled":                               # the rows tid + 256 i, i >= 1, of the reflectors
        k = min(d, 2 * j)
        g["qr_factors"][256:, :k] *= 1 + 1e-9
    elif name == "t_offdiag_zero":
        T = np.triu(g["T"], 1)
        a, b = np.unravel_index(np.argmax(np.abs(T)), T.shape)
        assert T[a, b] != 0
        g["T"][a, b] = 0.0
    elif name == "v_transposed":
        g["V"] = np.asfortranarray(np.triu(g["V"]).T)
    elif name == "logdet_row_dropped":
        i = int(np.argmax(np.abs(np.log(s[256:])))) + 256
        g["logdet"] = g["logdet"] - 2 * np.log(s[i])
    elif name == "mu_alpha_for_sqrt":                          # row i: theta_i + alpha_i (W~ (s . g))_i
        i = 256 + int(np.argmax(np.abs(s[256:] - 1) * np.abs(g["mu"][256:] - np.asarray(ref.theta[256:], dtype=np.float64))))
        g["mu"][i] = float(ref.theta[i]) + s[i] * (g["mu"][i] - float(ref.theta[i]))
    elif name == "b_s_columns_swapped":
        g["B"][:, [j, j + 1]] = g["B"][:, [j + 1, j]]
    elif name == "d22_without_diag_r":
        Ri = _triu_inv(np.asarray(ref.R, dtype=np.float64))
        g["D"][j:, j:] -= Ri.T @ np.diag(np.diag(np.asarray(ref.R, dtype=np.float64))) @ Ri
    elif name == "mu_head_dropped":                            # x = s.g - Vh (t1 + t2) + e_head (V'V head - head), head = Q_k'(s . g): the last term
        _, Vh, T, V, _, _ = factor_parts(f)                    # is added by the i == 0 slot of the register kernel only
        k = min(d, 2 * j)
        Qk = -Vh @ (T @ Vh[:k].T)
        Qk[np.arange(k), np.arange(k)] += 1
        head = Qk.T @ (ref.s * ref.g)
        g["mu"][:k] -= np.asarray(ref.s[:k] * (V.T @ (V @ head) - head), dtype=np.float64)
    else:
        raise KeyError(name)
    return g


# ---- Python mirror of the dispatch (pf_launch_fit, launch_fit_t, pf_launch_fit_tsqr, pf_launch_fit_panel) ----------------------------------------
def plan_for(d, J, force=None):
    """the plan ONE fit_batch(J) launch takes at dimension d; force = PFMI_FIT_KERNEL ("mem", "panel", "tsqr") or None"""
    kp = kpad_for(J)
    f = force[0] if force else ""
    if d > 1024:
        if f not in ("m", "p") and d <= 32768 and kp in TS_RC and not (kp == 32 and d < 4096 and f != "t"):
            nch = -(-d // (TS_NT * TS_RC[kp]))
            if nch * kp <= TS_STACK:
                return f"fit:tsqr:{kp}"
        if f != "m" and d <= 32 * FP_NT and 8 <= kp <= 32:
            rpt = -(-d // FP_NT)
            bucket, cols = (5, 4) if rpt <= 5 else (10, 4) if rpt <= 10 else (20, 4) if rpt <= 20 else (32, 2)
            return f"fit:panel:{kp},{bucket},{cols}"
    if kp <= 16 and f != "m" and d <= 1024:
        return f"fit:reg:{kp},{1 if d <= 256 else 2 if d <= 512 else 4}"
    return f"fit:gen:{kp}"


PANEL_BUCKETS = ((5, 4), (10, 4), (20, 4), (32, 2))
ALL_PLANS = ([f"fit:reg:{kp},{rpt}" for kp in (4, 8, 12, 16) for rpt in (1, 2, 4)] + [f"fit:gen:{kp}" for kp in KPADS]
             + [f"fit:tsqr:{kp}" for kp in TS_RC] + [f"fit:panel:{kp},{b},{c}" for kp in TS_RC for b, c in PANEL_BUCKETS])
# Nothing that exists is out of reach: the register kernel has no KPAD above 16 and the large-d kernels none of 4 or 64 (those shapes
# run the general kernel, which is why fit:gen:<KPAD> has every KPAD); the panel kernel at KPAD 8 .. 20 and the TSQR kernel at KPAD 32
# below d = 4096 are reached through PFMI_FIT_KERNEL.
EXCLUDED = {}
REACHABLE = [nm for nm in ALL_PLANS if nm not in EXCLUDED]


# ---- the grid --------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "d J lengths cond dep seed force bad", defaults=(None, None))
REGIMES = {"scaled": (1e4, None), "dep": (10.0, 1e-5), "plain": (10.0, None)}
J_FULL = {4: 2, 8: 4, 12: 6, 16: 8}
J_RAGGED = {4: 1, 8: 3, 12: 5, 16: 7}
RPT_EDGES = {1: (1, 256, (3, 63, 65, 255)), 2: (257, 512, (511, 257, 511, 257)), 4: (513, 1024, (1023, 513, 1023, 513))}


def make_case(d, J, regime, seed, K=2, force=None, bad=None, points=None):
    cond, dep = REGIMES[regime]
    n = J + 4 if points is None else points
    lengths = (n, n - 2)[:K]
    return Case(d, J, lengths, cond, dep, seed, force, bad)


def _grid():
    out, rot, seed = [], 0, 0
    names = ("scaled", "dep", "plain")

    def add(d, J, K=2, force=None, bad=None, points=None, regime=None):
        nonlocal rot, seed
        out.append(make_case(d, J, regime or names[rot % 3], 100 + seed, K, force, bad, points))
        rot += regime is None
        seed += 1

    # register kernel: every (KPAD, RPT) at its lowest and highest d with the full J, one odd d with the ragged J
    for ki, kp in enumerate((4, 8, 12, 16)):
        for rpt in (1, 2, 4):
            lo, hi, odd = RPT_EDGES[rpt]
            add(lo, J_FULL[kp])
            add(hi, J_FULL[kp], regime="dep")                 # every (KPAD, RPT) sees a dependent block
            add(odd[ki], J_RAGGED[kp])
    add(2, 4)                                                  # the RPT = 1 edges the covering above has not placed
    add(64, 6)
    # general kernel where it is the default: KPAD 20, 32, 64
    for Ja, Jb in ((10, 9), (16, 11), (17, 32)):
        add(1, Ja)
        add(1024, Ja, regime="dep")
        add(65, Jb)
        add(257, Jb)
    for kp in (4, 8, 12, 16):                                  # and forced at KPAD 4 .. 16
        add(64, J_FULL[kp], force="mem")
        add(513, J_RAGGED[kp], force="mem", regime="dep" if kp == 8 else None)
    add(1025, 2, K=1)                                          # d > 1024 at KPAD 4 / 64: no large-d kernel takes them
    add(1025, 17, K=1, points=12)
    # TSQR: KPAD 8 .. 20 at d = 1025 and at one row past a full chunk; KPAD 32 at d = 4096, forced at 1025
    for kp, J in ((8, 4), (12, 6), (16, 8), (20, 10)):
        add(1025, J, K=1, regime="dep" if kp in (8, 16) else None)
        add(TS_NT * TS_RC[kp] + 1, J, K=1, points=8)
    add(4096, 16, K=1, points=10, regime="dep")
    add(1025, 11, K=1, force="tsqr")
    # panel: every KPAD at d = 1025 (the default at KPAD 32) and one row past each bucket boundary
    for kp, J in ((8, 4), (12, 6), (16, 8), (20, 10), (32, 16)):
        add(1025, J, K=1, force=None if kp == 32 else "panel", regime="dep" if kp in (12, 32) else None)
        for bi, b in enumerate((5, 10, 20)):
            add(b * FP_NT + 1, J, K=1, force="panel", points=6, regime="dep" if (kp // 4 + bi) % 3 == 0 else None)
    # non-finite gradient component: the walk rejects the two pairs that touch the point; later fits read a hist_src with gaps
    add(300, 4, bad=(3, 5, float("nan")), regime="plain")      # fit:reg:8,2
    add(20, 10, bad=(3, 5, float("inf")), regime="plain")      # fit:gen:20
    return out


GRID = _grid()


def case_id(c):
    reg = next(nm for nm, v in REGIMES.items() if v == (c.cond, c.dep))
    return f"d{c.d}-J{c.J}-{reg}" + (f"-{c.force}" if c.force else "") + (f"-bad{c.bad[2]}" if c.bad else "")


def case_plan(c):
    return plan_for(c.d, c.J, c.force)


def family(plan):
    return plan.split(":")[1]


def oracle_walk(c):
    """the case's traces and the oracle's history walk of each: (thetas, grads, [(alpha_all, hist_len, hist_src, n_rejected)])"""
    th, gr = quad_history(c.d, c.lengths, c.cond, c.dep, c.seed, c.bad)
    return th, gr, [po.lbfgs_history(t, g, c.J) for t, g in zip(th, gr)]
