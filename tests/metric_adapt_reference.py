"""Reference of the windowed metric adaptation of the device warm-up (pathfinder.jl_amd/csrc/adapt.h, hmc_rows.h: hm_whiten, hm_metric_end;
include/pfmi.h: pfmi_chain_scale_set, pfmi_hmc_adapt_metric_enqueue, pfmi_nuts_adapt_metric_enqueue).  Not collected by pytest; used by
tests/test_metric_adapt_cpu.py and tests/test_gpu_metric_adapt.py.

`windows`        the window rule of include/pfmi.h restated in Python.
`whiten_ld`      u = L \\ dx in np.longdouble on hmc_reference.Metric; `whiten_np` the float64 NumPy statement; `whiten_bound` what a float64
                 implementation may deviate from whiten_ld.
`scale_ld`       Welford and the regularised variance of a window's rows in long double; `scale_np` the NumPy statement (np.var);
                 `scale_bound` the bound on the scale.
`ScaledMetric`   Metric with a per-coordinate scale: L(v) = M.L(c v), R(g) = c M.R(g), and the matching majorants; hmc_reference.check and
                 nuts_reference.check take it where they take a Metric.
`mirror`         adapt_reference.mirror with the windows: a float64 statement of static HMC whose warm-up adapts step size and scale.
`check_run`      the teacher-forced checker of such a run, the device's or the mirror's: whitened rows, every window's scale, every
                 step-size segment between restarts.

Tolerances follow the project's rule (tests/adapt_reference.py, profiles/chain_diag_parity.md): a float64 value may deviate from the
long-double reference by the larger of 8 x the deviation of the float64 NumPy statement on the same input and a floor counted from the
operations.  u = 2^-53; EPS = 2^-52 = 2 u as in hmc_reference.  Nothing is fitted to the code under test.

The whiten pass.  z = dx / s (one rounding more than the s . g of the R pass, which C_apply's 16 already counts), w = Vh'z, tv = T'w,
y = z - Vh tv: the reduction map of the R pass, so with S_y = z + |Vh| |T'| |Vh'| z (z = |dx| / s) every y_i is within
C_apply EPS S_y,i (hmc_reference.c_apply).  Tail rows are done.  Head rows solve V'u = y_head by forward substitution in the order the
kernel states (hm_whiten: u_a = (..(y_a - V[0][a] u_0) - .. - V[a-1][a] u_{a-1}) / V[a][a], one fma per term, one division): by Higham,
Accuracy and Stability of Numerical Algorithms, Theorem 8.5, the computed u solves (V' + dV) u = y^ with |dV| <= gamma_k |V'|, k the
operations of a row (at most KPAD fmas and the division), so
    |u^ - u| <= |V'^-1| (C_apply EPS S_y,head) + (KPAD + 2) u |V'^-1| |V'| |u^|
(the first term: the error y_head already has, carried through the solve; (KPAD + 2) u covers gamma_{KPAD + 1} for every KPAD <= 64).

Welford and the regularisation, n rows of one coordinate, a = max |u_t|.  One update is dl = u - mean, mean += dl / n, M2 = fma(dl, u - mean,
M2): five roundings.  The running mean: each update adds at most 3 u a and damps what is there, so |mean^ - mean| <= E = 4 n u a at
every t.  A term of M2 is (u_t - mean_{t-1}) (u_t - mean_t) >= 0, so M2 is a sum without cancellation: its factors carry E each, the
product and the n accumulations (n + 3) u of the sum:
    |M2^ - M2| <= E A1 + n E^2 + (n + 4) u M2,      A1 = sum_{t >= 2} |u_t - mean_{t-1}| + |u_t - mean_t|
(the first update is exact: mean_1 = u_1 and its term is u_1 times an exact 0)
D = fma(n / (n + 5), M2 / (n - 1), 5 / (n + 5)) takes four roundings and the square root one:
    |D^ - D| <= n / ((n + 5) (n - 1)) |M2^ - M2| + 4 u D,        |c^ - c| <= |D^ - D| / (2 sqrt(D)) + u c
A column with mean 1e8 and unit spread: E A1 is 1e-5 of M2 -- loose, but the sum-of-squares formula misses it by ten orders."""
import numpy as np

import adapt_reference as A
import hmc_reference as H

LD = H.LD
U = 2.0 ** -53
SHRINK = 5.0
NO_METRIC_WINDOW, KEPT_METRIC, RECORD_WHITENED = 2, 4, 4          # PFMI_ADAPT_*
MIN_WINDOWED = 20


# ---- the window rule -----------------------------------------------------------------------------------------------------------------
def windows(W):
    """(init, term, ends): the first window's start, the transitions after the last window, the exclusive ends; no window below 20"""
    if W < MIN_WINDOWED:
        return W, 0, []
    init, term, base = 75, 50, 25
    if init + base + term > W:
        init, term = (15 * W) // 100, (10 * W) // 100
        base = W - init - term
    end = W - term
    ends, e, s = [], init, base
    while e < end:
        e = end if e + s + 2 * s - 1 >= end else e + s
        ends.append(e)
        s *= 2
    return init, term, ends


TABLE = {20: [18], 100: [90], 150: [100], 151: [101], 200: [100, 150], 201: [100, 151], 300: [100, 150, 250], 1000: [100, 150, 250, 450, 950]}


# ---- the whiten pass -----------------------------------------------------------------------------------------------------------------
def _forward(Vt, y):
    """V'u = y by forward substitution in the dtype of the arguments (Vt = V' lower triangular)"""
    u = np.array(y)
    for a in range(len(u)):
        u[a] = (u[a] - Vt[a, :a] @ u[:a]) / Vt[a, a]
    return u


def whiten(M, dx):
    """u = L \\ dx in M's dtype: z = dx / s, y = z - Vh T'Vh'z, head <- V'^-1 head"""
    k = M.k
    z = np.asarray(dx, dtype=M.dt) / M.s
    y = z - M.Vh @ (M.T.T @ (M.Vh.T @ z))
    y[:k] = _forward(M.V.T, y[:k])
    return y


def whiten_ld(M, dx):
    return whiten(M.astype(LD), np.asarray(dx, dtype=LD))


def whiten_np(M, dx):
    return whiten(M.astype(np.float64), np.asarray(dx, dtype=np.float64))


def whiten_floor(M, dx, u_val, kpad):
    """the floor of the docstring, per coordinate, around the computed u_val"""
    ML = M.astype(LD)
    k, d = M.k, M.d
    z = np.abs(np.asarray(dx, dtype=LD)) / ML.s
    Sy = z + np.abs(ML.Vh) @ (np.abs(ML.T).T @ (np.abs(ML.Vh).T @ z))
    fl = H.c_apply(d, kpad) * H.EPS * Sy
    if k:
        Vi = np.abs(np.linalg.inv(np.asarray(ML.V.T, dtype=np.float64))).astype(LD)          # |V'^-1| (its own rounding is far inside the factor 8)
        fl[:k] = Vi @ fl[:k] * (1 + 1e-10) + (kpad + 2) * U * (Vi @ (np.abs(ML.V.T) @ np.abs(np.asarray(u_val[:k], dtype=LD))))
    return fl


def whiten_ratio(M, dx, u_val, kpad):
    """max over coordinates of |u_val - whiten_ld| / bound, bound = max(8 |whiten_np - whiten_ld|, floor)"""
    ref = whiten_ld(M, dx)
    dev = np.abs(np.asarray(whiten_np(M, dx), dtype=LD) - ref)
    bound = np.maximum(8 * dev, whiten_floor(M, dx, u_val, kpad))
    err = np.abs(np.asarray(u_val, dtype=LD) - ref)
    with np.errstate(all="ignore"):
        return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))


# ---- Welford and the regularised variance -----------------------------------------------------------------------------------------------
def scale_ld(u, target=1.0, ddof=1):
    """(c, D, M2, A1) per column of the rows u (n, d) in long double; c = sqrt(D) (NaN where D is not positive and finite)"""
    u = np.asarray(u, dtype=LD)
    n, d = u.shape
    mean, m2, a1 = np.zeros(d, dtype=LD), np.zeros(d, dtype=LD), np.zeros(d, dtype=LD)
    with np.errstate(all="ignore"):
        for t in range(n):
            dl = u[t] - mean
            mean = mean + dl / LD(t + 1)
            m2 = m2 + dl * (u[t] - mean)
            if t:
                a1 = a1 + np.abs(dl) + np.abs(u[t] - mean)
        D = (LD(n) / LD(n + SHRINK)) * m2 / LD(n - ddof) + LD(target) * LD(SHRINK) / LD(n + SHRINK)
        c = np.sqrt(D)
    return c, D, m2, a1


def scale_np(u):
    """the float64 NumPy statement: D = n / (n + 5) var(u, ddof = 1) + 5 / (n + 5)"""
    u = np.asarray(u, dtype=np.float64)
    n = u.shape[0]
    with np.errstate(all="ignore"):
        return np.sqrt(n / (n + SHRINK) * np.var(u, axis=0, ddof=1) + SHRINK / (n + SHRINK))


def scale_ok(D):
    D = np.asarray(D, dtype=np.float64)
    return bool(np.all(np.isfinite(D)) and np.all(D > 0))


def scale_floor(u):
    """the floor of the docstring on c, per column"""
    u = np.asarray(u, dtype=LD)
    n = u.shape[0]
    c, D, m2, a1 = scale_ld(u)
    E = 4 * n * U * np.max(np.abs(u), axis=0)
    dm2 = E * a1 + n * E * E + (n + 4) * U * m2
    dD = LD(n) / (LD(n + SHRINK) * LD(n - 1)) * dm2 + 4 * U * D
    return dD / (2 * np.sqrt(D)) + U * c


def scale_ratio(u, c_val):
    """max over columns of |c_val - scale_ld| / bound, bound = max(8 |scale_np - scale_ld|, floor)"""
    ref = scale_ld(u)[0]
    dev = np.abs(np.asarray(scale_np(u), dtype=LD) - ref)
    bound = np.maximum(8 * dev, scale_floor(u))
    return float(np.max(np.abs(np.asarray(c_val, dtype=LD) - ref) / bound))


def host_metric_update(lib, u, scale_in, rc=False):
    """pfmi_host_metric_update: (scale_out, status) (rc=True: only the return code)"""
    import ctypes as C
    u = np.ascontiguousarray(u, dtype=np.float64)
    n, d = u.shape
    cin = np.ascontiguousarray(scale_in, dtype=np.float64)
    out, st = np.full(d, np.nan), C.c_int32(-1)
    dp = C.POINTER(C.c_double)
    code = lib.pfmi_host_metric_update(C.c_int64(n), C.c_int32(d), u.ctypes.data_as(dp), cin.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(st))
    if rc:
        return code
    assert code == 0, code
    return out, st.value


def host_windows(lib, W, cap=32):
    """pfmi_adapt_windows: (rc, init, term, ends)"""
    import ctypes as C
    init, term, n = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    ends = np.zeros(max(cap, 1), dtype=np.int64)
    rc = lib.pfmi_adapt_windows(C.c_int64(W), C.byref(init), C.byref(term), ends.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int32(cap), C.byref(n))
    return rc, init.value, term.value, ends[:max(n.value, 0)].tolist()


# ---- the scaled metric --------------------------------------------------------------------------------------------------------------
class ScaledMetric:
    """Sigma = L diag(c)^2 L' on a Metric M: L(v) = M.L(c v), R(g) = c M.R(g).  The scale costs one rounding per pass, relative to a term
    the majorants below already hold (c |.|); hmc_reference.c_apply counts 16 for the roundings of the inputs and the final multiply-adds
    -- four -- and slack, and one step of the checkers is EPS = 2 u, so the existing constant has room for it and stays as it is.
    fault="output_side": the scale on the other side of each operator (the CPU test shows that the checkers reject it)."""

    def __init__(self, M, c, fault=None):
        self.M, self.dt, self.d, self.k, self.fault = M, M.dt, M.d, M.k, fault
        self.c = np.asarray(c, dtype=M.dt)

    def astype(self, dtype):
        return ScaledMetric(self.M.astype(dtype), self.c, self.fault)

    def L(self, v, fault=None):
        if self.fault == "output_side":
            return self.c * self.M.L(np.asarray(v, dtype=self.dt))
        return self.M.L(self.c * np.asarray(v, dtype=self.dt))

    def R(self, g, fault=None):
        if self.fault == "output_side":
            return self.M.R(self.c * np.asarray(g, dtype=self.dt))
        return self.c * self.M.R(g)

    def L_abs(self, va):
        return self.M.L_abs(self.c * np.asarray(va, dtype=self.dt))

    def R_abs(self, ga):
        return self.c * self.M.R_abs(ga)


# ---- the float64 mirror: adapt_reference.mirror with the windows ------------------------------------------------------------------------
FAULTS = ("target_1e-3", "m2_over_n", "no_restart", "whiten_Lk")     # (the fifth, the scale on the output side of L, is ScaledMetric's)


def mirror(M, logp_and_grad, x0, seed, eps0, Lf, W, T, delta=0.8, c0=None, fault=None):
    """adapt_reference.mirror whose warm-up also adapts the scale in windows.  Returns its dictionary and "window_ends", "scale_trace"
    (nwin, d), "whitened" (rows of the window transitions), "states" (W, d) the state after every warm-up transition, "scale" (d,)."""
    from pfmi.hmc import dual_averaging_init, dual_averaging_update
    d = M.d
    init, _, ends = windows(W)
    c = np.ones(d) if c0 is None else np.array(c0, dtype=np.float64)
    x0 = np.array(x0, dtype=np.float64)
    x = x0.copy()
    out = {k: [] for k in ("draws", "logp", "accept_prob", "divergent", "eps_trace", "accept_trace", "warm_divergent", "scale_trace", "whitened",
                           "states")}
    st = dual_averaging_init(np.float64(eps0))
    eps, status = float(eps0), (0 if ends else NO_METRIC_WINDOW)
    win, rows = 0, []
    with np.errstate(all="ignore"):
        lp, g = logp_and_grad(x)
        lp = float(lp)
        wg = M.R(np.asarray(g, dtype=np.float64))
        for t in range(W + T):
            v = H.momentum(seed, d, t)
            H0 = -lp + 0.5 * float(v @ v)
            v = v + 0.5 * eps * (c * wg)
            xt = x + eps * M.L(c * v)
            bad = False
            for i in range(1, Lf + 1):
                lpt, gt = logp_and_grad(xt)
                lpt, gt = float(lpt), np.asarray(gt, dtype=np.float64)
                wt = M.R(gt)
                bad = bad or not (np.isfinite(lpt) and np.all(np.isfinite(gt)))
                if i < Lf:
                    v = v + eps * (c * wt)
                    xt = xt + eps * M.L(c * v)
                else:
                    v = v + 0.5 * eps * (c * wt)
            H1 = -lpt + 0.5 * float(v @ v)
            dH = H1 - H0
            div = bad or not np.isfinite(H1) or dH > 1000.0
            a = 0.0 if div else min(1.0, float(np.exp(-dH)))
            if H.accept_uniform(seed, t) < a:
                x, lp, wg = xt.copy(), lpt, wt
            if t < W:
                out["eps_trace"].append(eps); out["accept_trace"].append(a); out["warm_divergent"].append(int(div)); out["states"].append(x.copy())
                st, e1, ebar = dual_averaging_update(st, a, delta)
                cand = float(e1) if t + 1 < W else float(ebar)
                if cand > 0.0 and np.isfinite(cand):
                    eps = cand
                else:
                    status |= A.KEPT_STEP
                if win < len(ends) and t >= (init if win == 0 else ends[win - 1]):
                    u = whiten_np(M, x - x0)
                    if fault == "whiten_Lk":
                        u = u / c
                    rows.append(u); out["whitened"].append(u)
                    if t + 1 == ends[win]:
                        R = np.array(rows)
                        n = len(rows)
                        mean, m2 = np.zeros(d), np.zeros(d)
                        for q in range(n):
                            dl = R[q] - mean
                            mean = mean + dl / (q + 1.0)
                            m2 = m2 + dl * (R[q] - mean)
                        D = n / (n + SHRINK) * (m2 / (n if fault == "m2_over_n" else n - 1.0)) + (1e-3 if fault == "target_1e-3" else 1.0) * SHRINK / (n + SHRINK)
                        if scale_ok(D):
                            c = np.sqrt(D)
                        else:
                            status |= KEPT_METRIC
                        out["scale_trace"].append(c.copy())
                        if fault != "no_restart":
                            st = dual_averaging_init(np.float64(eps))
                        win, rows = win + 1, []
            else:
                out["draws"].append(x.copy()); out["logp"].append(lp); out["accept_prob"].append(a); out["divergent"].append(int(div))
    res = {k: np.array(v) for k, v in out.items()}
    res["step_size"], res["status"], res["window_ends"], res["scale"] = eps, status, np.array(ends, dtype=np.int64), c
    return res


# ---- the checker of a run's adaptation (teacher-forced) -----------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def check_run(M, kpad, x0, W, delta, run, c0=None):
    """`run`: "states" (W, d) the state after every warm-up transition (the device's: from its replay), "whitened" (nwt, d), "scale_trace"
    (nwin, d), "eps_trace", "accept_trace" (W,), "step_size".  Checks every whitened row against the long-double whiten of
    states[t] - x0, every window's scale against the long-double update of the RECORDED rows, and every step-size segment between restarts
    against adapt_reference.bound with the restart's step size as eps0.  Returns {"whiten", "scale", "eps"}: the largest error / bound
    of each; raises Mismatch beyond 1."""
    init, _, ends = windows(W)
    marg = {"whiten": 0.0, "scale": 0.0, "eps": 0.0}

    def need(q, r, *what):
        marg[q] = max(marg[q], r)
        if not r <= 1.0:
            raise Mismatch((q, r) + what)

    x0 = np.asarray(x0, dtype=np.float64)
    if len(np.asarray(run["scale_trace"])) != len(ends):
        raise Mismatch(("windows", len(run["scale_trace"]), len(ends)))
    c = np.ones(M.d) if c0 is None else np.asarray(c0, dtype=np.float64)
    for j, e in enumerate(ends):
        b = init if j == 0 else ends[j - 1]
        rows = np.asarray(run["whitened"])[b - init:e - init]
        for t in range(b, e):
            need("whiten", whiten_ratio(M, np.asarray(run["states"][t], dtype=np.float64) - x0, rows[t - b], kpad), "transition", t)
        D = scale_ld(rows)[1]
        if scale_ok(D):
            need("scale", scale_ratio(rows, run["scale_trace"][j]), "window", j)
            c = np.asarray(run["scale_trace"][j], dtype=np.float64)
        elif not np.array_equal(run["scale_trace"][j], c):
            raise Mismatch(("a window without a positive finite variance must keep the scale", j))
    eps_t, acc_t = np.asarray(run["eps_trace"], dtype=np.float64), np.asarray(run["accept_trace"], dtype=np.float64)
    cuts = [0] + list(ends) + [W]
    for b, e in zip(cuts[:-1], cuts[1:]):
        if e == b:
            continue
        be, bb, re, rb = A.bound(eps_t[b], delta, acc_t[b:e])
        n = e - b
        vals = [eps_t[b + m] for m in range(1, n)] + ([eps_t[e]] if e < W else [])
        for m, val in enumerate(vals, start=1):
            need("eps", abs(float(LD(val) / re[m] - 1)) / be[m - 1], "segment", b, "update", m)
        if e == W:
            need("eps", abs(float(LD(run["step_size"]) / rb[n - 1] - 1)) / bb[n - 1], "final step size")
    return marg


# ---- the cases of tests/test_gpu_metric_adapt.py ------------------------------------------------------------------------------------------
# (d, J, target, W, T): two windows (the doubling and both restarts) where a transition is cheap, one window on the shapes where one thread
# owns two rows and on the streamed route
CASES = [(5, 2, tn, 200, 4) for tn in ("gauss", "funnel")] + [(64, 6, tn, 200, 4) for tn in ("gauss", "funnel")] + \
        [(257, 16, tn, 20, 2) for tn in ("gauss", "funnel")] + [(20000, 6, "gauss", 20, 2)]
LF, DEPTH = 3, 4                  # as adapt_reference.BIT_LF, BIT_DEPTH


def case_id(case):
    return "%s-d%d-J%d" % (case[2], case[0], case[1])
