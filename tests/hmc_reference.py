"""Reference of the static-HMC step kernel (pathfinder.jl_amd/csrc/hmc_kernel.hip).  Not collected by pytest; used by
tests/test_gpu_hmc_steps.py / tests/test_gpu_hmc.py and pinned on the CPU by tests/test_hmc_reference_cpu.py.

Two things live here.

`mirror`   a float64 NumPy statement of the transition of include/pfmi.h (pfmi_hmc_enqueue), driven by a host logp_and_grad.  It
           returns exactly what the kernel records: per round the closure's input X, its output (lp, g) and the whitened momentum v
           after the round's launch; per transition x, lp, a, H1 - H0 and the divergent flag.  `fault=` injects one wrong step (the
           CPU test shows that the checker rejects each of them).

`check`    a np.longdouble checker of such a recording (the kernel's or the mirror's).  It is TEACHER-FORCED: for every recorded
           round it recomputes wt = R g, v and the next X in long double from the recording's own previous v, X and closure output,
           so errors do not accumulate along a trajectory.  At every trajectory end it recomputes H0, H1, a and the decision.

The metric is one fit's factor (s = sqrt(alpha), Householder vectors Vh (d x k, unit diagonal), the compact-WY T (k x k upper), the
Cholesky factor V (k x k upper); k = min(d, 2 j)):
    L v = s . (z - Vh T Vh'z),  z = [V'v_1; v_2]            (PFMI_OP_UNWHITEN)
    R g = [V y_1; y_2],  y = z - Vh T'Vh'z,  z = s . g       (PFMI_OP_RMUL)

Tolerances: |value - ref| <= C eps S with eps = 2^-52 (two unit roundoffs per counted step), S the same sums with every term replaced
by its absolute value, and C counted from the kernel's reduction map, never fitted to GPU output:
    C_apply = ceil(d / 256)   rows a thread accumulates into its partial of w = Vh'z (one fma per row)
            + 6               butterfly steps of the wave sum
            + 4               waves summed in wave order
            + 3 KPAD          the head transform with V, tv = T w (or T'w), and Vh[i, :] tv: three contractions of at most KPAD terms
            + 16              the roundings of the inputs (s . g, e s . y), the final multiply-adds and slack for the order of the last adds
  v   |v - v_ref| <= C_apply eps S_v,   S_v = |v_prev| + e S_R(|g|)      (e / 2 at a trajectory's ends; at an opening |z| + (e/2) S_wg)
  X   |X - X_ref| <= C_apply eps S_X,   S_X = |base| + e S_L(|v|)
  H   C_sum = ceil(d / 256) + 6 + 4 + 8 for the sums |v|^2 (no contraction):
      |dH - dH_ref| <= eps (C_sum (|lp0| + |z|^2 / 2) + C_sum (|lp1| + |vf|^2 / 2) + C_apply sum_i |vf_i| S_v,i) =: B_H
  a   |a - a_ref| <= a_ref (B_H + 8 eps (1 + |dH|)) + eps           (exp is correct to a few ulp of its argument's rounding)
A decision is BORDERLINE when |log u - (H0 - H1)| <= B_H + 8 eps (1 + |dH|) (or |dH - 1000| <= B_H for the divergence limit):
borderline decisions are exempt, no other is; `check` returns their number and the caller caps it (2 % of a case's transitions).
"""
import numpy as np

import scan_reference as sr
from helpers import oracle_factor_from_gpu

LD = sr.LD
EPS = sr.EPS64
ACCEPT_STREAM = 3                 # PF_RNG_STREAM_HMC_ACCEPT (pathfinder.jl_amd/csrc/pfmi_common.h)
DBL_MAX = float(np.finfo(np.float64).max)
KPADS = (4, 8, 12, 16, 20, 32, 64)
LDS_RES = 150 * 1024              # HM_LDS_RES: the factor rows are staged in LDS when d KPAD 8 B fit


def kpad_for(J):
    return next(o for o in KPADS if 2 * J <= o)


def resident(d, kpad):
    return d * kpad * 8 <= LDS_RES


def c_apply(d, kpad):
    return -(-d // 256) + 6 + 4 + 3 * kpad + 16


def c_sum(d):
    return -(-d // 256) + 6 + 4 + 8


class Metric:
    """one fit's factor in `dtype`; L, R and their absolute-value majorants"""

    def __init__(self, s, Vh, T, V, dtype=np.float64):
        self.dt = dtype
        self.s = np.asarray(s, dtype=dtype)
        self.d = len(self.s)
        self.Vh = np.asarray(Vh, dtype=dtype).reshape(self.d, -1)
        self.k = self.Vh.shape[1]
        k = self.k
        self.T = np.triu(np.asarray(T, dtype=dtype).reshape(k, k))
        self.V = np.triu(np.asarray(V, dtype=dtype).reshape(k, k))

    @classmethod
    def from_fit(cls, f, dtype=np.float64):
        """f: a pfmi_get_fit dictionary (Engine.get_fit)"""
        F = oracle_factor_from_gpu(f)
        Lf = sr.LDFactor(F, f["mu"])
        k = Lf.k
        T = np.asarray(f["T"], dtype=np.float64).reshape(k, k) if k else np.zeros((0, 0))
        return cls(Lf.s, Lf.Vh, T, Lf.V, dtype)

    def astype(self, dtype):
        return Metric(self.s, self.Vh, self.T, self.V, dtype)

    def L(self, v, fault=None):
        k = self.k
        z = np.array(v, dtype=self.dt)
        z[:k] = self.V.T @ z[:k]
        y = z - self.Vh @ (self.T @ (self.Vh.T @ z))
        return y if fault == "no_sqrt_alpha" else self.s * y

    def R(self, g, fault=None):
        k = self.k
        z = self.s * np.asarray(g, dtype=self.dt)
        Tt = self.T if fault == "T_for_Tt" else self.T.T
        y = z - self.Vh @ (Tt @ (self.Vh.T @ z))
        y[:k] = self.V @ y[:k]
        return y

    def L_abs(self, va):
        k = self.k
        z = np.array(va, dtype=self.dt)
        z[:k] = np.abs(self.V).T @ z[:k]
        return self.s * (z + np.abs(self.Vh) @ (np.abs(self.T) @ (np.abs(self.Vh).T @ z)))

    def R_abs(self, ga):
        k = self.k
        z = self.s * np.asarray(ga, dtype=self.dt)
        y = z + np.abs(self.Vh) @ (np.abs(self.T).T @ (np.abs(self.Vh).T @ z))
        y[:k] = np.abs(self.V) @ y[:k]
        return y


def random_metric(d, j, rng):
    """a synthetic factor of the fit's shape: k = min(d, 2 j) reflectors (dlarft's T), V upper with a positive diagonal, s > 0"""
    k = min(d, 2 * j)
    Vh = np.zeros((d, k))
    T = np.zeros((k, k))
    for c in range(k):
        Vh[c, c] = 1.0
        Vh[c + 1:, c] = rng.standard_normal(d - c - 1) * 0.5
        tau = 2.0 / (Vh[:, c] @ Vh[:, c])
        T[c, c] = tau
        if c:
            T[:c, c] = -tau * (T[:c, :c] @ (Vh[:, :c].T @ Vh[:, c]))
    V = np.triu(rng.standard_normal((k, k)) * 0.3)
    V[np.arange(k), np.arange(k)] = 0.5 + rng.random(k)
    return Metric(np.exp(0.3 * rng.standard_normal(d)), Vh, T, V)


def accept_uniform(seed, t):
    import pfmi
    r = int(np.asarray(pfmi.hostrng.rand_u64(int(seed), np.array([t], dtype=np.uint64), ACCEPT_STREAM))[0])
    return (r >> 11) * 2.0 ** -53


def momentum(seed, d, t):
    return sr.normals(int(seed), d, 0, [int(t) & 0xFFFFFFFF])[:, 0]


# ---- the float64 mirror ----------------------------------------------------------------------------------------------------------
def mirror(M, logp_and_grad, x0, seed, eps, Lf, T, fault=None, refresh=True):
    """T transitions of one chain from x0.  Returns a recording (see `check`)."""
    d = M.d
    x = np.array(x0, dtype=np.float64)
    rec = {"x0": x.copy(), "X": [], "lp": [], "g": [], "v": [], "draws": [], "logp": [], "accept_prob": [], "energy_error": [], "divergent": []}

    def evaluate(xt):
        with np.errstate(all="ignore"):
            l, g = logp_and_grad(xt)
        rec["X"].append(xt.copy()); rec["lp"].append(float(l)); rec["g"].append(np.array(g, dtype=np.float64))
        return float(l), np.asarray(g, dtype=np.float64)

    with np.errstate(all="ignore"):
        lp, g = evaluate(x)
        wg = M.R(g, fault)
        v = np.zeros(d)
        for t in range(T):
            if refresh or t == 0:
                v = momentum(seed, d, t + 1 if fault == "normals_t1" else t)
            H0 = -lp + 0.5 * float(v @ v)
            v = v + (-0.5 if fault == "half_sign" else 0.5) * eps * wg
            xt = x + eps * M.L(v, fault)
            rec["v"].append(v.copy())
            bad = False
            for i in range(1, Lf + 1):
                lpt, gt = evaluate(xt)
                wt = M.R(gt, fault)
                bad = bad or not (np.isfinite(lpt) and np.all(np.isfinite(gt)))
                if i < Lf:
                    v = v + eps * wt
                    xt = xt + eps * M.L(v, fault)
                    rec["v"].append(v.copy())
                else:
                    v = v + (1.0 if fault == "full_kick_end" else 0.5) * eps * wt
            H1 = -lpt + 0.5 * float(v @ v)
            dH = H1 - H0
            div = bad or not np.isfinite(H1) or dH > 1000.0
            a = 0.0 if div else min(1.0, float(np.exp(-dH)))
            u = accept_uniform(seed, t + 1 if fault == "uniform_counter" else t)
            if u < a:
                x, lp, wg = xt.copy(), lpt, wt
            rec["draws"].append(x.copy()); rec["logp"].append(lp); rec["accept_prob"].append(a)
            rec["energy_error"].append(dH if np.isfinite(dH) else DBL_MAX); rec["divergent"].append(int(div))
        rec["v"].append(v.copy())                           # (the last round's v is not looked at)
    for k_ in ("X", "g", "v", "draws"):
        rec[k_] = np.array(rec[k_])
    for k_ in ("lp", "logp", "accept_prob", "energy_error"):
        rec[k_] = np.array(rec[k_], dtype=np.float64)
    rec["divergent"] = np.array(rec["divergent"], dtype=np.int32)
    return rec


def gpu_recording(x0, path, got, k):
    """chain k's recording from Engine.hmc_path() and Engine.hmc_get()"""
    X, lp, g, v = path
    return {"x0": np.asarray(x0, dtype=np.float64), "X": X[:, k, :].T, "lp": lp[k], "g": g[:, k, :].T, "v": v[:, k, :].T,
            "draws": got["draws"][:, :, k].T, "logp": got["logp"][k], "accept_prob": got["accept_prob"][k],
            "energy_error": got["energy_error"][k], "divergent": got["divergent"][k]}


# ---- the long-double checker -------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def check(M, rec, seed, eps, Lf, kpad, label=""):
    """teacher-forced long-double check of a recording of T transitions (1 + T Lf rounds) that started at transition 0.
    Returns {"borderline", "accepted", "rejected", "margins": {quantity: max err / bound}}; raises Mismatch."""
    ML = M.astype(LD)
    d = M.d
    T = len(rec["logp"])
    assert len(rec["lp"]) == 1 + T * Lf, (len(rec["lp"]), T, Lf)
    Ca, Cs = c_apply(d, kpad), c_sum(d)
    e = LD(eps)
    marg = {"v": 0.0, "X": 0.0, "dH": 0.0, "a": 0.0}
    out = {"borderline": 0, "accepted": 0, "rejected": 0, "divergent": 0, "margins": marg}

    def need(cond, *what):
        if not cond:
            raise Mismatch((label,) + what)

    def close(q, val, ref, S, C, *what):
        err = np.abs(np.asarray(val, dtype=LD) - ref)
        bound = C * EPS * np.asarray(S, dtype=LD)
        with np.errstate(all="ignore"):
            m = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
        marg[q] = max(marg[q], m)
        need(m <= 1.0, q, m) if not what else need(m <= 1.0, q, m, *what)

    Xr, gr, vr, lpr = rec["X"], rec["g"], rec["v"], rec["lp"]
    need(np.array_equal(Xr[0], rec["x0"]), "round 0 did not evaluate x0")
    x = np.asarray(rec["x0"], dtype=np.float64)
    lp = float(lpr[0])
    need(np.isfinite(lp) and np.all(np.isfinite(gr[0])), "non-finite start")
    wg, Swg = ML.R(gr[0]), ML.R_abs(np.abs(gr[0]))
    for t in range(T):
        # ---- the opening: fresh momentum, first half kick, first drift (recorded in round t Lf)
        r0 = t * Lf
        z = np.asarray(momentum(seed, d, t), dtype=LD)
        H0 = -LD(lp) + np.sum(z * z) / 2
        S_H0 = abs(LD(lp)) + np.sum(z * z) / 2
        close("v", vr[r0], z + e / 2 * wg, np.abs(z) + e / 2 * Swg, Ca, "opening", t)
        v = np.asarray(vr[r0], dtype=LD)
        close("X", Xr[r0 + 1], np.asarray(x, dtype=LD) + e * ML.L(v), np.abs(x) + e * ML.L_abs(np.abs(v)), Ca, "opening", t)
        bad = False
        for i in range(1, Lf + 1):
            r = r0 + i
            g, lpt = gr[r], float(lpr[r])
            bad = bad or not (np.isfinite(lpt) and np.all(np.isfinite(g)) and np.all(np.isfinite(vr[r - 1])))
            if bad:
                continue
            wt, Swt = ML.R(g), ML.R_abs(np.abs(g))
            vp = np.asarray(vr[r - 1], dtype=LD)
            if i < Lf:
                close("v", vr[r], vp + e * wt, np.abs(vp) + e * Swt, Ca, "round", r)
                v = np.asarray(vr[r], dtype=LD)
                if np.all(np.isfinite(vr[r])):
                    close("X", Xr[r + 1], np.asarray(Xr[r], dtype=LD) + e * ML.L(v), np.abs(Xr[r]) + e * ML.L_abs(np.abs(v)), Ca, "round", r)
        r = r0 + Lf
        trial = Xr[r]
        took = bool(np.array_equal(rec["draws"][t], trial))
        need(took or np.array_equal(rec["draws"][t], x), "row is neither the trial nor the state", t)
        a_k, de_k, div_k = float(rec["accept_prob"][t]), float(rec["energy_error"][t]), int(rec["divergent"][t])
        need(np.isfinite(a_k) and np.isfinite(de_k), "non-finite record", t)
        exempt = False
        if bad:
            need(div_k == 1 and a_k == 0.0 and not took, "a non-finite trajectory must be divergent and rejected", t)
            accept = False
        else:
            vf = vp + e / 2 * wt
            Svf = np.abs(vp) + e / 2 * Swt
            H1 = -LD(lpt) + np.sum(vf * vf) / 2
            dH = H1 - H0
            B_H = EPS * (Cs * S_H0 + Cs * (abs(LD(lpt)) + np.sum(vf * vf) / 2) + Ca * np.sum(np.abs(vf) * Svf))
            if not np.isfinite(float(dH)):
                need(div_k == 1 and a_k == 0.0 and not took, "a non-finite energy must be divergent and rejected", t)
                accept = False
            else:
                close("dH", de_k, dH, B_H / EPS, 1.0, "transition", t)
                B_dec = float(B_H + 8 * EPS * (1 + abs(dH)))
                div = bool(dH > 1000)
                if abs(float(dH) - 1000.0) <= float(B_H):
                    exempt = True
                a_ref = LD(0) if div else min(LD(1), np.exp(-dH))
                u = accept_uniform(seed, t)
                accept = bool(u < a_ref)
                if not div and u > 0 and abs(float(np.log(LD(u)) + dH)) <= B_dec:
                    exempt = True
                if not exempt:
                    need(div_k == int(div), "divergent flag", t, float(dH))
                    close("a", a_k, a_ref, a_ref * (B_dec / EPS) + 1, 1.0, "transition", t)
                    need(took == accept, "decision", t, float(u), float(a_ref))
                else:
                    out["borderline"] += 1
                    accept = took
        need(took == accept or exempt, "decision", t)
        out["divergent"] += div_k
        if took:
            x, lp = np.asarray(trial, dtype=np.float64), lpt
            wg, Swg = wt, Swt
            out["accepted"] += 1
        else:
            out["rejected"] += 1
        need(float(rec["logp"][t]) == lp, "recorded logp is not the state's", t)
    return out


# ---- the grid of tests/test_gpu_hmc_steps.py (shapes, targets, seeds, step sizes; the CPU test runs the same cases on the mirror) ----
GRID_T, GRID_LF, GRID_K = 4, 3, 3
# d x J in {2, 6, 16, 32} (KPAD 4, 12, 32, 64); the paddings in between (J = 4, 8, 10: KPAD 8, 16, 20) at d = 64, and KPAD 20 at d = 5 < KPAD
GRID_MID = [(64, 4), (64, 8), (64, 10), (5, 10)]
GRID = ([(d, J, tn, GRID_T) for d in (5, 64, 257, 1000) for J in (2, 6, 16, 32) for tn in ("gauss", "funnel")]
        + [(d, J, tn, GRID_T) for d, J in GRID_MID for tn in ("gauss", "funnel")] + [(20000, 6, "gauss", 2)])
EPS_MULT = (0.4, 1.0, 2.2)        # per chain, times d^(-1/4): a small step accepts, a large one rejects


def case_id(case):
    return "%s-d%d-J%d" % (case[2], case[0], case[1])


def grid_target(pfmi, tn, d):
    """the Gaussian rank-2 target at a scale a history of a few pairs represents, or the funnel"""
    return pfmi.t_funnel(d) if tn == "funnel" else pfmi.t_lowrank(d, r=2, seed=2, wscale=2.0 / np.sqrt(d))


def grid_path_x0(pfmi, tn, d):
    u = pfmi.HostRNG(100 + d).rand(d)
    return (u * 2 - 1)[None, :] if tn == "funnel" else (u * 4 - 2)[None, :]


def grid_eps(d):
    return np.array(EPS_MULT) * d ** -0.25


def grid_seeds(d, J):
    import pfmi
    return np.asarray(pfmi.hostrng.rand_u64(9000 + 7 * d + J, np.arange(GRID_K, dtype=np.uint64), 9), dtype=np.uint64)


# ---- the energy-order and sampling cases of tests/test_gpu_hmc.py (run on the mirror by tests/test_hmc_reference_cpu.py) -------------
# Both use the fit of a path's FIRST point as the metric: j_eff = 0, Sigma = diag(alpha) with alpha = 1 -- the identity, which the
# CPU can state without a GPU fit (the GPU tests assert that the fit they use is exactly that).
ENERGY_RUNS = ((0.1, 4), (0.05, 8))         # (step size, leapfrog steps): the same trajectory length
ENERGY_RATIO = (3.5, 4.5)                   # second-order integrator: max |H1 - H0| scales by 4 + O(e^2)
ENERGY_K = 16
SAMPLING_K, SAMPLING_T, SAMPLING_LF, SAMPLING_EPS = 256, 60, 4, 0.3


def identity_metric(d):
    return Metric(np.ones(d), np.zeros((d, 0)), np.zeros((0, 0)), np.zeros((0, 0)))


def target_cov(tg):
    W = tg.Wd / tg.a[:, None]
    return np.diag(1.0 / tg.a) + W @ W.T


def energy_case(pfmi):
    """(target, metric, x0 (d, K) drawn from the target, seeds): one transition per chain, so both runs see the same starts and momenta"""
    d = 64
    tg = pfmi.t_lowrank(d, r=2, seed=2, wscale=2.0 / np.sqrt(d))
    Lc = np.linalg.cholesky(target_cov(tg))
    x0 = np.asfortranarray(tg.mean[:, None] + Lc @ np.random.default_rng(11).standard_normal((d, ENERGY_K)))
    seeds = np.asarray(pfmi.hostrng.rand_u64(4242, np.arange(ENERGY_K, dtype=np.uint64), 9), dtype=np.uint64)
    return tg, identity_metric(d), x0, seeds


def sampling_case(pfmi):
    """(target, metric, x0 (d,): 3 standard deviations off the mean in every coordinate, seeds, Cholesky factor of the true covariance)"""
    tg = pfmi.t_lowrank(8, r=2)
    cov = target_cov(tg)
    x0 = tg.mean + 3.0 * np.sqrt(np.diag(cov))
    seeds = np.asarray(pfmi.hostrng.rand_u64(777, np.arange(SAMPLING_K, dtype=np.uint64), 9), dtype=np.uint64)
    return tg, identity_metric(8), x0, seeds, np.linalg.cholesky(cov)


def sampling_stats(tg, Lc, fin):
    """coordinate means and variances of the final states fin (d, n) whitened with the target's true covariance"""
    z = np.linalg.solve(Lc, fin - tg.mean[:, None])
    return z.mean(axis=1), z.var(axis=1, ddof=1)


def sampling_ok(mean, var, n=SAMPLING_K):
    """sampling-distribution bounds: 5 standard errors of a mean of n unit normals, and of their sample variance"""
    return bool(np.all(np.abs(mean) <= 5.0 / np.sqrt(n)) and np.all(np.abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / (n - 1))))
