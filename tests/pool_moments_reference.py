"""Reference of pfmi_pool_moments for ONE run, in NumPy longdouble (a restatement of the four formulas of include/pfmi.h, including the
zero-weight skip), with the absolute sums A_p = sum |w^q (x - c)^p| the error bound of the GPU tests is stated in.  Not collected by
pytest."""
import numpy as np

LD = np.longdouble


def run_moments(X, w=None, center=None):
    """X (d, N) draws of one run, w (N,) weights or None (= 1, nothing skipped), center (d,) or None (= 0).
    Returns dict(s1, s2, s2w (d,), wsum (2,), A1, A2, A2w (d,), Aw (2,)) as longdouble."""
    X = np.asarray(X, dtype=np.float64)
    d, N = X.shape
    if w is None:
        wl = np.ones(N, dtype=LD)
        keep = np.ones(N, dtype=bool)
    else:
        w = np.asarray(w, dtype=np.float64)
        assert w.shape == (N,)
        keep = w != 0.0                       # a column of weight exactly 0 contributes nothing, whatever it holds
        wl = w.astype(LD)
    c = np.zeros(d, dtype=LD) if center is None else np.asarray(center, dtype=np.float64).astype(LD)
    T = X[:, keep].astype(LD) - c[:, None]
    wk = wl[keep]
    with np.errstate(invalid="ignore", over="ignore"):
        t1 = wk[None, :] * T
        t2 = t1 * T
        t2w = t1 * t1
        return dict(s1=t1.sum(axis=1), s2=t2.sum(axis=1), s2w=t2w.sum(axis=1), wsum=np.array([wk.sum(), (wk * wk).sum()], dtype=LD),
                    A1=np.abs(t1).sum(axis=1), A2=np.abs(t2).sum(axis=1), A2w=np.abs(t2w).sum(axis=1),
                    Aw=np.array([np.abs(wk).sum(), (wk * wk).sum()], dtype=LD))


def pool_moments(P, w=None, center=None):
    """P (d, N_r, K) pool, w (K * N_r,) weights of these runs in pool order or None: the per-run results stacked run-major,
    dict(s1, s2, s2w, A1, A2, A2w (K, d), wsum, Aw (K, 2))"""
    d, N_r, K = P.shape
    runs = [run_moments(P[:, :, k], None if w is None else w[k * N_r:(k + 1) * N_r], center) for k in range(K)]
    return {key: np.stack([r[key] for r in runs]) for key in runs[0]}


def bound(N_r, A):
    """|gpu - ref| <= (N_r + 4) 2^-53 A: any summation order of N_r fp64 terms is within (N_r - 1) u of the exact sum relative to the
    sum of absolute values, and three roundings (x - c, times w, times the second factor) form each term."""
    return (N_r + 4) * LD(2.0) ** -53 * A


def summary(P, w=None):
    """mean, var, ess, run_weights of the whole pool P (d, N_r, K) under weights w (K * N_r,) (None: uniform), two-pass, longdouble"""
    d, N_r, K = P.shape
    m1 = pool_moments(P, w, None)
    W = m1["wsum"][:, 0].sum()
    mean = m1["s1"].sum(axis=0) / W
    m2 = pool_moments(P, w, np.asarray(mean, dtype=np.float64))
    var = m2["s2"].sum(axis=0) / W - (m2["s1"].sum(axis=0) / W) ** 2
    return dict(mean=mean, var=var, ess=W * W / m1["wsum"][:, 1].sum(), run_weights=m1["wsum"][:, 0] / W,
                mcse_mean=np.sqrt(m2["s2w"].sum(axis=0)) / W)
