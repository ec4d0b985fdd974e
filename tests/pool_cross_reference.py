"""Reference of pfmi_pool_cross in NumPy longdouble (a restatement of the definition of include/pfmi.h, including the zero-weight skip and
the propagation of a NaN), with the absolute sums A[i][j] = |C_in| + sum |w t_i t_j| the error bound of the GPU tests is stated in.
Not collected by pytest."""
import numpy as np

LD = np.longdouble


def run_cross(X, w=None, center=None):
    """X (d, N) draws of one run, w (N,) weights or None (= 1, nothing skipped), center (d,) or None (= 0).
    Returns (C, A), (d, d) longdouble: C = sum_n (w t) t', A = sum_n |w t| |t|'."""
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
    with np.errstate(invalid="ignore", over="ignore"):
        WT = wl[keep][None, :] * T
        return WT @ T.T, np.abs(WT) @ np.abs(T).T


def pool_cross(P, w=None, center=None, carry=None):
    """P (d, N_r, K) pool, w (K * N_r,) weights of these runs in pool order or None, carry (d, d) or None: (C, A) of the pool, the
    runs added in run order on top of the carry"""
    d, N_r, K = P.shape
    C = np.zeros((d, d), dtype=LD) if carry is None else np.asarray(carry, dtype=np.float64).astype(LD)
    A = np.abs(C)
    for k in range(K):
        c, a = run_cross(P[:, :, k], None if w is None else w[k * N_r:(k + 1) * N_r], center)
        C, A = C + c, A + a
    return C, A


def bound(M, A):
    """|gpu - ref| <= (M + 4) 2^-53 A, M the number of added terms (K N_r, plus 1 with a carry): any order of M fp64 additions is
    within (M - 1) u of the exact sum relative to the sum of absolute values, and three roundings form a term (the two centrings and
    the weight; the product is exact inside the fused multiply-add)."""
    return (M + 4) * LD(2.0) ** -53 * A


def covariance(P, w=None):
    """two-pass weighted covariance of the whole pool P (d, N_r, K) under weights w (K * N_r,) (None: uniform), longdouble:
    dict(mean, cov, W, A) with A the absolute sums of the cross moments about the (float64-rounded) mean"""
    d, N_r, K = P.shape
    P2 = P.reshape(d, N_r * K, order="F")
    wl = np.ones(N_r * K, dtype=LD) if w is None else np.asarray(w, dtype=np.float64).astype(LD)
    keep = np.ones(N_r * K, dtype=bool) if w is None else np.asarray(w) != 0.0
    W = wl[keep].sum()
    mean = (wl[keep][None, :] * P2[:, keep].astype(LD)).sum(axis=1) / W
    m64 = np.asarray(mean, dtype=np.float64)
    C, A = pool_cross(P, w, m64)
    delta = (wl[keep][None, :] * (P2[:, keep].astype(LD) - m64.astype(LD)[:, None])).sum(axis=1) / W
    return dict(mean=mean, cov=C / W - np.outer(delta, delta), W=W, A=A, delta=delta)
