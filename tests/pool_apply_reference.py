"""Reference of pfmi_pool_apply in NumPy longdouble (a restatement of the two definitions of include/pfmi.h, including the zero-weight skip
and the propagation of a NaN), with the absolute sums the error bounds of the GPU tests are stated in: A_z[n][j] = sum_i |t_i v_ji| for
the scores and A_Y[j][i] = |y_in| + sum |w t_i z_j| for the apply.  Not collected by pytest."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53


def _columns(P):
    """the pool (d, N_r, K) as its flat list of columns (d, K N_r), run k at columns [k N_r, (k + 1) N_r)"""
    d, N_r, K = P.shape
    return np.asarray(P, dtype=np.float64).reshape(d, N_r * K, order="F")


def _centred(P, w, center):
    """(T (d, S) longdouble: x - center, keep (S,): which columns count, wl (S,) longdouble weights)"""
    X = _columns(P)
    d, S = X.shape
    if w is None:
        keep, wl = np.ones(S, dtype=bool), np.ones(S, dtype=LD)
    else:
        w = np.asarray(w, dtype=np.float64)
        assert w.shape == (S,)
        keep, wl = w != 0.0, w.astype(LD)            # a column of weight exactly 0 contributes nothing, whatever it holds
    c = np.zeros(d, dtype=LD) if center is None else np.asarray(center, dtype=np.float64).astype(LD)
    return X.astype(LD) - c[:, None], keep, wl


def pool_scores(P, w, center, V):
    """P (d, N_r, K) pool, w (K N_r,) weights in pool order or None (= 1, nothing skipped), center (d,) or None (= 0), V (r, d).
    Returns (Z, A_z), (K N_r, r) longdouble: Z[n][j] = sum_i t_i(n) V[j][i], exactly 0 in a skipped column, and A_z = sum_i |t_i V[j][i]|."""
    T, keep, _ = _centred(P, w, center)
    Vl = np.asarray(V, dtype=np.float64).astype(LD)
    S, r = T.shape[1], Vl.shape[0]
    Z, A = np.zeros((S, r), dtype=LD), np.zeros((S, r), dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        Z[keep] = T[:, keep].T @ Vl.T
        A[keep] = np.abs(T[:, keep]).T @ np.abs(Vl).T
    return Z, A


def pool_apply(P, w, center, Z, y_in=None, rows=None):
    """Y[j][i] = y_in[j][i] + sum_n (w t_i(n)) Z[n][j] over the counted columns, with the scores Z (K N_r, r) GIVEN (the device's, or
    pool_scores'): (Y, A_Y), (r, d) longdouble, A_Y = |y_in| + sum_n |w t_i Z[n][j]|.  rows: only these coordinates (columns of Y)."""
    T, keep, wl = _centred(P, w, center)
    if rows is not None:
        T = T[rows]
    Zl = np.asarray(Z).astype(LD)
    r = Zl.shape[1]
    Y = np.zeros((r, T.shape[0]), dtype=LD) if y_in is None else np.asarray(y_in, dtype=np.float64).astype(LD)
    if y_in is not None and rows is not None:
        Y = Y[:, rows]
    with np.errstate(invalid="ignore", over="ignore"):
        WT = wl[keep][None, :] * T[:, keep]
        return Y + (WT @ Zl[keep]).T, np.abs(Y) + (np.abs(WT) @ np.abs(Zl[keep])).T


def propagated(P, w, center, A_z, rows=None):
    """what the scores' own error adds to Y: sum_n |w t_i(n)| (d + 4) u A_z[n][j], (r, d)"""
    T, keep, wl = _centred(P, w, center)
    if rows is not None:
        T = T[rows]
    d = P.shape[0]
    return (d + 4) * U * (np.abs(wl[keep][None, :] * T[:, keep]) @ A_z[keep]).T


def bound_scores(d, A_z):
    """|gpu - ref| <= (d + 4) 2^-53 A_z: d products added in some order ((d - 1) u relative to the absolute sum, padding terms are
    exact zeros) and one rounding per centring; the product is exact inside the fused multiply-add"""
    return (d + 4) * U * A_z


def bound(M, A):
    """|gpu - ref| <= (M + 4) 2^-53 A_Y, M the number of added terms (K N_r, plus 1 with a carry): the form and derivation of
    pool_cross_reference.bound (the centring and the weight round a term's first factor, the second is the given score)"""
    return (M + 4) * U * A

