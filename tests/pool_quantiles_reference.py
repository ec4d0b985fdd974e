"""Reference of pfmi_pool_cdf and of the weighted type-1 quantiles built on it (definition: include/pfmi.h), in NumPy longdouble: a
stable sort per row, cumulative weights with ties merged, then the definition.  Not collected by pytest."""
import numpy as np

LD = np.longdouble


def _counted(X, w):
    """X (d, S), w (S,) or None -> (X of the counted columns, their weights as longdouble)"""
    X = np.asarray(X, dtype=np.float64)
    if w is None:
        return X, np.ones(X.shape[1], dtype=LD)
    w = np.asarray(w, dtype=np.float64)
    assert w.shape == (X.shape[1],)
    keep = w != 0.0                                # a column of weight exactly 0 is skipped whatever it holds
    return X[:, keep], w[keep].astype(LD)


def cdf(P, w, T):
    """P (d, S) pool, w (S,) weights or None (= 1, nothing skipped), T (nthr, d) thresholds:
    dict(wle, below, above (nthr, d): wle longdouble, the others float64; nanflag (d,) int32)"""
    X, wl = _counted(P, w)
    T = np.asarray(T, dtype=np.float64)
    nthr, d = T.shape
    wle = np.zeros((nthr, d), dtype=LD)
    below = np.full((nthr, d), -np.inf)
    above = np.full((nthr, d), np.inf)
    for j in range(nthr):
        le = X <= T[j][:, None]                    # (a NaN compares false on both sides)
        gt = X > T[j][:, None]
        wle[j] = np.where(le, wl[None, :], LD(0)).sum(axis=1)
        below[j] = np.max(np.where(le, X, -np.inf), axis=1, initial=-np.inf)
        above[j] = np.min(np.where(gt, X, np.inf), axis=1, initial=np.inf)
    return dict(wle=wle, below=below, above=above, nanflag=np.isnan(X).any(axis=1).astype(np.int32))


def row_table(x, wl):
    """distinct values of one row in ascending order, U (weight at or below) and L (weight strictly below) per value"""
    order = np.argsort(x, kind="stable")
    xs, cw = x[order], np.cumsum(wl[order])
    last = np.concatenate([xs[1:] != xs[:-1], [True]])          # the last column of every run of ties
    vals, U = xs[last], cw[last]
    return vals, U, np.concatenate([[LD(0)], U[:-1]])


def quantiles(P, w, probs, W=None):
    """Weighted type-1 quantiles of every row of P (d, S) under weights w (S,) (None: unit weights) at `probs`; W: the total weight
    the targets p * W are formed with (a float64, as the host has it; default: the longdouble sum rounded to float64).
    Returns (q (nq, d) float64, margin (nq, d) longdouble = min(U(q) - p W, p W - L(q)))."""
    X, wl = _counted(P, w)
    probs = np.asarray(probs, dtype=np.float64)
    d = X.shape[0]
    if W is None:
        W = np.float64(wl.sum())
    q = np.full((probs.size, d), np.nan)
    margin = np.full((probs.size, d), np.nan, dtype=LD)
    if not W > 0:
        return q, margin
    for i in range(d):
        if np.isnan(X[i]).any():
            continue
        vals, U, L = row_table(X[i], wl)
        for a, p in enumerate(probs):
            t = LD(np.float64(p) * np.float64(W))                   # that double product
            m = int(np.searchsorted(U, t, side="left"))             # the first value with U >= t
            m = min(m, vals.size - 1)                               # none (rounding at p = 1): the largest value
            q[a, i] = vals[m]
            margin[a, i] = min(U[m] - t, t - L[m])
    return q, margin
