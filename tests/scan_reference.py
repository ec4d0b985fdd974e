"""Extended-precision per-draw reference of the single-pass ELBO scan (pathfinder.jl_amd/csrc/elbo_qf_kernel.hip).  Not collected by
pytest; used by tests/test_gpu_scan_reference.py and pinned on the CPU by tests/test_scan_reference_cpu.py.

For one fit and a subset of its draws it restates, in np.longdouble, what oracle/pf_oracle.c computes in double:
  normals  u = po.randn_fill(seed, d, ., n0 + n)             (bit-identical to the device's normals, pinned in test_oracle_rng.py)
  draw     x = mu + s . Q [V' u_1; u_2],  Q = H_0 .. H_{k-1}    (pfo_rand_and_logpdf / pfo_lmul_L / pfo_apply_q, reflector by reflector)
  logq     -(d log 2pi + logdet + |u|^2) / 2                  (logdet: the factor's own, an input of the scan)
  logp     pfo_logp_gauss (diagonal, low-rank part, offset) or pfo_logp_funnel
and, per draw, the SCALES the scan's rounding error is proportional to:
  S_q = (d log 2pi + |logdet| + |u|^2) / 2
  S_p = |offset| + (sum_i a_i E_i^2 + sum_j Gab_j^2) / 2                                  (Gaussian family)
        ((T/3)^2 + (d - 1) T + exp(-tau) (1 + T) sum_{i >= 1} E_i^2) / 2                  (funnel, T = E_0)
  with E = |mu - m| + s . Y, Y = |z| + |Vh| |Tw| |Vh|' |z| (z = [V'u_1; u_2] formed as |V|'|u_1|), Gab = |G| |Wd|' E: the same
  sums as the scan's expanded form with every term replaced by its absolute value (Vh, Tw = the compact-WY form Q = I - Vh Tw Vh' the
  scan contracts with).  A rounding error of relative size eps in any term of the scan's sums moves logp by at most eps S_p.
The factor is the GPU's own (eng.get_fit, in the conventions of helpers.oracle_factor_from_gpu), so the check is per draw and strict
whatever the conditioning of the fit.
"""
import os
import re

import numpy as np

from helpers import oracle_factor_from_gpu
from oracle import pf_oracle as po

LD = np.longdouble
assert np.finfo(LD).eps <= 1e-18, "np.longdouble is not an extended type on this platform: the reference would be double precision"
EPS64 = float(np.finfo(np.float64).eps)
_PI = LD("3.14159265358979323846264338327950288")
LOG2PI = np.log(LD(2) * _PI)

_TAB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pathfinder.jl_amd", "csrc", "pfmi_icdftab.h")


def _tab_const(name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, open(_TAB).read())
    assert m, name
    return int(m.group(1))


ICDF_NB_LDS = _tab_const("PF_ICDF_NB_LDS")            # binades of the scan's LDS copy of the inverse-CDF table
ICDF_TAILBITS = _tab_const("PF_ICDF_TAILBITS")        # words below 2^TAILBITS are refined with a second Philox word
MISS_BELOW = 1 << (31 - ICDF_NB_LDS)                  # |word| below this: outside the LDS copy -> the scan's fix-up (pf_icdf4_fix)
NORMAL_ROUNDS = po.NORMAL_ROUNDS
_M32 = np.uint64(0xFFFFFFFF)


def philox_words(seed, n, g, word3=0, rounds=NORMAL_ROUNDS):
    """Philox4x32-R words of counters (n, g, 0, word3) under key = seed, vectorised over n and g (broadcast); (4, ...) uint64 holding
    uint32 values.  The normal stream's counter layout (pfo_randn4): n = draw (mod 2^32), g = row group of 4."""
    n, g = np.broadcast_arrays(np.asarray(n, dtype=np.uint64) & _M32, np.asarray(g, dtype=np.uint64) & _M32)
    c = [n.copy(), g.copy(), np.zeros_like(n), np.full_like(n, word3)]
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64(int(seed) >> 32)
    for _ in range(rounds):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack(c)


def miss_count(seed, d, draws):
    """normals of rows < d of the given draw counters (n0 + n, any integers: wrapped to 32 bits like the device) whose Philox word lies
    outside the scan's LDS table copy, i.e. that take the look-up's miss path"""
    draws = np.asarray(draws, dtype=np.int64) & 0xFFFFFFFF
    ng = (d + 3) // 4
    W = philox_words(seed, draws[:, None].astype(np.uint64), np.arange(ng, dtype=np.uint64)[None, :])   # (4, n, ng)
    mag = (W & np.uint64(0x7FFFFFFF)).transpose(1, 2, 0).reshape(len(draws), 4 * ng)[:, :d]
    return int(np.sum(mag < MISS_BELOW))


def normals(seed, d, n0, idx):
    """(d, len(idx)) float64: the normals of draws n0 + idx (contiguous runs in one oracle call each)"""
    idx = np.asarray(idx, dtype=np.int64)
    U = np.empty((d, len(idx)))
    s = 0
    while s < len(idx):
        e = s + 1
        while e < len(idx) and idx[e] == idx[e - 1] + 1:
            e += 1
        U[:, s:e] = po.randn_fill(int(seed), d, e - s, int(n0) + int(idx[s]))
        s = e
    return U


class LDFactor:
    """a Pathfinder fit in long double: s = sqrt(alpha), Householder vectors Vh (d x k, unit diagonal), tau, V (k x k upper), mu,
    logdet (the factor's own double), and the compact-WY Tw of Q = H_0 .. H_{k-1} = I - Vh Tw Vh' (for the scales only)"""

    def __init__(self, F, mu):
        d, k = F.d, F.k
        self.d, self.k = d, k
        self.s = np.asarray(F.sqrt_alpha, dtype=LD)
        self.mu = np.asarray(mu, dtype=LD)
        self.logdet = LD(float(F.logdet))
        Vh = np.zeros((d, k), dtype=LD)
        for c in range(k):
            Vh[c, c] = 1
            Vh[c + 1:, c] = np.asarray(F.QR[c + 1:d, c], dtype=LD)
        self.Vh = Vh
        self.tau = np.asarray(F.tau[:k], dtype=LD)
        self.V = np.triu(np.asarray(F.V[:k, :k], dtype=LD))
        Tw = np.zeros((k, k), dtype=LD)                       # LAPACK dlarft, forward / columnwise
        for i in range(k):
            Tw[i, i] = self.tau[i]
            if i:
                Tw[:i, i] = -self.tau[i] * (Tw[:i, :i] @ (Vh[:, :i].T @ Vh[:, i]))
        self.Tw = Tw

    @classmethod
    def from_gpu(cls, eng, p, j):
        f = eng.get_fit(p, j)
        return cls(oracle_factor_from_gpu(f), f["mu"])

    def draws(self, U):
        """U (d, n) normals -> (X, Y_abs) in long double: X = mu + s . Q [V'u_1; u_2], reflector by reflector (pfo_apply_q)"""
        k = self.k
        Z = np.asarray(U, dtype=LD).copy()
        Za = np.abs(Z)
        if k:
            Z[:k] = self.V.T @ Z[:k]                          # lmul!(V', x[1:k])  (src/woodbury.jl:139)
            Za[:k] = np.abs(self.V).T @ Za[:k]
        for c in range(k - 1, -1, -1):                        # lmul!(Q, x): H_{k-1} first  (dorm2r, pfo_apply_q)
            if self.tau[c] == 0:
                continue
            v = self.Vh[c:, c]
            w = self.tau[c] * (v @ Z[c:])
            Z[c:] -= v[:, None] * w[None, :]
        Ya = Za
        if k:
            Ya = Za + np.abs(self.Vh) @ (np.abs(self.Tw) @ (np.abs(self.Vh).T @ Za))
        X = self.mu[:, None] + self.s[:, None] * Z
        return X, Ya


def target_logp(tg, X, Ea):
    """(logp, S_p) in long double of draws X (d, n); Ea = |x - m| bounds (d, n) of the scan's terms"""
    d = X.shape[0]
    if tg.kind == 1:                                          # funnel (pfo_logp_funnel)
        tau = X[0]
        ss = np.sum(X[1:] ** 2, axis=0) * np.exp(-tau)
        lp = ((tau / 3) ** 2 + (d - 1) * tau + ss) / -2
        Ta = Ea[0]
        S = ((Ta / 3) ** 2 + (d - 1) * Ta + np.exp(-tau) * (1 + Ta) * np.sum(Ea[1:] ** 2, axis=0)) / 2
        return lp, S
    mean, a = np.asarray(tg.mean, dtype=LD), np.asarray(tg.a, dtype=LD)
    E = X - mean[:, None]
    q = np.sum(a[:, None] * E * E, axis=0)
    Sq = np.sum(a[:, None] * Ea * Ea, axis=0)
    corr = np.zeros(X.shape[1], dtype=LD)
    Sc = np.zeros(X.shape[1], dtype=LD)
    if tg.r:
        Wd = np.asarray(tg.Wd, dtype=LD).reshape(d, -1)[:, :tg.r]
        G = np.tril(np.asarray(tg.G, dtype=LD).reshape(tg.r, tg.r))
        g = G @ (Wd.T @ E)
        corr = np.sum(g * g, axis=0)
        ga = np.abs(G) @ (np.abs(Wd).T @ Ea)
        Sc = np.sum(ga * ga, axis=0)
    off = LD(tg.offset)
    return off - (q - corr) / 2, abs(off) + (Sq + Sc) / 2


class Ref:
    """per-draw long-double reference of draws n0 + idx of one fit: lp, lq, S_p, S_q (float64 arrays over idx), misses, and -- when idx
    is every draw 0 .. N-1 -- the fit's ELBO and SE in long double (elbo, se; None otherwise)"""

    def __init__(self, F, tg, seed, N, n0=0, idx=None):
        idx = np.arange(N) if idx is None else np.unique(np.asarray(idx, dtype=np.int64))
        assert idx.size and idx[0] >= 0 and idx[-1] < N
        d = F.d
        self.idx, self.N, self.n0 = idx, N, n0
        U = normals(seed, d, n0, idx)
        X, Ya = F.draws(U)
        Ea = np.abs(F.mu - np.asarray(tg.mean, dtype=LD) if tg.kind != 1 else F.mu)[:, None] + F.s[:, None] * Ya
        lp, Sp = target_logp(tg, X, Ea)
        usq = np.sum(np.asarray(U, dtype=LD) ** 2, axis=0)
        lq = -(d * LOG2PI + F.logdet + usq) / 2
        Sq = (d * LOG2PI + abs(F.logdet) + usq) / 2
        self.lp_ld, self.lq_ld, self.X = lp, lq, X
        self.lp, self.lq = lp.astype(np.float64), lq.astype(np.float64)
        self.S_p, self.S_q = Sp.astype(np.float64), Sq.astype(np.float64)
        self.misses = miss_count(seed, d, n0 + idx)
        self.elbo = self.se = None
        if idx.size == N:
            r = lp - lq
            m = np.sum(r) / N
            self.elbo = m
            self.se = np.sqrt(np.sum((r - m) ** 2) / (N - 1) / N) if N > 1 else LD(0)


def scan_reference(eng, p, j_eff, tg, seed, N, n0=0, idx=None):
    """the reference of draws n0 + idx of fit p (history length j_eff) of the engine's last fit_batch, target tg"""
    return Ref(LDFactor.from_gpu(eng, p, int(j_eff)), tg, seed, N, n0, idx)


def draw_subset(N, rng, extra=()):
    """N <= 128: every draw.  Otherwise the first 32, the last 48 (the ragged last group among them), 32 random ones, plus `extra`."""
    if N <= 128:
        return np.arange(N)
    pick = [np.arange(32), np.arange(N - 48, N), rng.choice(N, 32, replace=False), np.asarray(extra, dtype=np.int64)]
    return np.unique(np.concatenate(pick))
