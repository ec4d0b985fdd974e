"""Cheap synthetic fits for the extended-precision parity modules (tests/test_gpu_scan_reference.py, tests/test_gpu_draw_reference.py):
traces that every fit accepts in full, the built-in target families by (TGT, RPAD), and the fitted engine state.  Not collected by
pytest."""
import numpy as np

import scan_reference as sr


def _walk(pfmi, m, sig, K, L, seed):
    """K synthetic optimisation traces of L + 1 points towards m on the diagonal Gaussian (m, sig^2) with its exact gradients: every
    pair has s'y > 0, so every fit takes min(l, J) pairs -- cheap traces for any d and any number of fits"""
    tt = pfmi.GaussTarget(m, sig ** 2)
    rng = np.random.default_rng(seed)
    d = len(m)
    th, gr = [], []
    for _ in range(K):
        w = rng.uniform(-2, 2, d)
        pts = []
        for i in range(L + 1):
            pts.append(m + sig * w)
            w = 0.75 * w + 0.5 * 0.85 ** i * rng.normal(size=d)
        P = np.array(pts)
        th.append(P)
        gr.append(np.array([tt.grad(x) for x in P]))
    return th, gr


def _target(pfmi, tgt, rpad, m, sig, seed, mean_shift=None):
    d = len(m)
    if tgt == 2:
        return pfmi.FunnelTarget(d)
    rng = np.random.default_rng(seed)
    r = {0: 0, 8: 5, 16: 12}[rpad]
    mm = m if mean_shift is None else m + mean_shift
    W = 0.3 * rng.normal(size=(d, r)) if r else None
    return pfmi.GaussTarget(mm, sig ** 2, W, offset=1.25 if r == 0 else -0.5)


class Setup:
    """traces of K paths x (L + 1) points at dimension d, fitted with history length J"""

    def __init__(self, pfmi, eng, d, J, K, L, seed=1, sig=None, mean=None):
        rng = np.random.default_rng(100 + seed)
        self.m = rng.normal(size=d) if mean is None else mean
        self.sig = np.exp(rng.uniform(-0.7, 0.7, d)) if sig is None else sig
        th, gr = _walk(pfmi, self.m, self.sig, K, L, seed)
        eng.set_target(pfmi.GaussTarget(self.m, self.sig ** 2))
        eng.set_traces(th, gr)
        eng.fit_batch(J)
        self.status, self.jeff, _, _ = eng.fit_status()
        self.d, self.J, self.P = d, J, eng.P
        self.offsets = np.asarray(eng.offsets)
        starts = set(self.offsets[:-1].tolist())
        self.fits = np.array([p for p in range(eng.P) if p not in starts])          # the scan's fit list (point 0 of a path has none)
        self.ok = np.array([p for p in self.fits if self.status[p] == 0])
        self.seeds = np.array([sr.po.rand_u64(7 + seed, p, 9) for p in range(eng.P)], dtype=np.uint64)
        assert len(self.ok) >= 1 and self.status[self.fits[-1]] == 0
