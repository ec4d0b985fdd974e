"""Reference side of the per-run PSIS tests (pfmi_pool_psis_runs; test infrastructure, NumPy only, not collected).

1. `host_diagnostics`: the host arithmetic of RunDiagnostics restated in NumPy (ess, log_evidence, the `ok` mask).
2. `sumsq_rel_bound`, `lse_is_the_constant`: the two checks that have no bit-for-bit counterpart in pfmi_psis -- the sum of squared
   weights (any summation order of N non-negative terms is within N 2^-52 relative of the exact sum, hence of np.sum) and the
   logsumexp (it is the constant the kernel subtracted: fl(lr_i - lse) must be log_weights_i at every index PSIS did not replace).
3. `prescribed`: the special-value vectors, one per run.
4. `oracle_pool_ratios`: the log ratios of pool_common's named pools from the CPU oracle's own fits and draws (no GPU), on which the
   oracle is admitted as the GPU tests' reference.
"""
import numpy as np

import psis_reference as pr


# ---- 1. host arithmetic ---------------------------------------------------------------------------------------------------------------
def host_diagnostics(pareto_k, lse, sumsq, N_r, threshold=0.7):
    """(ess, log_evidence, ok): 1 / sumsq, lse - log(N_r), and k <= threshold with False where k is NaN"""
    k = np.asarray(pareto_k, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.float64(1.0) / np.asarray(sumsq, dtype=np.float64)
        ok = np.array([(not np.isnan(v)) and bool(v <= threshold) for v in k], dtype=bool)
    return ess, np.asarray(lse, dtype=np.float64) - np.log(np.float64(N_r)), ok


# ---- 2. the checks without a bit-for-bit counterpart ----------------------------------------------------------------------------------
def sumsq_rel_bound(N_r):
    """worst case of a sum of N_r non-negative terms added in any order, relative to the exact sum"""
    return N_r * 2.0 ** -52


def same_bits(a, b):
    """elementwise: the same float64 bit pattern, or both NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def lse_is_the_constant(lr, log_weights, lse, pareto_k):
    """indices at which fl(lr_i - lse) differs from log_weights_i, among the indices PSIS did not replace: all of them when nothing
    was fitted (no tail, or pareto_k NaN), else everything outside the tail of psis_reference.tail_indices"""
    lr = np.ascontiguousarray(lr, dtype=np.float64)
    keep = np.ones(len(lr), dtype=bool)
    tail, _ = pr.tail_indices(lr)
    if tail is not None and not np.isnan(pareto_k):
        keep[tail] = False
    with np.errstate(invalid="ignore"):
        want = lr - np.float64(lse)
    return np.flatnonzero(keep & ~same_bits(want, log_weights))


# ---- 3. prescribed vectors --------------------------------------------------------------------------------------------------------------
def _signed_zeros(S, rng):
    """ten log ratios alternating +0.0 / -0.0 straddle the cutoff, one of them in the tail: by isless the +0.0 of largest index.  (One
    only: the shifted tail starts with as many exact zeros, and the grid of the fit divides by its entry (M + 2) / 4 - 1, which is entry
    1 at M = 8.)"""
    M = pr.tail_length(S)
    grp = np.sort(rng.choice(S, 10, replace=False))
    lr = -np.abs(rng.normal(size=S)) * 1.5 - 1e-3
    others = np.setdiff1d(np.arange(S), grp)
    up = rng.choice(others, M - 1, replace=False)
    lr[up] = np.abs(rng.normal(size=M - 1)) * 1.5 + 1e-3
    lr[grp] = np.where(np.arange(10) % 2 == 0, 0.0, -0.0)
    return lr


def _constant_tail(S, rng):
    """the M + 1 largest all equal (M + 3 entries at 5.0 above a clipped body): the shifted tail is zero, nothing is fitted"""
    lr = np.minimum(pr._light(rng, S), 4.0)
    lr[rng.choice(S, pr.tail_length(S) + 3, replace=False)] = 5.0
    return lr


def prescribed(N_r):
    """name -> log ratios of one run.  isless puts every NaN above +Inf, so a single NaN always lies IN the tail; "outside" needs more
    NaNs than the tail holds: M + 2 of them (both signs) fill the tail, the cutoff and one place below it.  At N_r = 1000 the rows of
    psis_reference.CASES of that size are used as they are."""
    rng = np.random.default_rng(4000 + N_r)
    M = pr.tail_length(N_r)
    assert M >= 5 and N_r > M + 12
    light = lambda: pr._light(rng, N_r)                                                     # noqa: E731
    out = {"all_equal": np.full(N_r, -1.25), "all_neginf": np.full(N_r, -np.inf)}
    v = light(); v[N_r // 3] = pr._nan(False); out["nan_in_tail"] = v
    v = light(); idx = rng.choice(N_r, M + 2, replace=False)
    v[idx] = np.where(np.arange(M + 2) % 2 == 0, pr._nan(False), pr._nan(True)); out["nan_outside_tail"] = v
    v = light(); v[(2 * N_r) // 3] = np.inf; out["one_posinf"] = v
    if N_r == 1000:
        out["signed_zeros"] = np.array(pr.case_lr("signed_zeros_1000"))
        out["constant_tail"] = np.array(pr.case_lr("degenerate_1000"))
        out["nan_in_tail"] = np.array(pr.case_lr("nan_neg_1000"))
    else:
        out["signed_zeros"] = _signed_zeros(N_r, rng)
        out["constant_tail"] = _constant_tail(N_r, rng)
    out["light"] = light()
    return {k: np.ascontiguousarray(x, dtype=np.float64) for k, x in out.items()}


PRESCRIBED_POOLS = (("all_equal", "nan_in_tail", "nan_outside_tail"), ("all_neginf", "one_posinf", "signed_zeros"),
                    ("constant_tail", "light", "all_equal"))


# ---- 4. the named pools on the CPU oracle ---------------------------------------------------------------------------------------------
def oracle_pool_ratios(pfmi, name, K, N_r, J=6):
    """log ratios [K N_r] of pool_common._pool(name, K, N_r) from the oracle alone: the same traces, every path's last fit, N_r draws
    from seed 1000 + 7 k -- the oracle's factor, its normals, its target"""
    from helpers import oracle_target
    from oracle import pf_oracle as po
    from pool_common import _traces
    tg, traces = _traces(pfmi, name)
    otg = oracle_target(tg)
    out = []
    for k in range(K):
        tr = traces[k]
        alpha_all, hl, hs, _ = po.lbfgs_history(tr.points, tr.gradients, J)
        l = len(tr.points) - 1
        j = int(hl[l])
        d = tr.points.shape[1]
        S = np.stack([tr.points[s + 1] - tr.points[s] for s in hs[l, :j]], axis=1) if j else np.zeros((d, 0))
        Y = np.stack([tr.gradients[s] - tr.gradients[s + 1] for s in hs[l, :j]], axis=1) if j else np.zeros((d, 0))
        B, D = po.lbfgs_inverse_hessian(alpha_all[l], S, Y)
        F = po.Factor(alpha_all[l], B, D)
        assert F.status == 0, (name, k, F.status)
        X, logq = F.rand_and_logpdf(F.fit_mean(tr.points[l], tr.gradients[l]), po.randn_fill(1000 + 7 * k, d, N_r))
        out.append(otg.logp(X) - logq)
    return np.concatenate(out)
