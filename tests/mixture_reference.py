"""Reference side of the mixture logpdf tests (tests/test_gpu_mixture.py, tests/test_gpu_mixture_geometry.py,
tests/test_mixture_reference_cpu.py).  Plain NumPy, no GPU.  Not collected by pytest.

  ref_logpdf          logpdf of one fit in long double, from (alpha, B, D, mu) alone: nothing of the factor the kernels read
  mixture_geometry    what pf_launch_mixture_logpdf (csrc/mixture_kernels.hip) launches for (d, kpad, N, K, ncu): kernel, STAGE,
                      components per workgroup, groups, LDS bytes -- a restatement of the launcher's rules
  GRID / components   the (J, d) rows of the geometry tests, their targets, and the rule that picks their components; the CPU side
                      (oracle factors) and the GPU side (Engine) apply the same rule, so the sensitivity test of
                      test_mixture_reference_cpu.py speaks about the components the GPU tests run
  lane_logpdf         the float64 algebra of pf_logpdf_lane on a factor given as (Vh, T, V, mu, 1 / sqrt(alpha), logdet): what a
                      kernel computes when one of its staged buffers holds another component's data
"""
import numpy as np
from scipy.linalg import solve_triangular

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON   # noqa: F401  (one long-double skip convention for the suite)

LD = np.longdouble


# ---- extended-precision reference ----------------------------------------------------------------------------------------------------
def _solve_ld(M, R):
    """M^{-1} R by Gaussian elimination with partial pivoting in long double; also log|det M|"""
    M = M.astype(LD).copy()
    R = R.astype(LD).copy()
    m = M.shape[0]
    logdet = LD(0)
    for c in range(m):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
            R[[c, piv]] = R[[piv, c]]
        logdet += np.log(np.abs(M[c, c]))
        f = M[c + 1:, c] / M[c, c]
        M[c + 1:, c:] -= np.outer(f, M[c, c:])
        R[c + 1:] -= np.outer(f, R[c])
    for c in range(m - 1, -1, -1):
        R[c] = (R[c] - M[c, c + 1:] @ R[c + 1:]) / M[c, c]
    return R, logdet


def _chol_ld(S):
    n = S.shape[0]
    L = np.zeros_like(S)
    for j in range(n):
        v = S[j, j] - L[j, :j] @ L[j, :j]
        L[j, j] = np.sqrt(v)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def ref_logpdf(f, X, route=None):
    """logpdf(MvNormal(mu, diag(alpha) + B D B'), X) in long double: dense Sigma and a Cholesky for d <= 64, the Woodbury identity
    (A + B D B')^{-1} = A^{-1} - A^{-1} B (I + D G)^{-1} D B' A^{-1}, G = B' A^{-1} B, det = det A det(I + D G) above.
    route "dense" / "woodbury" forces one of the two at any d (the reference checked against itself)"""
    a, B, D, mu = (f[k].astype(LD) for k in ("alpha", "B", "D", "mu"))
    d, m = B.shape
    Z = np.asarray(X, dtype=LD) - mu[:, None]
    if route == "dense" or (route is None and d <= 64):
        L = _chol_ld(np.diag(a) + B @ D @ B.T)
        Y = Z.copy()
        for i in range(d):                                # forward substitution L y = z
            Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
        quad = np.sum(Y * Y, axis=0)
        logdet = 2 * np.sum(np.log(np.diag(L)))
    else:
        AiB = B / a[:, None]
        quad = np.sum(Z * Z / a[:, None], axis=0)
        logdet = np.sum(np.log(a))
        if m:
            M = np.eye(m, dtype=LD) + D @ (B.T @ AiB)
            U = AiB.T @ Z                                 # B' A^{-1} z
            S, ld = _solve_ld(M, D @ U)
            quad = quad - np.sum(U * S, axis=0)
            logdet = logdet + ld
    return (-(d * np.log(2 * LD(np.pi)) + logdet) / 2 - quad / 2).astype(np.float64)


def _top_eig(f):
    """(lambda_max, v_max) of Sigma = diag(alpha) + B D B'"""
    a, B, D = f["alpha"], f["B"], f["D"]
    d = len(a)
    if d <= 512:
        lam, V = np.linalg.eigh(np.diag(a) + B @ D @ B.T)
        return lam[-1], V[:, -1]
    v = np.random.default_rng(0).normal(size=d)
    for _ in range(500):                                  # power iteration on the low-rank-plus-diagonal operator
        w = a * v + B @ (D @ (B.T @ v))
        v = w / np.linalg.norm(w)
    return float(v @ (a * v + B @ (D @ (B.T @ v)))), v


# ---- the launcher's rules (pf_launch_mixture_logpdf) --------------------------------------------------------------------------------
MX_STATIC_LDS = {4: 2784, 8: 3072, 12: 3424, 16: 3840, 20: 6368, 32: 8192}   # doubles: wred, ntv, wsum, head, sred, t_s, vc_s
MX_LDS_MAX = 160 * 1024
MX_DMAX = 1024


def mx_static_lds(kpad):
    """mx_static_lds of mixture_kernels.hip: 8 waves x ceil(kpad / 16) W fragments of 4 x 64, three kpad x 16 tiles, 8 x 64 partial
    sums, T and V"""
    return 8 * ((kpad + 15) // 16) * 4 * 64 + 3 * kpad * 16 + 8 * 64 + 2 * kpad * kpad


def kpad_for(J):
    return next(o for o in (4, 8, 12, 16, 20, 32, 64) if 2 * J <= o)


def mixture_geometry(d, kpad, N, K, ncu):
    """dict(route, stage, cpb, ngroups, lds_bytes) of an unforced pfmi_mixture_logpdf call.  route "mfma": the main kernel, groups of
    cpb components per 16-point tile, ng = ceil(8 ncu / ntiles) groups wanted (at most K), the factor staged in LDS where static +
    dynamic LDS fit in 160 KB; route "lane": one grid row per component, no LDS"""
    if d > MX_DMAX or kpad > 32:
        return dict(route="lane", stage=False, cpb=1, ngroups=K, lds_bytes=0)
    ntiles = (N + 15) // 16
    ng = min(max(-(-8 * ncu // ntiles), 1), K)
    cpb = -(-K // ng)
    static = 8 * MX_STATIC_LDS[kpad]
    dyn = 8 * 32 * ((d + 31) // 32) * (kpad + 2)
    stage = static + dyn <= MX_LDS_MAX
    return dict(route="mfma", stage=stage, cpb=cpb, ngroups=-(-K // cpb), lds_bytes=static + (dyn if stage else 0))


def natural_N(ncu):
    """a number of points at which the unforced launcher loops over components: ntiles = ncu + 2, so ng = ceil(8 ncu / (ncu + 2)) = 8
    for every ncu >= 15, and K = 20 gives cpb = 3 and 7 groups, the last of 2 components; the last tile holds 5 points"""
    return 16 * (ncu + 1) + 5


# ---- the rows of the geometry tests ---------------------------------------------------------------------------------------------------
# (J, d, STAGE or None for the lane route): every reachable instantiation <kpad, STAGE> of pf_mixture_mfma_kernel at d > 128, both sides
# of the STAGE boundary of kpad 16 / 20 / 32, d at and around a 32-row step, a 128-row block, the 1024-row limit, and d < kpad
GRID = [(2, 200, True), (4, 257, True), (6, 1024, True), (8, 896, True), (8, 897, False), (10, 640, True), (10, 641, False),
        (16, 352, True), (16, 353, False), (16, 1024, False),
        (6, 5, True), (6, 31, True), (6, 32, True), (6, 33, True), (6, 128, True), (6, 129, True), (6, 1025, None)]
INVARIANCE = [(6, 1024), (8, 896), (10, 641), (16, 353), (6, 33)]       # group-size invariance (bit-exact)
NATURAL = (6, 64)                                                        # the unforced launcher, K = 20
FAILED = (5, 40)                                                         # the failed-fit construction of test_gpu_mixture.py
SEED, MAXITERS, PER_PATH = 7, 60, 3


def grid_target(pfmi, d):
    """a target whose two 60-iteration L-BFGS paths fill a history of every J of the grid"""
    return pfmi.t_lowrank(d, r=min(8, max(1, d // 2)), seed=4)


def grid_traces(pfmi, J, d):
    from helpers import make_traces
    return make_traces(grid_target(pfmi, d), 2, SEED, history_length=J, maxiters=MAXITERS)


def pick_points(npts, jeff, J, per_path=PER_PATH):
    """the components of a row: of each path the fit points with a full history (jeff == J), per_path of them evenly spread over the
    first half (later fits of a converging path have all but the same mean on every path), the paths interleaved -- so a component's
    predecessor in the list is a fit of the other path.
    npts: points per path; jeff: per fit point, paths concatenated.  Returns fit point numbers."""
    off = np.concatenate([[0], np.cumsum(npts)]).astype(int)
    per = []
    for k in range(len(npts)):
        cand = off[k] + np.flatnonzero(np.asarray(jeff[off[k]:off[k + 1]]) == J)
        assert (len(cand) - 1) // 2 >= per_path - 1, (k, len(cand), per_path)
        per.append([int(cand[i]) for i in np.round(np.linspace(0, (len(cand) - 1) // 2, per_path)).astype(int)])
    return [per[k][i] for i in range(per_path) for k in range(len(npts))]


def make_points(pts, fits, draw, extra=True):
    """the columns of _points of test_gpu_mixture.py (draws of each component, the next component's mean, the point 50 standard
    deviations out along the component's top eigenvector), plus with `extra` the mean of the components' means.
    draw(p) -> (d, ndraw) draws of fit p"""
    cols = []
    for k, p in enumerate(pts):
        cols.append(draw(p))
        cols.append(fits[pts[(k + 1) % len(pts)]]["mu"][:, None])
        lam, v = _top_eig(fits[p])
        cols.append((fits[p]["mu"] + 50 * np.sqrt(lam) * v)[:, None])
    if extra:
        cols.append(np.mean([fits[p]["mu"] for p in pts], axis=0)[:, None])
    return np.asfortranarray(np.concatenate(cols, axis=1))


# ---- the components on the CPU (oracle factors) ---------------------------------------------------------------------------------------
def oracle_components(traces, J, per_path=PER_PATH):
    """(pts, fits, comps) of the traces by the oracle: pts by pick_points; fits[p] = dict(alpha, B, D, mu, logdet) for ref_logpdf;
    comps[p] = dict(Vh, T, V, mu, rsqa, logdet), the arrays the mixture kernel reads for fit p (T: LAPACK dlarft of the reflectors)"""
    from oracle import pf_oracle as po
    hist, jeff = [], []
    for tr in traces:
        alpha_all, hl, hs, _ = po.lbfgs_history(tr.points, tr.gradients, J)
        hist.append((alpha_all, hl, hs))
        jeff.extend(int(v) for v in hl)
    npts = [len(tr) for tr in traces]
    off = np.concatenate([[0], np.cumsum(npts)]).astype(int)
    pts = pick_points(npts, jeff, J, per_path)
    fits, comps = {}, {}
    for p in pts:
        k = int(np.searchsorted(off, p, side="right") - 1)
        l, tr = p - off[k], traces[k]
        alpha_all, hl, hs = hist[k]
        d = tr.points.shape[1]
        S = np.stack([tr.points[s + 1] - tr.points[s] for s in hs[l, :J]], axis=1)
        Y = np.stack([tr.gradients[s] - tr.gradients[s + 1] for s in hs[l, :J]], axis=1)
        B, D = po.lbfgs_inverse_hessian(alpha_all[l], S, Y)
        F = po.Factor(alpha_all[l], B, D)
        assert F.status == 0, (p, F.status)
        mu = F.fit_mean(tr.points[l], tr.gradients[l])
        fits[p] = dict(alpha=F.alpha, B=F.B, D=F.D, mu=mu, logdet=F.logdet)
        kk = F.k
        Vh = np.tril(F.QR[:, :kk], -1) + np.eye(d, kk)
        T = np.zeros((kk, kk))
        for i in range(kk):                               # LAPACK dlarft, forward / columnwise
            T[i, i] = F.tau[i]
            if i:
                T[:i, i] = -F.tau[i] * (T[:i, :i] @ (Vh[:, :i].T @ Vh[:, i]))
        comps[p] = dict(Vh=Vh, T=T, V=np.triu(F.V[:kk, :kk]), mu=mu, rsqa=1.0 / F.sqrt_alpha, logdet=F.logdet)
    return pts, fits, comps


def oracle_draws(fits, comps, ndraw=4, seed=11):
    """draw(p) for make_points from the oracle's factor: mu + sqrt(alpha) . Q [V'u_1; u_2] with the device's normals of (seed, p)"""
    from helpers import fit_seeds
    from oracle import pf_oracle as po
    seeds = fit_seeds(max(fits) + 1, seed)

    def draw(p):
        c = comps[p]
        d, k = c["Vh"].shape
        Z = po.randn_fill(int(seeds[p]), d, ndraw).copy()
        Z[:k] = c["V"].T @ Z[:k]
        Z = Z - c["Vh"] @ (c["T"] @ (c["Vh"].T @ Z))
        return fits[p]["mu"][:, None] + Z / c["rsqa"][:, None]
    return draw


def lane_logpdf(c, X):
    """pf_logpdf_lane in float64 NumPy on the arrays of one component: e = (x - mu) / sqrt(alpha), r = e - Vh T'(Vh' e), V' y = r[:k],
    -(d log 2 pi + logdet) / 2 - (|y|^2 + |r[k:]|^2) / 2"""
    d, k = c["Vh"].shape
    e = (np.asarray(X, dtype=np.float64) - c["mu"][:, None]) * c["rsqa"][:, None]
    r = e - c["Vh"] @ (c["T"].T @ (c["Vh"].T @ e))
    y = solve_triangular(c["V"], r[:k], trans="T", lower=False)
    ss = np.sum(y * y, axis=0) + np.sum(r[k:] * r[k:], axis=0)
    return -(d * np.log(2 * np.pi) + c["logdet"]) / 2 - ss / 2
