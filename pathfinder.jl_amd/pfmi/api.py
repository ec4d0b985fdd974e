"""Host-side mirror of the reference's public API for the hot path:

    pathfinder()       reference src/singlepath.jl:142-257
    multipathfinder()  reference src/multipath.jl:118-245
    resample()         reference src/resample.jl:20-46
    fit_mvnormals()    reference src/mvnormal.jl:14-21
    maximize_elbo()    reference src/elbo.jl:1-10

Same names, argument meaning and failure behaviour; the numerics run in libpfmi.so on the GPU.  Runs
are batched: the host performs the K optimisations (each with its own seeded rng copy, as
src/multipath.jl:190-193), then ONE fit_batch / elbo_batch / pool_build covers every path.

(The north-star host language is Julia; no Julia toolchain exists in this image, so the host mirror
is Python and the Julia `ccall` wrapper lives, untested, in pathfinder.jl_amd/julia/ -- INTEGRATION.md.)
"""
import dataclasses
import gc
import os
import warnings
from collections.abc import Sequence
from dataclasses import dataclass, field
from typing import Any, List, Optional

import numpy as np

from ._lib import PfmiError, PfmiRetry
from .core import Engine, StaleHandleError  # noqa: F401
from .hostrng import HostRNG, rand_u64_multi
from .optimize import OptimizationTrace, optimize_with_trace

DEFAULT_HISTORY_LENGTH = 6     # src/Pathfinder.jl:24
DEFAULT_NDRAWS_ELBO = 5        # src/Pathfinder.jl:27
_RETRIES = 2                   # how often a call is re-enqueued after PFMI_ERR_RETRY (pfmi._lib.PfmiRetry)


class _LazySeq(Sequence):
    """list-like whose items are built on first access (the reference materialises L fits / ELBO estimates per path;
    at 10^4 fits that is pure host overhead when only a few are ever looked at)"""

    def __init__(self, n, make):
        self._n, self._make, self._items = n, make, {}

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        if i not in self._items:
            self._items[i] = self._make(i)
        return self._items[i]


class PosDefException(ArithmeticError):
    """mirrors LinearAlgebra.PosDefException thrown by pdfactorize (src/woodbury.jl:202,205)"""


# ---- distribution objects -------------------------------------------------------------------------------
@dataclass
class WoodburyPDFactorization:      # src/woodbury.jl:12-21
    U: np.ndarray                   # diag of the (diagonal) Cholesky factor of A = sqrt(alpha)
    Q_factors: np.ndarray           # QRCompactWY factors (d x 2j)
    Q_T: np.ndarray                 # compact-WY T (k x k)
    V: np.ndarray                   # upper Cholesky factor (k x k)


@dataclass
class WoodburyPDMat:                # src/woodbury.jl:246-257
    A: np.ndarray                   # diagonal (d,)
    B: np.ndarray                   # (d, 2j)
    D: np.ndarray                   # (2j, 2j)
    F: WoodburyPDFactorization
    logdet: float

    engine: Any = field(repr=False, default=None)
    point: int = -1
    token: Any = field(repr=False, default=None)      # engine.fit_token() this handle was made under

    def dense(self):
        return np.diag(self.A) + self.B @ self.D @ self.B.T

    def _op(self, op, x):
        if self.engine is None:
            raise RuntimeError("this WoodburyPDMat was built on the host (inv / scaling): it has no device factor")
        self.engine.check_token(self.token, "WoodburyPDMat")
        return self.engine.woodbury_apply(self.point, op, x)

    # PDMats surface on the device (reference src/woodbury.jl:326-423)
    def unwhiten(self, x): return self._op("unwhiten", x)
    def whiten(self, x): return self._op("whiten", x)
    def invunwhiten(self, x): return self._op("invunwhiten", x)
    def mul(self, x): return self._op("mul", x)
    def solve(self, x): return self._op("solve", x)
    def quad(self, x): return self._op("quad", x)
    def invquad(self, x): return self._op("invquad", x)

    def diag(self):
        if self.engine is None:
            return self.A + np.einsum("ij,jk,ik->i", self.B, self.D, self.B)
        self.engine.check_token(self.token, "WoodburyPDMat")
        return self.engine.woodbury_diag(self.point)

    # inv(W) and W * c build NEW WoodburyPDMat objects on the host from the downloaded pieces, exactly as the reference does
    # (src/woodbury.jl:50-52, 218-223, 317-321, 357-360); they carry no engine handle (dense() / diag() work, the device operators do not).
    def thin_Q(self):
        """first k columns of Q = I - Vh T Vh' (Vh = unit-lower Householder vectors of F.Q_factors)"""
        d, k = self.B.shape[0], self.F.V.shape[0]
        Vh = np.tril(self.F.Q_factors[:, :k], -1) + np.eye(d, k)
        Q1 = -Vh @ (self.F.Q_T @ Vh[:k, :].T)
        Q1[:k, :] += np.eye(k)
        return Q1

    def inv(self):
        """inv(W) = WoodburyPDMat(pdunfactorize(inv(F))...): F^-1 = (U'^-1, Q, V'^-1), A = U'U, B = U'Q, D = V'V - I"""
        Ui = 1.0 / self.F.U                                       # inv(U') of the diagonal U
        k = self.F.V.shape[0]
        Vi = np.linalg.solve(self.F.V.T, np.eye(k)) if k else np.zeros((0, 0))     # inv(V'): lower triangular
        Fi = WoodburyPDFactorization(Ui, self.F.Q_factors, self.F.Q_T, Vi)
        B = Ui[:, None] * self.thin_Q()
        D = Vi.T @ Vi - np.eye(k)
        return WoodburyPDMat(Ui * Ui, B, D, Fi, -self.logdet)

    def __mul__(self, c):
        """W * c (src/woodbury.jl:357-360): c > 0 -> WoodburyPDMat(A c, B, D c), otherwise the dense matrix times c"""
        c = float(c)
        if not c > 0:
            return self.dense() * c
        sc = np.sqrt(c)
        F = WoodburyPDFactorization(self.F.U * sc, self.F.Q_factors, self.F.Q_T, None)     # V of the scaled matrix is not formed
        return WoodburyPDMat(self.A * c, self.B.copy(), self.D * c, F, self.logdet + len(self.A) * np.log(c))

    __rmul__ = __mul__

    # the rest of the surface the reference tests (test/woodbury.jl:228-309)
    @property
    def dim(self): return len(self.A)                               # PDMats.dim, src/woodbury.jl:367

    @property
    def T(self): return self                                        # adjoint / transpose: W is symmetric (src/woodbury.jl:313-315)

    def __add__(self, c):
        """W + c I (src/woodbury.jl:333-338: through PDMats' ScalMat sum, i.e. a dense matrix)"""
        return self.dense() + float(c) * np.eye(len(self.A))

    __radd__ = __add__

    def rdiv(self, X):
        """X / W for row vectors / row blocks (n,) or (r, n): (W \\ X')' with the device solve (test/woodbury.jl:299-305)"""
        X = np.asarray(X, dtype=np.float64)
        return self.solve(X.T.copy()).T if X.ndim == 2 else self.solve(X)


@dataclass
class MvNormal:
    """MvNormal{WoodburyPDMat} (src/mvnormal.jl:18).  mu / Sigma may be left to be downloaded from the engine on first access
    (multipathfinder keeps ~10^4 of these as handles)."""
    mu_: Any
    Sigma_: Any
    engine: Any = field(repr=False, default=None)
    point: int = -1
    j: int = -1                      # effective history length of this fit (needed to size B, D when materialising)
    token: Any = field(repr=False, default=None)      # engine.fit_token() this handle was made under

    def _live(self):
        self.engine.check_token(self.token, "MvNormal")

    def _materialise(self):
        if self.Sigma_ is None and self.engine is not None and self.j >= 0:
            self._live()
            f = self.engine.get_fit(self.point, self.j)
            F = WoodburyPDFactorization(np.sqrt(f["alpha"]), f["qr_factors"], f["T"], f["V"])
            self.Sigma_ = WoodburyPDMat(f["alpha"], f["B"], f["D"], F, f["logdet"], self.engine, self.point, self.token)
            self.mu_ = f["mu"]
        return self

    @property
    def mu(self): return self._materialise().mu_
    @property
    def Sigma(self): return self._materialise().Sigma_

    def logpdf(self, X):
        self._live()
        return self.engine.logpdf(self.point, X)

    def rand(self, seed, n, n0=0):
        self._live()
        return self.engine.draws(self.point, seed, n, n0)[0]


class MixtureModel(list):
    """Distributions.MixtureModel of the K runs' fits with uniform prior (src/multipath.jl:215-216).  It IS the list of the MvNormal
    components, so every use of fit_distribution as a list stays valid.  Densities run on the device: each engine evaluates its
    own components in one call (Engine.mixture_logpdf, include/pfmi.h pfmi_mixture_logpdf) and the per-engine sums are combined
    with logaddexp in engine order.  A component whose engine has been refitted raises StaleHandleError."""

    @property
    def ncomponents(self): return len(self)

    @property
    def components(self): return list(self)

    @property
    def probs(self): return np.full(len(self), 1.0 / len(self))

    def _live(self):
        if len(self) == 0:
            raise ValueError("MixtureModel without components")
        for c in self:
            c._live()

    def _engine_groups(self):
        """[(engine, [component indices])], engines in order of first appearance: multipathfinder's contiguous engine blocks"""
        groups = []
        for k, c in enumerate(self):
            for eng, ks in groups:
                if eng is c.engine:
                    ks.append(k)
                    break
            else:
                groups.append((c.engine, [k]))
        return groups

    def _lse(self, X, componentwise):
        self._live()
        X = np.asarray(X, dtype=np.float64)
        vec = X.ndim == 1
        X2 = np.asfortranarray(X.reshape(X.shape[0], -1, order="F"))
        lse, comp = None, (np.empty((X2.shape[1], len(self)), order="F") if componentwise else None)
        for eng, ks in self._engine_groups():
            r = eng.mixture_logpdf([self[k].point for k in ks], X2, componentwise=componentwise)
            part = r[0] if componentwise else r
            if componentwise:
                comp[:, ks] = r[1]
            lse = part if lse is None else np.logaddexp(lse, part)
        return lse, comp, vec

    def mean(self):
        self._live()
        return np.mean(np.stack([np.asarray(c.mu) for c in self]), axis=0)

    def logpdf(self, X):
        """log((1/K) sum_k pdf_k(x)) of each column of X (d, N); a vector x gives a number"""
        lse, _, vec = self._lse(X, False)
        out = lse - np.log(len(self))
        return float(out[0]) if vec else out

    def pdf(self, X):
        return np.exp(self.logpdf(X))

    def componentwise_logpdf(self, X):
        """(N, K): column k is logpdf(components[k], X) (Distributions.componentwise_logpdf); a vector x gives (K,)"""
        _, comp, vec = self._lse(X, True)
        return comp[0] if vec else comp

    def rand(self, rng, n):
        """(X (d, n), component_ids): ids = min(floor(K u), K - 1) + 1 for u = rng.rand(n) (1-based like the reference's
        draw_component_ids), then K draw seeds rng.rand_u64(K); the columns with id k + 1 are, in order, the draws of component
        k from its seed (the pool's draw kernel, Engine.draws)."""
        self._live()
        K = len(self)
        u = rng.rand(n)
        ids = np.minimum(np.floor(K * u).astype(np.int64), K - 1) + 1
        seeds = rng.rand_u64(K)
        X = np.empty((self[0].engine.d, n), order="F")
        for k, c in enumerate(self):
            cols = np.flatnonzero(ids == k + 1)
            if len(cols):
                X[:, cols] = c.engine.draws(c.point, int(seeds[k]), len(cols))[0]
        return X, ids


@dataclass
class ELBOEstimate:                 # src/elbo.jl:22-29
    value: float
    std_err: float
    engine: Any = field(repr=False, default=None)
    point: int = -1
    seed: int = 0
    ndraws: int = 0
    _cache: Any = field(repr=False, default=None)
    token: Any = field(repr=False, default=None)

    def _materialise(self):         # draws are regenerated on demand from the seed
        if self._cache is None:
            self.engine.check_token(self.token, "ELBOEstimate")
            self._cache = self.engine.draws(self.point, self.seed, self.ndraws)
        return self._cache

    @property
    def draws(self): return self._materialise()[0]
    @property
    def log_densities_target(self): return self._materialise()[1]
    @property
    def log_densities_fit(self): return self._materialise()[2]
    @property
    def log_density_ratios(self):
        x = self._materialise()
        return x[1] - x[2]

    def __str__(self):
        return f"ELBO estimate: {self.value:.2f} ± {self.std_err:.2f}"


@dataclass
class PSISResult:
    weights: np.ndarray
    log_weights: np.ndarray
    pareto_shape: float
    tail_length: int


@dataclass
class PathfinderResult:             # src/singlepath.jl:53-70
    input: Any
    rng: Any
    logp: Any
    fit_distribution: MvNormal
    draws_: Any = field(repr=False)     # (d, ndraws) array, or a thunk that downloads / regenerates it on first access
    fit_iteration: int = 0
    num_tries: int = 0
    optim_trace: Any = None
    fit_distributions: Any = None       # sequence of MvNormal
    elbo_estimates: Any = None          # sequence of ELBOEstimate
    num_bfgs_updates_rejected: int = 0
    success: bool = True
    draw_seed: int = 0
    ndraws_per_run: int = 0             # number of columns of `draws` (the stored candidates resample() reuses)

    @property
    def draws(self):
        if callable(self.draws_):
            self.draws_ = self.draws_()
        return self.draws_

    def __str__(self):                  # Base.show, src/singlepath.jl:72-83
        lines = ["Single-path Pathfinder result", f"  tries: {self.num_tries}", f"  draws: {self.draws.shape[1]}",
                 f"  fit iteration: {self.fit_iteration} (total: {len(self.optim_trace) - 1})"]
        if self.fit_iteration >= 1:
            lines.append(f"  fit ELBO: {str(self.elbo_estimates[self.fit_iteration - 1]).replace('ELBO estimate: ', '')}")
        lines.append(f"  fit distribution: MvNormal(dim = {self.draws.shape[0]}, Sigma = WoodburyPDMat)")
        return "\n".join(lines)

    @property
    def fit_distribution_transformed(self): return self.fit_distribution
    @property
    def draws_transformed(self): return self.draws


@dataclass
class MultiPathfinderResult:        # src/multipath.jl:31-44
    input: Any
    rng: Any
    logp: Any
    fit_distribution: List[MvNormal]        # MixtureModel: the list of the uniform mixture's components (src/multipath.jl:215-216)
    draws: np.ndarray
    draw_component_ids: np.ndarray          # 1-based like the reference
    pathfinder_results: List[PathfinderResult]
    psis_result: Optional[PSISResult]
    engine: Any = field(repr=False, default=None)
    ndraws_per_run: int = 0
    engines: Any = field(repr=False, default=None)      # the engines the runs are sharded over (contiguous blocks)
    proposal: str = "component"                         # what the PSIS weights divide logp by: the run's own fit, or the "mixture" of all
    pool_transform: Any = None                          # moment_match: the (scale, shift) every pooled candidate is moved by; None: as drawn
    moment_match_history: Any = None                    # moment_match: [(step name, k-hat, accepted), ...]

    @property
    def fit_distribution_transformed(self): return self.fit_distribution
    @property
    def draws_transformed(self): return self.draws

    def summary(self, importance=True):
        """importance-weighted posterior summaries from ALL pooled candidates, reduced on the device: importance_summary(self)"""
        return importance_summary(self, importance=importance)

    def quantiles(self, probs=(0.025, 0.25, 0.5, 0.75, 0.975), importance=True):
        """importance-weighted quantiles (len(probs), d) from ALL pooled candidates, searched on the device:
        importance_quantiles(self, probs)"""
        return importance_quantiles(self, probs, importance=importance)

    def covariance(self, importance=True):
        """importance-weighted posterior covariance (with mean and correlation) from ALL pooled candidates, reduced on the device:
        importance_covariance(self)"""
        return importance_covariance(self, importance=importance)

    def correlation(self, importance=True):
        """the (d, d) correlation matrix of covariance(): importance_covariance(self).corr"""
        return importance_covariance(self, importance=importance).corr

    def lowrank_covariance(self, rank, **kw):
        """the top `rank` eigenpairs of the importance-weighted posterior covariance plus its residual diagonal, the (d, d) matrix
        never formed: importance_lowrank_covariance(self, rank, **kw)"""
        return importance_lowrank_covariance(self, rank, **kw)

    def moment_match(self, **kw):
        """importance-weighted moment matching of the pooled candidates on the device: moment_match(self, **kw)"""
        return moment_match(self, **kw)

    def run_diagnostics(self, source="component"):
        """every run's own Pareto k-hat, effective sample size and evidence estimate -- which runs a bad pooled k-hat comes from --
        from one pass on the device over the pool: importance_run_diagnostics(self, source=source)"""
        return importance_run_diagnostics(self, source=source)

    def __str__(self):                  # Base.show, src/multipath.jl:46-65
        lines = ["Multi-path Pathfinder result", f"  runs: {len(self.pathfinder_results)}", f"  draws: {self.draws.shape[1]}"]
        if self.psis_result is not None:
            k = self.psis_result.pareto_shape
            assessment = "very bad" if k > 1 else "bad" if k > 0.7 else "ok" if k > 0.5 else "good"
            lines.append(f"  Pareto shape diagnostic: {round(k, 2)} ({assessment})")
        return "\n".join(lines)


# ---- helpers --------------------------------------------------------------------------------------------
_STATUS_MSG = {1: "A = diag(alpha) is not positive definite", 2: "C = I + R D R' is not positive definite",
               3: "non-finite factor"}


def _make_dist(eng, p, jeff, materialise=True):
    dist = MvNormal(None, None, eng, p, int(jeff[p]), eng.fit_token())
    return dist._materialise() if materialise else dist


def _make_dists(eng, p0, npts, status, jeff, materialise=True):
    if not materialise:                       # handles only: built on first access
        return _LazySeq(npts, lambda l: _make_dist(eng, p0 + l, jeff, False))
    return [_make_dist(eng, p0 + l, jeff, True) for l in range(npts)]


def fit_mvnormals(points, gradients, history_length=5, engine=None, eps=1e-12, Hinit="gilbert"):
    """fit_mvnormals(θs, ∇logpθs; history_length, Hinit, ϵ) -> (dists, num_bfgs_updates_rejected)
    reference src/mvnormal.jl:14-21 (keywords forwarded to lbfgs_inverse_hessians, src/inverse_hessian.jl:25).  Hinit: "gilbert" (the
    reference's default gilbert_init) or "nocedal_wright" ((α, s, y) -> fill(y's / y'y), test/inverse_hessian.jl:49).  Raises
    PosDefException like WoodburyPDMat's constructor."""
    eng = engine or Engine()
    eng.set_traces([np.asarray(points)], [np.asarray(gradients)])
    eng.fit_batch(history_length, eps, hinit=Hinit)
    status, jeff, _, nrej = eng.fit_status()
    bad = np.nonzero(status)[0]
    if len(bad):
        raise PosDefException(f"fit {int(bad[0])}: {_STATUS_MSG.get(int(status[bad[0]]), 'failed')}")
    return _make_dists(eng, 0, len(points), status, jeff), int(nrej[0])


def maximize_elbo(rng, target, dists, ndraws, ntasks=1):
    """maximize_elbo(rng, logp, dists, ndraws, ntasks) -> (iteration_opt, estimates)
    reference src/elbo.jl:1-10.  `dists` must be a contiguous slice of one fit_mvnormals result."""
    if len(dists) == 0:
        return 0, []                                        # src/elbo.jl:7
    eng = dists[0].engine
    seeds_l = rng.rand_u64(len(dists))                      # src/elbo.jl:2
    seeds = np.zeros(eng.P, dtype=np.uint64)
    for dist, s in zip(dists, seeds_l):
        seeds[dist.point] = s
    eng.set_target(target)
    eng.set_callback_threads(ntasks)                        # src/elbo.jl:3-6: logp over `ntasks` tasks (host closures; no-op for device targets)
    elbo, se, _ = eng.elbo_batch(ndraws, seeds)
    ests = [ELBOEstimate(float(elbo[d.point]), float(se[d.point]), eng, d.point, int(seeds[d.point]), ndraws,
                         token=eng.fit_token()) for d in dists]
    return _findmax_skipnan([e.value for e in ests])[1], ests


def _findmax_skipnan(xs):
    """reference src/utils.jl:55-72 (1-based index)"""
    state = None
    for i, xi in enumerate(xs, 1):
        if state is None:
            state = (xi, i)
            continue
        if np.isnan(xi):
            continue
        if np.isnan(state[0]) or xi > state[0]:
            state = (xi, i)
    return state


class UniformSampler:               # src/singlepath.jl:332-344
    def __init__(self, scale):
        if not scale > 0:
            raise ValueError("scale of uniform sampler must be positive.")   # DomainError
        self.scale = scale

    def __call__(self, rng, point):
        point[:] = rng.rand(len(point)) * 2 * self.scale - self.scale
        return point


class DeviceOptimizationTrace:
    """OptimizationTrace (src/optimize.jl:94-100) of a path optimised on the device; the arrays are downloaded on
    first access (valid while the engine still holds this batch of traces)."""

    def __init__(self, engine, k, n):
        self._eng, self._k, self._n, self._cache = engine, k, n, None
        self._token = engine.trace_token()

    def __len__(self):
        return self._n

    def materialise(self):
        if self._cache is None:
            self._eng.check_token(self._token, "DeviceOptimizationTrace")
            self._cache = self._eng.get_trace(self._k)
        return self

    @property
    def points(self): return self.materialise()._cache[0]
    @property
    def log_densities(self): return self.materialise()._cache[1]
    @property
    def gradients(self): return self.materialise()._cache[2]


def _closure_gradient(target):
    """a device closure target that carries a value-and-gradient closure (pfmi_set_target_gradient)"""
    return getattr(target, "kind", 2) == 3 and getattr(target, "has_device_gradient", False)


def _use_device_optimizer(target, optimizer, history_length=DEFAULT_HISTORY_LENGTH):
    builtin = getattr(target, "kind", 2) in (0, 1)
    if _closure_gradient(target) and optimizer in ("auto", "device"):  # rounds of the closure L-BFGS: any d, the fit path's J limit
        if history_length > 32:
            if optimizer == "device":
                raise ValueError("optimizer='device' with a gradient closure needs history_length <= 32")
            return False
        return True
    if optimizer == "device" and not builtin:
        raise ValueError("optimizer='device' needs a built-in target (analytic gradient on the GPU) or a device closure with a gradient")
    if optimizer == "auto":                                  # the device L-BFGS keeps a path's vectors in registers (d <= 16 384) and its
        return builtin and getattr(target, "d", 0) <= 16384 and history_length <= 16      # ring in LDS / a scratch of 16 pairs
    return optimizer == "device"


def _use_stream(target, on_device, history_length=DEFAULT_HISTORY_LENGTH):
    """the streaming pipeline (pfmi_stream_enqueue: fits and ELBO scans while the paths are still being optimised) for a run that optimises
    on the device: built-in targets and device closures with a gradient, history_length <= 16 (the pipeline pads to 32 columns), unless
    PFMI_NO_STREAM=1.  (A shape the library cannot stream is refused with -4 and takes the packed route.)"""
    if not on_device or history_length > 16 or os.environ.get("PFMI_NO_STREAM") == "1":
        return False
    return getattr(target, "kind", 2) in (0, 1) or _closure_gradient(target)


# ---- batched driver shared by pathfinder / multipathfinder ------------------------------------------------
def _comm_for(engs):
    """the pfmi_comm joining `engs` (cached on the first engine; a single engine forms a world of one without RCCL)"""
    from .core import Comm
    key = tuple(id(e) for e in engs)
    cache = engs[0].__dict__.setdefault("_comm_cache", {})
    if key not in cache or cache[key].h is None:
        cache[key] = Comm.init_all(engs)
    return cache[key]


def _blocks(K, G):
    """contiguous blocks of paths, one per engine, the first K % G one path longer (pool order stays k-major, src/resample.jl:93; any
    nruns over any number of engines, like the reference's nruns over ntasks, src/multipath.jl:131-146, 190-208)"""
    if K < G:
        raise ValueError(f"nruns={K} is smaller than the number of engines {G}: every engine needs at least one run")
    base, rem = divmod(K, G)
    out, k0 = [], 0
    for g in range(G):
        k1 = k0 + base + (1 if g < rem else 0)
        out.append((k0, k1))
        k0 = k1
    return out


def _run_paths(engs, target, inits, run_rngs, *, dim, history_length, ndraws_elbo, ntries, init_sampler,
               optimizer_kwargs, materialise, optimizer="auto", strict=True, pool=None):
    """Runs every path to success (or ntries), batching the GPU work over the engines (contiguous blocks of paths, one engine per
    GPU, driven by THIS host thread: every stage is enqueued on all engines before the first wait).  Returns per-path dicts.
    The K optimisations run on the device for built-in targets (pfmi_optimize_batch, all paths of an engine in one launch) and
    through the host driver for callback targets (the reference's general case, src/optimize.jl:35-59).
    pool = dict(N_r, ndraws, importance, replace, seed): the pooled stage (winners picked on the device, pool, PSIS, index selection,
    gather) is enqueued right behind the ELBO scan -- no host round trip in between; its result is valid when no path needed a retry
    and is recomputed with the retry otherwise."""
    K = len(inits)
    G = len(engs)
    blocks = _blocks(K, G)
    state = [dict(itry=0, done=False) for _ in range(K)]
    for g, (k0, k1) in enumerate(blocks):
        for k in range(k0, k1):
            state[k].update(eng=engs[g], g=g, kl=k - k0)
    pending = list(range(K))
    on_device = _use_device_optimizer(target, optimizer, history_length)
    closure_opt = on_device and _closure_gradient(target)
    stream_ok = _use_stream(target, on_device, history_length)
    okw = {k: v for k, v in optimizer_kwargs.items() if k in ("maxiters", "g_tol")}
    pooled = None
    while pending:
        pooled_error = None
        tables = None                                               # per engine: (fit_status, elbo_batch_wait, psis_weights) delivered by the pooled wait
        need = []
        for k in pending:
            st = state[k]
            st["itry"] += 1
            if st["itry"] == 1 and inits[k] is not None:
                st["x0"] = np.array(inits[k], dtype=np.float64)
            else:
                need.append(k)
        if need and type(init_sampler) is UniformSampler:          # src/singlepath.jl:167-168, 277 -- all runs in one Philox batch
            u = np.stack(rand_u64_multi([run_rngs[k] for k in need], [dim] * len(need)))
            x0s = ((u >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)) * 2 * init_sampler.scale - init_sampler.scale
            for i, k in enumerate(need):
                state[k]["x0"] = x0s[i]
        else:
            for k in need:
                state[k]["x0"] = init_sampler(run_rngs[k], np.empty(dim))
        predrawn = None
        streamed = False
        if on_device and stream_ok:
            # ONE dataflow per engine (pfmi_stream_enqueue): the fits and ELBO scans of the trace points a path has already produced run
            # while the paths are still being optimised.  The per-fit seeds of every run for the LONGEST possible trace are drawn up front
            # from copies of the runs' rngs (a run that was finished in an earlier try keeps the stream it had).
            cap = int(okw.get("maxiters", 1000)) + 1
            try:
                for eng, (k0, k1) in zip(engs, blocks):             # the optimiser starts at once; the seed streams follow while it runs
                    eng.stream_enqueue(np.stack([s["x0"] for s in state[k0:k1]]), ndraws_elbo, None, history_length, **okw)
                streamed = True
            except PfmiError as ex:
                for e2 in engs:                                     # engines enqueued before the refusal / failure are released
                    e2.stream_cancel()
                if getattr(ex, "code", 0) != -4:                    # PFMI_ERR_UNSUPPORTED: the packed route below (on every engine)
                    raise
                stream_ok = False
            except BaseException:
                for e2 in engs:                                     #  an engine enqueued before the failure must not stay "active":
                    e2.stream_cancel()                              # a caller's persistent Engine has to survive a failed call
                raise
        if streamed:
            try:
                for k, sd in zip(pending, rand_u64_multi([run_rngs[k].copy() for k in pending], [cap] * len(pending))):
                    state[k]["stream_tab"] = sd
                predrawn = {k: state[k]["stream_tab"] for k in pending}
                for eng, (k0, k1) in zip(engs, blocks):
                    eng.stream_seeds(np.concatenate([s["stream_tab"] for s in state[k0:k1]]))
                active = list(zip(engs, blocks))
                gc_was_on = gc.isenabled()
                gc.disable()                # this thread IS the pipeline's scheduler for the next millisecond or two: a full collection (tens of
                try:                        # milliseconds) in here would starve every GPU it drives (profiles/r05_experiments.md section 5)
                    while active:                                   # the calling thread schedules every engine's pipeline
                        active = [(eng, b) for eng, b in active if not eng.stream_pump()]
                finally:
                    if gc_was_on:
                        gc.enable()
                for eng, (k0, k1) in zip(engs, blocks):
                    npts = eng.stream_wait()
                    for k in range(k0, k1):
                        state[k]["trace"] = DeviceOptimizationTrace(eng, k - k0, int(npts[k - k0]))
                        if materialise:
                            state[k]["trace"].materialise()
            except BaseException:           # KeyboardInterrupt while pumping, a failure in the seed draw, an engine's pump error: no engine
                for e2 in engs:             # may be left with a streaming call outstanding
                    try:
                        e2.stream_cancel()
                    except Exception:
                        pass
                raise
        elif on_device:     # every path in one launch per engine; finished paths are recomputed identically from their x0
            for eng, (k0, k1) in zip(engs, blocks):
                eng.optimize_batch_enqueue(np.stack([s["x0"] for s in state[k0:k1]]), history_length, **okw)
            if closure_opt:
                # the rounds of every engine are pumped in turn by this thread (each pump calls the closure for the rounds it launches);
                # a closure that raised cancels every engine's call, and the exception propagates with the engines usable again
                try:
                    active = list(engs)
                    while active:
                        active = [eng for eng in active if not eng.optimize_batch_pump()]
                except BaseException:
                    for e2 in engs:
                        try:
                            e2.optimize_batch_cancel()
                        except Exception:
                            pass
                    raise
            # while the optimisations run: the per-fit seeds of every pending run for the LONGEST possible trace, drawn from copies of
            # the runs' rngs (counter-based: the real rng is advanced by L_k once L_k is known, so the stream consumption is the
            # reference's: rand!(rng_k, UInt64[L_k]), src/elbo.jl:2)
            cap = int(okw.get("maxiters", 1000)) + 1
            predrawn = dict(zip(pending, rand_u64_multi([run_rngs[k].copy() for k in pending], [cap] * len(pending))))
            for eng, (k0, k1) in zip(engs, blocks):
                npts = eng.optimize_batch_wait()
                for k in range(k0, k1):
                    state[k]["trace"] = DeviceOptimizationTrace(eng, k - k0, int(npts[k - k0]))
                    if materialise:
                        state[k]["trace"].materialise()
        else:
            for k in pending:
                state[k]["trace"] = optimize_with_trace(target, state[k]["x0"], history_length=history_length, **optimizer_kwargs)
            for eng, (k0, k1) in zip(engs, blocks):
                eng.set_traces([s["trace"].points for s in state[k0:k1]], [s["trace"].gradients for s in state[k0:k1]])
        # one batched fit + ELBO over every path (finished paths are recomputed identically from their seeds).  fit_batch only
        # ENQUEUES the history walk and the fits; the per-fit seeds are drawn on the host while they run
        if not streamed:
            for eng in engs:
                eng.fit_batch(history_length)
        if predrawn is not None:
            for k in pending:
                L = len(state[k]["trace"]) - 1
                state[k]["seeds"] = np.concatenate([[np.uint64(0)], predrawn[k][:L]]).astype(np.uint64)
                state[k]["fail_seed"] = np.uint64(predrawn[k][L])     # the value the rng would produce next (see below)
                run_rngs[k].counter += L
        else:
            fresh = rand_u64_multi([run_rngs[k] for k in pending], [len(state[k]["trace"]) - 1 for k in pending])
            for k, sd in zip(pending, fresh):                       # seeds = rand!(rng_k, UInt64[L_k])  (src/elbo.jl:2)
                state[k]["seeds"] = np.concatenate([[np.uint64(0)], sd]).astype(np.uint64)
                # what rand(rng_k, fit_distribution, ndraws) would use if this try ends in failure (src/singlepath.jl:231-233): peeked
                # from a copy, the run's rng only advances when the path really fails (_assemble_path)
                state[k]["fail_seed"] = np.uint64(run_rngs[k].copy().rand_u64(1)[0])
        if not streamed:
            for eng, (k0, k1) in zip(engs, blocks):
                eng.elbo_batch_enqueue(ndraws_elbo, np.concatenate([s["seeds"] for s in state[k0:k1]]))
        if pool is not None:                                        # optimistic: right behind the scan, no host round trip
            for eng, (k0, k1) in zip(engs, blocks):
                eng.pool_build_best(pool["N_r"], np.array([s["fail_seed"] for s in state[k0:k1]], dtype=np.uint64))
            comm = _comm_for(engs)
            # the pooled stage is ENQUEUED; the tables of this try (fit statuses, ELBO table, PSIS weights) are queued behind it and the one
            # wait below delivers everything: a single host round trip per try
            try:
                comm.psis_resample_enqueue(pool["ndraws"], importance=pool["importance"], replace=pool.get("replace", True), seed=pool["seed"])
                queued = []
                try:
                    for eng in engs:
                        eng.defer(1)
                    for g, eng in enumerate(engs):
                        queued.append((eng.fit_status(), eng.elbo_batch_wait(),
                                       eng.psis_weights(len(inits) * pool["N_r"]) if (g == 0 and pool["importance"]) else None))
                except BaseException:
                    for eng in engs:
                        eng.defer(-1)                               # nothing queued may be delivered into arrays that are going away
                    raise
                for eng in engs:
                    eng.defer(0)
            except PfmiRetry:
                raise
            except Exception as ex:                                 # surfaced AFTER the fit statuses: the reference would have thrown
                pooled_error = ex                                   # PosDefException from fit_mvnormals before it ever pooled
            else:
                try:
                    res, idx, draws = comm.psis_resample_wait()
                    pooled = dict(psis=res, idx=idx, draws=draws, comm=comm, weights=queued[0][2])
                    tables = queued
                except PfmiRetry:
                    for eng in engs:
                        eng.defer(-1)
                    raise
                except Exception as ex:
                    pooled_error = ex
                    try:                                            # whatever the failed wait did not deliver
                        for eng in engs:
                            eng.sync()
                        tables = queued
                    except PfmiRetry:
                        raise
                    except Exception:
                        for eng in engs:
                            eng.defer(-1)
        # ---- first wait of this try: everything above is in flight on every engine
        new_pending = []
        all_status, all_jeff = [], []
        for g, (eng, (k0, k1)) in enumerate(zip(engs, blocks)):
            status, jeff, logdet, nrej = tables[g][0] if tables is not None else eng.fit_status()
            all_status.append(status); all_jeff.append(jeff)
            bad = np.flatnonzero((status != 0) & (status != 4))      # (4 = PFMI_FIT_ABSENT: a slot of the streaming layout no path reached)
            if len(bad) and strict:
                # WoodburyPDMat's constructor throws inside fit_mvnormals (src/woodbury.jl:202,205) and nothing in
                # _pathfinder / the retry loop catches it (src/singlepath.jl:259-314): the reference's call fails as a whole
                p = int(bad[0])
                kl = int(np.searchsorted(eng.offsets, p, side="right") - 1)
                raise PosDefException(f"run {k0 + kl + 1}, fit {p - int(eng.offsets[kl]) + 1}: {_STATUS_MSG.get(int(status[p]), 'failed')} "
                                      f"({len(bad)} of {len(status)} fits failed; strict=False keeps them as NaN ELBOs instead)")
            elbo, se, best = tables[g][1] if tables is not None else eng.elbo_batch_wait()
            for k in range(k0, k1):
                st = state[k]
                kl = k - k0
                p0 = int(eng.offsets[kl])
                p1 = p0 + eng.path_len(kl)
                L = p1 - p0 - 1
                fit_it = int(best[kl])
                ok = L > 0                                           # src/singlepath.jl:299
                if fit_it > 0:
                    v = elbo[p0 + fit_it]
                    ok = ok and (not np.isnan(v)) and v != -np.inf   # :309-314
                else:
                    ok = False
                st.update(p0=p0, L=L, fit_iteration=fit_it, success=ok, status=status[p0:p1], jeff=jeff[p0:p1],
                          elbo=elbo[p0:p1], se=se[p0:p1], nrej=int(nrej[kl]), status_all=status, jeff_all=jeff)
                if not ok and st["itry"] < ntries and not st["done"]:
                    new_pending.append(k)
                else:
                    st["done"] = True
        if new_pending:
            # some run failed this try and is retried (src/singlepath.jl:259-283: the reference retries every run up to `ntries`
            # BEFORE it ever pools): the optimistic pooled stage above ran on that failed try's draws -- whatever it returned or
            # raised (e.g. "weights are all zero" when every run's ELBO was NaN) is stale; the retry iteration recomputes it
            pooled, pooled_error = None, None
        elif pooled_error is not None:                              # no retry pending: the pooled stage's failure is the call's failure
            raise pooled_error
        pending = new_pending
    return state, pooled


def _assemble_path(st, rng, ndraws_elbo, materialise, warn=True):
    eng = st["eng"]
    p0, L = st["p0"], st["L"]
    if not st["success"] and warn:
        warnings.warn(f"Pathfinder failed after {st['itry']} tries. Increase `ntries`, inspect the model for "
                      "numerical instability, or provide a more suitable `init_sampler`.")
    if st["nrej"] > 0 and warn:
        perc = round(st["nrej"] * 100 / (L + 1), 1)
        warnings.warn(f"{st['nrej']} ({perc}%) updates to the inverse Hessian estimate were rejected to keep it "
                      "positive definite.")
    dists = _make_dists(eng, p0, L + 1, st["status_all"], st["jeff_all"], materialise)
    tok = eng.fit_token()

    def _est(i, st=st):
        l = i + 1
        return ELBOEstimate(float(st["elbo"][l]), float(st["se"][l]), eng, p0 + l, int(st["seeds"][l]), ndraws_elbo,
                            token=tok)

    ests = _LazySeq(L, _est) if not materialise else [_est(i) for i in range(L)]
    fit_it = st["fit_iteration"]
    fit_point = p0 + fit_it                                       # fit_distributions[fit_iteration + 1]
    if st["success"]:
        draw_seed = int(st["seeds"][fit_it])                      # reuse the ELBO draws, top up if needed
    else:
        draw_seed = int(rng.rand_u64(1)[0])                       # rand(rng, fit_distribution, ndraws)
        assert draw_seed == int(st["fail_seed"])                  # what pfmi_pool_build_best was given for this path
    return dict(dists=dists, ests=ests, fit_point=fit_point, draw_seed=draw_seed)


def pathfinder(target, *, rng=None, init=None, dim=-1, init_scale=2, init_sampler=None, input=None,
               history_length=DEFAULT_HISTORY_LENGTH, ndraws_elbo=DEFAULT_NDRAWS_ELBO, ndraws=None, ntries=1000,
               ntasks=1, engine=None, materialise=True, optimizer="auto", strict=True, **optimizer_kwargs):
    """Single-path Pathfinder (reference src/singlepath.jl:142-257).  optimizer: "auto" (device L-BFGS for built-in
    targets, host driver for callbacks), "device" or "host".  strict: a non-positive-definite fit raises PosDefException like
    the reference (src/woodbury.jl:202,205); strict=False keeps the library's per-fit status / NaN-ELBO behaviour."""
    rng = rng if rng is not None else HostRNG(0)
    ndraws = ndraws_elbo if ndraws is None else ndraws
    init_sampler = init_sampler or UniformSampler(init_scale)
    if init is None:
        if dim <= 0:
            dim = getattr(target, "d", -1)
        if dim <= 0:
            raise ValueError("An initial point `init` or dimension `dim` must be provided.")   # :171
    else:
        dim = len(init)
    eng = engine or Engine()
    eng.set_target(target)
    eng.set_callback_threads(ntasks)                        # `ntasks` (src/singlepath.jl:114-117 -> src/elbo.jl:3-6): a host closure is called from ntasks threads
    rng_state = (rng.seed, rng.counter) if isinstance(rng, HostRNG) else None
    for attempt in range(_RETRIES + 1):
        try:
            state, _ = _run_paths([eng], target, [init], [rng], dim=dim, history_length=history_length,
                                  ndraws_elbo=ndraws_elbo, ntries=ntries, init_sampler=init_sampler,
                                  optimizer_kwargs=optimizer_kwargs, materialise=materialise, optimizer=optimizer, strict=strict)
            break
        except PfmiRetry:       # transient (GPU shared / dispatch serialised): the library switched to its wait-free route; same seeds again
            if attempt == _RETRIES or rng_state is None:
                raise
            rng.seed, rng.counter = rng_state
    st = state[0]
    a = _assemble_path(st, rng, ndraws_elbo, materialise)
    X = eng.draws(a["fit_point"], a["draw_seed"], ndraws)[0]     # src/singlepath.jl:226-233
    return PathfinderResult(input if input is not None else target, rng, target.logp,
                            a["dists"][st["fit_iteration"]], X, st["fit_iteration"], st["itry"], st["trace"],
                            a["dists"], a["ests"], st["nrej"], st["success"], a["draw_seed"], ndraws)


PROPOSALS = ("component", "mixture")


def _check_proposal(proposal, importance, engs):
    """The `proposal` keyword of multipathfinder / resample.  "component": every candidate is weighted by p / q_k of the run that drew
    it (the reference, src/resample.jl:81-95).  "mixture": by p / qbar with qbar the uniform mixture of all runs' fits, which needs
    every run's factor on the GPU that holds the candidate -- one engine, no communicator across processes."""
    if proposal not in PROPOSALS:
        raise ValueError(f"proposal must be one of {PROPOSALS}, got {proposal!r}")
    if proposal == "mixture":
        if not importance:
            raise ValueError('proposal="mixture" chooses the importance weights: it needs importance=True')
        if len(engs) > 1:
            raise ValueError('proposal="mixture" is limited to one engine: the mixture needs every run\'s fit on the GPU that holds '
                             "the candidate")
        from .core import _LIVE_COMMS
        for comm in list(_LIVE_COMMS):
            if comm.h is not None and engs[0] in comm.engines and comm.info()["world"] > 1:
                raise ValueError('proposal="mixture" is limited to one engine: this engine belongs to a communicator of several ranks')
    return proposal


def _mixture_pool_psis(eng, npr, points, seeds, want_weights=True, moved=None):
    """pool of the runs' fits `points` drawn with `seeds`, its mixture-proposal log ratios and their PSIS, all on the device of `eng`
    (the weights stay there for the index selection and the pool passes); returns the PSIS result.  moved: the (scale, shift) of a
    moment-matched result, applied to the pool once the ratios of the pool as built exist."""
    eng.pool_build(npr, points, seeds)
    eng.pool_mixture_ratios(want=False)
    if moved is not None:
        eng.pool_transform(moved[0], moved[1], want=False)
    ptr, S = eng.pool_mixture_ratios_dev()
    return eng.psis_dev(ptr, S, want_weights=want_weights)


def _mixture_pooled_stage(eng, npr, points, seeds, ndraws, seed, replace=True, moved=None):
    """the pooled stage under the mixture proposal: (PSIS result, indices, draws)"""
    res = _mixture_pool_psis(eng, npr, points, seeds, moved=moved)
    idx = eng.resample_indices(len(points) * npr, ndraws, importance=True, replace=replace, seed=seed)
    return res, idx, eng.pool_gather(idx)


def multipathfinder(target, ndraws, *, init=None, nruns=-1, ndraws_elbo=DEFAULT_NDRAWS_ELBO, ndraws_per_run=None,
                    rng=None, history_length=DEFAULT_HISTORY_LENGTH, importance=True, dim=-1, init_scale=2,
                    init_sampler=None, ntries=1000, ntasks=1, ntasks_per_run=1, input=None, engine=None, engines=None,
                    materialise=False, optimizer="auto", strict=True, proposal="component", **optimizer_kwargs):
    """Multi-path Pathfinder (reference src/multipath.jl:118-245).  optimizer, strict: see pathfinder().
    proposal="mixture": the pooled candidates are weighted by p / qbar, qbar the uniform mixture of the runs' fits (fit_distribution),
    instead of p / q_k of the run that drew them -- the deterministic-mixture weights of multiple importance sampling; one engine only.
    engines=[Engine(0), Engine(1), ...]: the runs are sharded in contiguous blocks over several GPUs driven by this one host thread
    (the reference fans them out over tasks, src/multipath.jl:190-208); the pooled stage (:215-225) goes through the RCCL group of
    the engines.  The result does not depend on the number of engines (test/multipath.jl:107-140 extended to GPUs)."""
    _check_proposal(proposal, importance, list(engines) if engines else [engine])
    if init is None:
        if nruns <= 0:
            raise ValueError("A positive `nruns` must be set or `init` must be provided.")     # :148-150
        inits = [None] * nruns
    else:
        inits = list(init)
    nruns = len(inits)
    if ndraws_per_run is None:
        ndraws_per_run = max(ndraws_elbo, -(-ndraws // max(nruns, 1)))                          # :138
    if ndraws > ndraws_per_run * nruns:
        warnings.warn("More draws requested than total number of draws across replicas. Draws will not be unique.")
    rng = rng if rng is not None else HostRNG(0)
    init_sampler = init_sampler or UniformSampler(init_scale)
    if dim <= 0:
        dim = getattr(target, "d", -1) if inits[0] is None else len(inits[0])
    run_seeds = rng.rand_u64(nruns)                                                             # :162
    run_rngs = [rng.copy().seed_(int(s)) for s in run_seeds]                                    # :189-193
    engs = list(engines) if engines else [engine or Engine()]
    for e in engs:
        e.set_target(target)
        # the reference spreads the runs over `ntasks` tasks and each run's logp evaluations over `ntasks_per_run` (src/multipath.jl:104-108,
        # 190-208); here the runs of an engine are ONE batch, so a host closure sees ntasks * ntasks_per_run threads per staged block
        e.set_callback_threads(max(1, int(ntasks)) * max(1, int(ntasks_per_run)))
    resample_seed = int(rng.rand_u64(1)[0])                                                     # _resample's draw from the top-level rng (:225)
    # draws_per_component = stack(draws) (:217), _compute_psis_result (:221), _resample (:225): enqueued behind the ELBO scan
    for attempt in range(_RETRIES + 1):
        try:
            state, pooled = _run_paths(engs, target, inits, run_rngs, dim=dim, history_length=history_length,
                                       ndraws_elbo=ndraws_elbo, ntries=ntries, init_sampler=init_sampler,
                                       optimizer_kwargs=optimizer_kwargs, materialise=materialise, optimizer=optimizer, strict=strict,
                                       pool=dict(N_r=ndraws_per_run, ndraws=ndraws, importance=importance, seed=resample_seed))
            break
        except PfmiRetry:       # transient (GPU shared / dispatch serialised): every run again from its own seed, the same answer
            if attempt == _RETRIES:
                raise
            run_rngs = [rng.copy().seed_(int(s)) for s in run_seeds]
    parts = [_assemble_path(st, r, ndraws_elbo, materialise) for st, r in zip(state, run_rngs)]
    # the per-run draws (d, N_r, K) stay on the device.  A run's block is a pure function of (fit, draw_seed, N_r): when it is
    # looked at it is REGENERATED from the seed (bit-identical to the pool block, tests: pool == eng.draws), so the handle
    # does not depend on what a later resample() put into the pool; it does depend on the fits, hence the token.
    results = []

    def _run_draws(eng, tok, fit_point, seed):
        eng.check_token(tok, "PathfinderResult.draws")
        return eng.draws(fit_point, seed, ndraws_per_run)[0]

    for k, (st, a) in enumerate(zip(state, parts)):
        eng = st["eng"]
        thunk = (lambda eng=eng, tok=eng.fit_token(), a=a: _run_draws(eng, tok, a["fit_point"], a["draw_seed"]))
        results.append(PathfinderResult(input if input is not None else target, run_rngs[k], target.logp,
                                        a["dists"][st["fit_iteration"]], thunk, st["fit_iteration"],
                                        st["itry"], st["trace"], a["dists"], a["ests"], st["nrej"], st["success"],
                                        a["draw_seed"], ndraws_per_run))
        if materialise:
            results[-1].draws
    S = nruns * ndraws_per_run
    psis_result = None
    if proposal == "mixture":       # the runs are final: the pooled stage again, every candidate weighted against the mixture of the winners
        res, idx, draws = _mixture_pooled_stage(engs[0], ndraws_per_run, [r.fit_distribution.point for r in results],
                                                [r.draw_seed for r in results], ndraws, resample_seed)
        pooled = dict(psis=res, idx=idx, draws=draws, weights=(res["weights"], res["log_weights"]))
    if importance:                                                                               # :220-224
        w, lw = pooled["weights"] if pooled.get("weights") is not None else engs[0].psis_weights(S)
        psis_result = PSISResult(w, lw, pooled["psis"]["pareto_shape"], pooled["psis"]["tail_length"])
    ids = pooled["idx"] // ndraws_per_run + 1                                                   # cld.(inds, N) with 1-based inds
    return MultiPathfinderResult(input if input is not None else target, rng, target.logp,
                                 MixtureModel([r.fit_distribution for r in results]), pooled["draws"], ids, results, psis_result, engs[0],
                                 ndraws_per_run, engs, proposal)


@dataclass
class ImportanceSummary:
    """Posterior summaries from the S = nruns * ndraws_per_run pooled candidates under their PSIS weights (importance_summary)."""
    mean: np.ndarray                # (d,) sum w x / W
    var: np.ndarray                 # (d,) sum w (x - mean)^2 / W
    std: np.ndarray                 # (d,) sqrt(var)
    mcse_mean: np.ndarray           # (d,) sqrt(sum w^2 (x - mean)^2) / W: Monte Carlo standard error of `mean`
    ess: float                      # W^2 / sum w^2
    run_weights: np.ndarray         # (nruns,) share of the mass each run carries
    ncandidates: int                # S
    pareto_shape: float             # k-hat of the pooled PSIS (NaN for uniform weights)


def _combine_moments(blocks):
    """Totals over runs of per-run arrays that arrive in blocks (one per engine, in global run order): the blocks are concatenated
    along the run axis and the rows added one by one in that order.  Only this function adds across runs, so the totals do not
    depend on how the runs are split into blocks."""
    rows = np.concatenate([np.asarray(b, dtype=np.float64) for b in blocks], axis=0)
    total = np.zeros(rows.shape[1:], dtype=np.float64)
    for row in rows:
        total = total + row
    return total


def _rebuild_pool(result, importance, mixture_ratios=False):
    """The preamble of the pooled summaries: every engine of `result` rebuilds its block of the pool from the runs' stored
    (fit, draw_seed, ndraws_per_run) and, with importance weighting, the pooled PSIS is re-run so that every engine holds the weights
    of the global pool.  Returns (owners, weighted, pareto_shape); owners: one (engine, col_offset) per engine in global run order,
    col_offset the global pool column of the engine's first draw.  mixture_ratios: every engine also forms the mixture-proposal
    ratios of its pool (Engine.pool_mixture_ratios) -- on the pool AS BUILT, before a moment-matched result's map is applied, which
    then carries them along (a moved pool's mixture ratios follow from those of the pool as built and are not formed afresh)."""
    engs = result.engines or [result.engine]
    runs = result.pathfinder_results
    for r in runs:
        r.fit_distribution._live()                                  # the fits must still be the engine's current ones
    npr = runs[0].ndraws_per_run
    seeds = [r.draw_seed for r in runs]
    moved = getattr(result, "pool_transform", None)                 # a moment-matched result: its map follows every rebuild
    if getattr(result, "proposal", "component") == "mixture" and bool(importance) and result.psis_result is not None:
        _check_proposal("mixture", True, engs)                      # the weights of the mixture route, as multipathfinder formed them
        res = _mixture_pool_psis(engs[0], npr, [r.fit_distribution.point for r in runs], seeds, want_weights=False, moved=moved)
        return [(engs[0], 0)], True, res["pareto_shape"]
    owners = []
    for eng, (k0, k1) in zip(engs, _blocks(len(runs), len(engs))):
        eng.pool_build(npr, [r.fit_distribution.point for r in runs[k0:k1]], seeds[k0:k1])
        if mixture_ratios:
            eng.pool_mixture_ratios(want=False)
        if moved is not None:
            eng.pool_transform(moved[0], moved[1], want=False)
        owners.append((eng, k0 * npr))
    weighted = bool(importance) and result.psis_result is not None
    pareto_shape = float("nan")
    if weighted:                                                    # weights of the rebuilt pool, replicated on every engine
        pareto_shape = _comm_for(engs).pool_psis()["pareto_shape"]
    return owners, weighted, pareto_shape


def _moment_pass(owners, weighted, center):
    """Engine.pool_moments of every owner about `center`: (wsum, s1, s2, s2w), each a list with one block of runs per engine"""
    parts = [eng.pool_moments(off, weighted, center) for eng, off in owners]
    return [[p[j] for p in parts] for j in range(4)]


def _first_moments(owners, weighted, want_mean=True):
    """The moment pass about the origin: (wsum blocks, wtot = (sum w, sum w^2) over all runs, W = sum w, mean = sum w x / W -- None
    when it is not wanted)"""
    wsum_b, s1_b, _, _ = _moment_pass(owners, weighted, None)
    wtot = _combine_moments(wsum_b)
    return wsum_b, wtot, wtot[0], (_combine_moments(s1_b) / wtot[0] if want_mean else None)


def importance_summary(result, *, importance=True):
    """Importance-weighted posterior mean, variance, Monte Carlo standard error, effective sample size and per-run mass from ALL
    candidates of a multipathfinder result -- not from the resampled `result.draws`, which only add resampling noise to the
    estimator the PSIS weights already define.  The pool stays on the device: every engine of `result.engines` rebuilds its block of
    the pool from the runs' stored (fit, draw_seed, ndraws_per_run) exactly as resample() does for stored draws, the pooled PSIS is
    re-run, and two moment passes (Engine.pool_moments: about the origin, then about the mean) return 3 d numbers per run.  Across
    runs only the host adds, in run order, so the summary is bit-identical for any number of engines.  importance=False, or a
    result without psis_result: uniform weights.  Raises StaleHandleError when the engines hold newer fits."""
    owners, weighted, pareto_shape = _rebuild_pool(result, importance)
    wsum_b, wtot, W, mean = _first_moments(owners, weighted)
    _, c1_b, c2_b, c2w_b = _moment_pass(owners, weighted, mean)
    var = _combine_moments(c2_b) / W - (_combine_moments(c1_b) / W) ** 2
    mcse = np.sqrt(_combine_moments(c2w_b)) / W
    run_weights = np.concatenate([b[:, 0] for b in wsum_b]) / W
    S = len(result.pathfinder_results) * result.pathfinder_results[0].ndraws_per_run
    return ImportanceSummary(mean, var, np.sqrt(var), mcse, float(W * W / wtot[1]), run_weights, S, pareto_shape)


@dataclass
class RunDiagnostics:
    """PSIS of every run of a multipathfinder result on the run's own ndraws_per_run candidates (importance_run_diagnostics); every
    field has one entry per run, in run order."""
    pareto_shape: np.ndarray        # k-hat of the run's own log ratios; NaN where PSIS does not smooth (fewer than 25 candidates, a non-finite tail)
    tail_length: np.ndarray         # M = min(cld(N_r, 5), ceil(3 sqrt(N_r)))
    ess: np.ndarray                 # 1 / sum w^2 of the run's own normalised, smoothed weights
    log_evidence: np.ndarray        # logsumexp of the run's smoothed log ratios - log N_r: log Z estimated from this run alone
    elbo: np.ndarray                # the ELBO estimate of the run's chosen fit; NaN when fit_iteration == 0
    success: np.ndarray             # the run's success flag (bool)
    ndraws_per_run: int             # N_r

    def ok(self, threshold=0.7):
        """mask of the runs whose k-hat is at most `threshold` (False where k-hat is NaN)"""
        return _run_ok(self.pareto_shape, threshold)


def _run_ok(pareto_shape, threshold=0.7):
    with np.errstate(invalid="ignore"):
        return np.asarray(pareto_shape, dtype=np.float64) <= threshold       # (NaN <= x is False)


def _run_diagnostics_host(pareto_shape, tail_length, lse, sumsq, ndraws_per_run, elbo, success):
    """The host arithmetic of importance_run_diagnostics, a pure function of the arrays Engine.pool_psis_runs downloads (concatenated
    in run order): ess = 1 / sumsq, log_evidence = lse - log(ndraws_per_run) with the log taken once."""
    sumsq = np.asarray(sumsq, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = 1.0 / sumsq
    log_evidence = np.asarray(lse, dtype=np.float64) - np.log(np.float64(ndraws_per_run))
    return RunDiagnostics(np.asarray(pareto_shape, dtype=np.float64), np.asarray(tail_length, dtype=np.int64), ess, log_evidence,
                          np.asarray(elbo, dtype=np.float64), np.asarray(success, dtype=bool), int(ndraws_per_run))


def importance_run_diagnostics(result, *, source="component"):
    """Per-run Pareto diagnostics of a multipathfinder result: PSIS of each run's own ndraws_per_run candidates -- k-hat, tail length,
    effective sample size, the run's own evidence estimate -- next to the run's ELBO and success flag, so that a bad pooled k-hat can
    be traced to the runs behind it.  Every engine of `result.engines` rebuilds its block of the pool as importance_summary does and
    makes ONE pass over it (Engine.pool_psis_runs: one workgroup per run); no pooled PSIS is run and no communicator is used, and the
    engines' current PSIS weights stay as they are.  A run's numbers depend on its own candidates alone, so the result is
    bit-identical for any number of engines.  source="mixture": the candidates are weighted against the uniform mixture of all runs'
    fits (one engine, as proposal="mixture").  Raises StaleHandleError when the engines hold newer fits."""
    if source not in PROPOSALS:
        raise ValueError(f"source must be one of {PROPOSALS}, got {source!r}")
    if source == "mixture":
        _check_proposal("mixture", True, result.engines or [result.engine])
    owners, _, _ = _rebuild_pool(result, False, mixture_ratios=(source == "mixture"))
    parts = [eng.pool_psis_runs(source) for eng, _ in owners]
    runs = result.pathfinder_results
    elbo = [r.elbo_estimates[r.fit_iteration - 1].value if r.fit_iteration >= 1 else float("nan") for r in runs]
    cat = {name: np.concatenate([p[name] for p in parts]) for name in ("pareto_shape", "tail_length", "lse", "sumsq")}
    return _run_diagnostics_host(cat["pareto_shape"], cat["tail_length"], cat["lse"], cat["sumsq"], runs[0].ndraws_per_run, elbo,
                                 [r.success for r in runs])


@dataclass
class ImportanceCovariance:
    """Posterior covariance from the S = nruns * ndraws_per_run pooled candidates under their PSIS weights (importance_covariance)."""
    mean: np.ndarray                # (d,) sum w x / W
    cov: np.ndarray                 # (d, d) sum w (x - mean)(x - mean)' / W, symmetric bit for bit; its diagonal is ImportanceSummary.var
    corr: np.ndarray                # (d, d) cov / sqrt(diag x diag), unit diagonal; NaN rows and columns where var <= 0
    ess: float                      # W^2 / sum w^2
    ncandidates: int                # S
    pareto_shape: float             # k-hat of the pooled PSIS (NaN for uniform weights)


def _covariance_from_sums(C, c1, W):
    """(cov, corr) from the cross moments C about the mean, the centred first moments c1 and the total weight W:
    cov = C / W - delta delta' with delta = c1 / W -- on the diagonal exactly importance_summary's var -- and
    corr = cov / sqrt(diag x diag) with a unit diagonal, NaN where a variance is not positive."""
    delta = c1 / W
    cov = C / W - delta[:, None] * delta[None, :]
    var = np.diagonal(cov)
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(np.where(var > 0, var, np.nan))
        corr = cov / (sd[:, None] * sd[None, :])
    corr[np.diag_indices_from(corr)] = np.where(var > 0, 1.0, np.nan)
    return cov, corr


def _cross_of_pool(cross_passes, center):
    """the engines' cross passes chained in run order through the carry: cross_passes[e](center, carry) -> (d, d)"""
    C = None
    for cross_pass in cross_passes:
        C = cross_pass(center, C)                                   # the carry of the next engine
    return C


def importance_covariance(result, *, importance=True):
    """Importance-weighted posterior mean, covariance and correlation from ALL candidates of a multipathfinder result -- the dense
    summary a mixture of fits has no single Sigma for (an initial metric for HMC, say).  The pool is rebuilt and weighted as in
    importance_summary and stays on the device: two moment passes give W, the mean and the centred first moment, then one
    Engine.pool_cross pass per engine about the mean forms the d x d cross moments on the matrix cores, the engines chained in run
    order through the carry.  Across engines the host only forwards the carry, so the result is bit-identical for any number of
    engines; cov is symmetric bit for bit and its diagonal is importance_summary's var.  importance=False, or a result without
    psis_result: uniform weights (then np.cov(pool, ddof=0) to rounding).  Raises StaleHandleError when the engines hold newer fits."""
    owners, weighted, pareto_shape = _rebuild_pool(result, importance)
    _, wtot, W, mean = _first_moments(owners, weighted)
    c1 = _combine_moments(_moment_pass(owners, weighted, mean)[1])
    passes = [(lambda cen, carry, eng=eng, off=off: eng.pool_cross(off, weighted, cen, carry)) for eng, off in owners]
    cov, corr = _covariance_from_sums(_cross_of_pool(passes, mean), c1, W)
    S = len(result.pathfinder_results) * result.pathfinder_results[0].ndraws_per_run
    return ImportanceCovariance(mean, cov, corr, float(W * W / wtot[1]), S, pareto_shape)


@dataclass
class LowRankCovariance:
    """Diagonal plus low rank from the pooled candidates under their PSIS weights (importance_lowrank_covariance): the top eigenpairs
    of the posterior covariance and what they leave on the diagonal, diag(diag) + U diag(eigenvalues) U'."""
    mean: np.ndarray                # (d,) sum w x / W
    var: np.ndarray                 # (d,) the diagonal of the pooled covariance: ImportanceSummary.var
    eigenvalues: np.ndarray         # (rank,) Ritz values, descending
    eigenvectors: np.ndarray        # (d, rank) Ritz vectors U, orthonormal columns
    diag: np.ndarray                # (d,) max(var - sum_j eigenvalues_j U_ij^2, 0)
    residuals: np.ndarray           # (rank,) |cov U_j - eigenvalues_j U_j|_2: an eigenvalue of cov lies within residuals_j of eigenvalues_j
    passes: int                     # applications of the covariance to the block
    converged: bool                 # max residuals <= tol * eigenvalues[0] within max_passes
    ess: float                      # W^2 / sum w^2
    ncandidates: int                # S
    pareto_shape: float             # k-hat of the pooled PSIS (NaN for uniform weights)

    def dense(self):
        """(d, d): diag(diag) + U diag(eigenvalues) U'"""
        U = self.eigenvectors
        return np.diag(self.diag) + (U * self.eigenvalues) @ U.T

    def mul(self, x):
        """dense() @ x in O(d rank) per column; x (d,) or (d, N)"""
        x = np.asarray(x, dtype=np.float64)
        U = self.eigenvectors
        return (self.diag * x.T).T + U @ (self.eigenvalues * (U.T @ x).T).T

    def _capacitance(self):
        """(D^-1 U, the Cholesky factor of Lambda^-1 + U' D^-1 U) of the Woodbury identity; PosDefException unless diag > 0 and
        eigenvalues > 0"""
        if not np.all(self.diag > 0):
            raise PosDefException(f"LowRankCovariance: diag[{int(np.flatnonzero(~(self.diag > 0))[0])}] is not positive")
        if not np.all(self.eigenvalues > 0):
            raise PosDefException("LowRankCovariance: an eigenvalue is not positive")
        DU = (self.eigenvectors.T / self.diag).T
        return DU, np.linalg.cholesky(np.diag(1.0 / self.eigenvalues) + self.eigenvectors.T @ DU)

    def solve(self, x):
        """dense()^-1 x by the Woodbury identity on the host, O(d rank) per column; x (d,) or (d, N).  PosDefException when a diag
        entry is not positive."""
        x = np.asarray(x, dtype=np.float64)
        DU, L = self._capacitance()
        Dx = (x.T / self.diag).T
        y = np.linalg.solve(L.T, np.linalg.solve(L, DU.T @ x))
        return Dx - DU @ y

    @property
    def logdet(self):
        """log det dense() = sum log diag + sum log eigenvalues + log det(Lambda^-1 + U' D^-1 U)"""
        _, L = self._capacitance()
        return float(np.sum(np.log(self.diag)) + np.sum(np.log(self.eigenvalues)) + 2.0 * np.sum(np.log(np.diagonal(L))))


def _apply_of_pool(apply_passes, center, V):
    """the engines' apply passes chained in run order through the carry: apply_passes[e](center, V, carry) -> (r, d)"""
    Y = None
    for apply_pass in apply_passes:
        Y = apply_pass(center, V, Y)                                # the carry of the next engine
    return Y


def _lowrank_from_apply(apply, d, rank, *, oversample=8, tol=1e-6, max_passes=30, seed=0):
    """Block subspace iteration for the top `rank` eigenpairs of a symmetric positive semi-definite d x d operator given only as
    apply(Q (d, b)) -> operator @ Q (d, b).  b = min(d, 32, rank + oversample) columns; start: the thin QR of
    default_rng(seed).standard_normal((d, b)).  Per pass Y = apply(Q), B = (Q'Y + (Q'Y)') / 2, eigh(B) sorted descending gives the
    Ritz values lam and vectors U = Q E, and the same Y the residuals rho_j = |Y E_j - lam_j U_j|_2; stop when
    max_{j < rank} rho_j <= tol lam_1 or after max_passes, else Q = qr(Y).  Returns (lam (rank,), U (d, rank), rho (rank,), passes,
    converged).  ValueError when Y is not finite or rank is outside [1, min(d, 32)]."""
    if not 1 <= rank <= min(d, 32):
        raise ValueError(f"lowrank_covariance: rank must be in [1, min(d, 32)] = [1, {min(d, 32)}], got {rank}")
    if oversample < 0 or max_passes < 1:
        raise ValueError("lowrank_covariance: oversample must be >= 0 and max_passes >= 1")
    b = min(d, 32, rank + int(oversample))
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, b)))[0]
    passes, converged = 0, False
    while True:
        Y = np.asarray(apply(Q), dtype=np.float64)
        passes += 1
        if not np.all(np.isfinite(Y)):
            raise ValueError("lowrank_covariance: the covariance applied to the block is not finite (a non-finite draw under a non-zero weight)")
        B = Q.T @ Y
        lam, E = np.linalg.eigh((B + B.T) / 2)
        lam, E = lam[::-1], E[:, ::-1]
        Uv = Q @ E
        rho = np.linalg.norm(Y @ E - Uv * lam, axis=0)
        converged = bool(np.max(rho[:rank]) <= tol * lam[0])
        if converged or passes >= max_passes:
            return lam[:rank].copy(), np.ascontiguousarray(Uv[:, :rank]), rho[:rank].copy(), passes, converged
        Q = np.linalg.qr(Y)[0]


def importance_lowrank_covariance(result, rank, *, importance=True, oversample=8, tol=1e-6, max_passes=30, seed=0):
    """The top `rank` <= min(d, 32) eigenpairs of the importance-weighted posterior covariance of ALL candidates of a multipathfinder
    result, and the diagonal they leave: diagonal plus low rank, the metric Pathfinder itself uses at large d, for the mixture of fits.
    The (d, d) covariance of importance_covariance is never formed: a block subspace iteration (_lowrank_from_apply) applies it to
    b = min(d, 32, rank + oversample) vectors per pass through Engine.pool_apply -- two tall-skinny contractions over the pool on the
    matrix cores, 4 d b flops per draw instead of d^2 -- as cov V = (pool apply about the mean) / W - delta (delta' V), delta the centred
    first moment over W.  The pool is rebuilt and weighted as in importance_summary; mean and var have the bits of its mean and var.  The
    engines are chained in run order through the carry and the host algebra sees the same bits from one engine or several, so the
    whole result is bit-identical for any number of engines.  importance=False, or a result without psis_result: uniform weights.
    ValueError for a rank outside [1, min(d, 32)], for W == 0 and for a non-finite draw under a non-zero weight; StaleHandleError when
    the engines hold newer fits."""
    owners, weighted, pareto_shape = _rebuild_pool(result, importance)
    _, wtot, W, mean = _first_moments(owners, weighted)
    if not W > 0:
        raise ValueError("lowrank_covariance: the total weight W is 0")
    _, c1_b, c2_b, _ = _moment_pass(owners, weighted, mean)
    delta = _combine_moments(c1_b) / W
    var = _combine_moments(c2_b) / W - delta ** 2
    d = mean.shape[0]
    passes = [(lambda cen, V, carry, eng=eng, off=off: eng.pool_apply(off, weighted, cen, V, carry)) for eng, off in owners]

    def apply(Q):
        Y = _apply_of_pool(passes, mean, np.ascontiguousarray(Q.T)).T
        return Y / W - delta[:, None] * (delta @ Q)[None, :]

    lam, Uv, rho, npass, converged = _lowrank_from_apply(apply, d, rank, oversample=oversample, tol=tol, max_passes=max_passes, seed=seed)
    diag = np.maximum(var - (Uv * Uv) @ lam, 0.0)
    S = len(result.pathfinder_results) * result.pathfinder_results[0].ndraws_per_run
    return LowRankCovariance(mean, var, lam, Uv, diag, rho, npass, converged, float(W * W / wtot[1]), S, pareto_shape)


def _f64_key(x):
    """order-preserving map of doubles onto uint64: x < y implies key(x) < key(y) (-0.0 sorts just below +0.0)"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def _f64_unkey(k):
    """inverse of _f64_key"""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    top = (k >> np.uint64(63)).astype(bool)
    return np.where(top, k & np.uint64((1 << 63) - 1), ~k).view(np.float64)


def _quantile_pass_cap(B):
    """hard cap on the passes of _quantile_search with B thresholds per probability: the pass at +-inf, then key splitting alone
    divides the at most 2^64 keys of a bracket by B per pass and the last pass tests the remaining keys one by one"""
    return 2 + int(np.ceil(64.0 / np.log2(B)))


def _key_passes_needed(diff, B):
    """passes of key splitting that certainly close a bracket of `diff` keys (uint64 array): a pass leaves fewer than ceil(diff / B)
    keys, and at most B keys are tested one by one"""
    diff = diff.copy()
    Bu = np.uint64(B)
    need = np.ones(diff.shape, dtype=np.int64)
    while True:
        big = diff > Bu
        if not big.any():
            return need
        diff = np.where(big, diff // Bu + (diff % Bu != 0).astype(np.uint64), diff)
        need += big


def _quantile_search(cdf_pass, d, targets, B):
    """The bracket search of the weighted type-1 quantiles (definition: include/pfmi.h, pfmi_pool_cdf) on top of a CDF primitive.
    cdf_pass(T) takes thresholds (nthr, d) and returns (wle, below, above, nanflag) of the whole pool; targets (nq,) holds p * W per
    probability; every pass evaluates B thresholds per probability (nq * B <= 32).  Per (probability, coordinate) the bracket is
    (lo, hi]: lo = the smallest pool value above a threshold with U < p W, hi = a pool value with U >= p W; it is closed when
    lo == hi, the only pool value left.  Thresholds split [lo, hi) evenly in value space as long as the bracket, were it to make no
    progress, could still be closed by key splitting within the cap; otherwise they split the order-preserving keys.
    Returns (quantiles (nq, d), passes)."""
    targets = np.asarray(targets, dtype=np.float64)
    nq = targets.shape[0]
    cap = _quantile_pass_cap(B)
    t = targets[:, None]
    wle, below, above, nanflag = cdf_pass(np.stack([np.full(d, -np.inf), np.full(d, np.inf)]))
    passes = 1
    total, vmax = wle[1], below[1]
    # no value reaches p W (rounding at p = 1): the largest counted value; pool values of -inf that reach it: -inf
    hi = np.broadcast_to(vmax, (nq, d)).copy()
    lo = np.broadcast_to(above[0], (nq, d)).copy()
    done = (total[None, :] < t) | ((wle[0][None, :] >= t) & (wle[0][None, :] > 0))
    hi[(wle[0][None, :] >= t) & (wle[0][None, :] > 0)] = -np.inf
    done |= (lo == hi) | ~(total > 0)[None, :]                      # (no counted weight: NaN below)
    frac = (np.arange(B, dtype=np.float64) / B)[None, :, None]
    steps = np.arange(B, dtype=np.uint64)[None, :, None]
    while not done.all():
        if passes >= cap:
            raise RuntimeError(f"quantile search did not close within {cap} passes")       # (unreachable: see _quantile_pass_cap)
        klo, khi = _f64_key(lo), _f64_key(hi)
        diff = np.where(done, np.uint64(0), khi - klo)
        by_key = (_key_passes_needed(diff, B) > cap - passes - 1) | ~np.isfinite(lo) | ~np.isfinite(hi)
        with np.errstate(over="ignore", invalid="ignore"):
            Tv = lo[:, None, :] + (hi - lo)[:, None, :] * frac
        step = diff // np.uint64(B) + (diff % np.uint64(B) != 0).astype(np.uint64)
        off = np.minimum(steps * step[:, None, :], np.maximum(diff, np.uint64(1))[:, None, :] - np.uint64(1))
        Tk = _f64_unkey(klo[:, None, :] + off)
        T = np.where(by_key[:, None, :], Tk, Tv)
        T = np.where((T >= lo[:, None, :]) & (T < hi[:, None, :]), T, lo[:, None, :])       # (a closed bracket repeats its value)
        wle, below, above, nf = cdf_pass(T.reshape(nq * B, d))
        passes += 1
        nanflag = nanflag | nf
        wle, below, above = wle.reshape(nq, B, d), below.reshape(nq, B, d), above.reshape(nq, B, d)
        up = (wle >= t[:, :, None]) & (wle > 0)
        hi_new = np.minimum(hi, np.min(np.where(up, below, np.inf), axis=1))
        lo_new = np.maximum(lo, np.max(np.where(up, -np.inf, above), axis=1))
        hi, lo = np.where(done, hi, hi_new), np.where(done, lo, lo_new)
        done |= lo == hi
    q = hi.copy()
    q[:, (nanflag != 0) | ~(total > 0)] = np.nan
    return q, passes


CDF_THRESHOLDS_PER_PASS = 32        # thresholds of one pool_cdf call (profiles/pool_quantiles.md)


def importance_quantiles(result, probs=(0.025, 0.25, 0.5, 0.75, 0.975), *, importance=True, return_passes=False):
    """Importance-weighted quantiles of every coordinate from ALL candidates of a multipathfinder result: a (len(probs), d) array of
    the weighted type-1 (inverted-CDF) quantiles defined in include/pfmi.h (pfmi_pool_cdf) -- each an element of the pool, never an
    interpolation; NaN for a coordinate with a counted NaN or when the total weight is 0.  The pool is rebuilt and weighted as in
    importance_summary and stays on the device: W comes from one moment pass, then every pass of the bracket search
    (_quantile_search) is one Engine.pool_cdf call per engine, the engines chained in run order through the carry, so the result
    is bit-identical for any number of engines.  importance=False, or a result without psis_result: uniform weights (then equal to
    np.quantile(pool, probs, method="inverted_cdf")).  return_passes=True: also the number of CDF passes over the pool."""
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if probs.ndim != 1 or probs.size == 0 or not np.all((probs >= 0) & (probs <= 1)):
        raise ValueError("importance_quantiles: probs must be a non-empty sequence of numbers in [0, 1]")
    owners, weighted, _ = _rebuild_pool(result, importance)
    q, passes = _quantiles_of_owners(owners, weighted, probs)
    return (q, passes) if return_passes else q


def _quantiles_of_pool(engs, blocks, npr, weighted, probs):
    """_quantiles_of_owners for engines that hold the run blocks `blocks` (_blocks) of npr draws per run"""
    return _quantiles_of_owners([(eng, k0 * npr) for eng, (k0, _) in zip(engs, blocks)], weighted, probs)


def _quantiles_of_owners(owners, weighted, probs):
    """importance_quantiles after its preamble: the quantiles of the pool the owners (_rebuild_pool) hold now, (q, passes)"""
    d = owners[0][0].d
    W = _first_moments(owners, weighted, want_mean=False)[2]

    def cdf_pass(T):
        wle, below, above, nan = None, None, None, None
        for eng, off in owners:
            w, b, a, f = eng.pool_cdf(off, weighted, T, wle)
            wle = w                                                 # the carry of the next engine
            below = b if below is None else np.maximum(below, b)
            above = a if above is None else np.minimum(above, a)
            nan = f if nan is None else nan | f
        return wle, below, above, nan

    group = max(1, CDF_THRESHOLDS_PER_PASS // 4)                     # at least 4 thresholds per probability
    out, passes = [], 0
    for g0 in range(0, probs.size, group):
        p = probs[g0:g0 + group]
        q, n = _quantile_search(cdf_pass, d, p * W, max(2, CDF_THRESHOLDS_PER_PASS // p.size))
        out.append(q)
        passes += n
    return np.concatenate(out, axis=0), passes


def _resample(rng, comm, psis, ndraws_per_component, ndraws, replace=True):
    """_compute_psis_result + _resample (reference src/resample.jl:58-79) over the engines of `comm`: pooled PSIS, indices on the
    device, owner gather, component ids -- one synchronisation."""
    seed = int(rng.rand_u64(1)[0])
    res, idx, draws = comm.psis_resample(ndraws, importance=psis, replace=replace, seed=seed)
    ids = idx // ndraws_per_component + 1                          # cld.(inds, N) with 1-based inds
    return res, draws, ids


def resample(result, ndraws, *, rng=None, replace=True, importance=True, ndraws_per_run=None, ntasks=1, proposal=None):
    """resample(result::MultiPathfinderResult, ndraws; ...)  (reference src/resample.jl:20-46).  proposal: "component" or "mixture" as in
    multipathfinder; None takes the result's."""
    rng = rng if rng is not None else result.rng
    engs = result.engines or [result.engine]
    if proposal is None:
        proposal = getattr(result, "proposal", "component")
    _check_proposal(proposal, importance, engs)
    runs = result.pathfinder_results
    K = len(runs)
    blocks = _blocks(K, len(engs))
    for r in runs:
        r.fit_distribution._live()                                  # the fits must still be the engine's current ones
    if ndraws_per_run is not None:                                  # fresh candidates (:102-109)
        seeds = rng.rand_u64(K)
        npr = ndraws_per_run
    else:                                                           # reuse stored draws (:97-101): the candidates are
        npr = runs[0].ndraws_per_run                                # pathfinder_results[k].draws, whatever an earlier
        seeds = [r.draw_seed for r in runs]                         # resample() drew fresh
    S = K * npr
    # a moment-matched result's map belongs to its stored candidates: fresh candidates are taken as drawn
    moved = getattr(result, "pool_transform", None) if ndraws_per_run is None else None
    if proposal == "mixture":
        engs[0].set_callback_threads(ntasks)
        res, idx, draws = _mixture_pooled_stage(engs[0], npr, [r.fit_distribution.point for r in runs], seeds, ndraws,
                                                int(rng.rand_u64(1)[0]), replace=replace, moved=moved)
        ids = idx // npr + 1
    else:
        for eng, (k0, k1) in zip(engs, blocks):
            eng.set_callback_threads(ntasks)                        # src/resample.jl:85-92: logp over `ntasks` tasks
            eng.pool_build(npr, [r.fit_distribution.point for r in runs[k0:k1]], seeds[k0:k1])
            if moved is not None:
                eng.pool_transform(moved[0], moved[1], want=False)
        # PSIS of the (re)built pool: for stored draws this reproduces result.psis_result bit for bit
        res, draws, ids = _resample(rng, _comm_for(engs), importance, npr, ndraws, replace=replace)
    psis_result = None
    if importance:
        if (ndraws_per_run is None and result.psis_result is not None and len(result.psis_result.weights) == S
                and proposal == getattr(result, "proposal", "component")):
            # stored draws + stored PSIS: the reference hands the SAME object on (:31-41).  (A result of a fresh-candidate resample
            # stores weights of ITS candidates, not of pathfinder_results[k].draws: the reference would pair them with the wrong pool
            # and fail on the length; here the stored pool's PSIS is recomputed instead.)
            psis_result = result.psis_result
        else:
            w, lw = engs[0].psis_weights(S)
            psis_result = PSISResult(w, lw, res["pareto_shape"], res["tail_length"])
    return MultiPathfinderResult(result.input, result.rng, result.logp, result.fit_distribution, draws, ids,
                                 runs, psis_result, engs[0], npr, engs, proposal, moved,
                                 getattr(result, "moment_match_history", None) if moved is not None else None)


# ---- importance-weighted moment matching of the pool (Paananen, Piironen, Buerkner, Vehtari 2021; loo::moment_match) --------------
MOMENT_MATCH_STEPS = ("T1", "T2")


def moment_match_step(step, sums0, sums, scale, shift):
    """The arithmetic of one moment-matching step, a pure function of moment sums of the CURRENT pool x (already moved by the
    cumulative map x = scale * x0 + shift).  sums0: the unweighted sums, sums: the importance-weighted ones, each
    (W, s1, c1, c2) = (sum w, sum w x, sum w (x - s1 / W), sum w (x - s1 / W)^2) as two Engine.pool_moments passes (about the origin,
    then about the mean) and _combine_moments give them.  step "T1" matches the mean: a = 1, b = m - m0; "T2" the mean and the
    marginal variance: a = sqrt(v / v0), b = m - a m0, with m = s1 / W and v = c2 / W - (c1 / W)^2 (m0, v0 from sums0).
    Returns (a, b, new_scale, new_shift): the candidate step x -> a x + b and its composition with the cumulative map,
    new_scale = a scale, new_shift = a shift + b."""
    if step not in MOMENT_MATCH_STEPS:
        raise ValueError(f"step must be one of {MOMENT_MATCH_STEPS}, got {step!r}")
    W0, s1_0, c1_0, c2_0 = sums0
    W, s1, c1, c2 = sums
    m0, m = s1_0 / W0, s1 / W
    if step == "T1":
        a = np.ones_like(m)
    else:
        v0 = c2_0 / W0 - (c1_0 / W0) ** 2
        v = c2 / W - (c1 / W) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.sqrt(v / v0)
    b = m - a * m0
    return a, b, a * scale, a * shift + b


def _moment_sums(owners, weighted):
    """(W, s1, c1, c2) of the pool the owners hold now: the two moment passes of importance_summary"""
    _, _, W, mean = _first_moments(owners, weighted)
    _, c1_b, c2_b, _ = _moment_pass(owners, weighted, mean)
    return W, mean * W, _combine_moments(c1_b), _combine_moments(c2_b)


def _map_ok(scale, shift):
    return bool(np.all(np.isfinite(scale)) and np.all(scale > 0.0) and np.all(np.isfinite(shift)))


def moment_match(result, *, k_threshold=0.7, max_iters=30, ndraws=None, rng=None, replace=True):
    """Importance-weighted moment matching of a multipathfinder result (Paananen, Piironen, Buerkner, Vehtari 2021; `moment_match` of
    the loo package) with the pool resident on the device.  All S pooled candidates are moved by ONE affine map x' = scale x0 + shift
    so that their plain moments meet their importance-weighted ones; the target is re-evaluated at the moved candidates in the same
    pass (Engine.pool_transform) and every run's proposal density changes by the constant -sum log scale, for the per-run proposals
    and for proposal="mixture" alike.  Per iteration, from the rebuilt pool and its pooled PSIS: stop when k-hat <= k_threshold;
    otherwise take the unweighted and the weighted mean and variance of the current pool (Engine.pool_moments of every engine, added
    across runs by _combine_moments in run order), try T1 (mean), then T2 (mean and marginal variance), each composed with the
    accepted cumulative map and applied to the pool AS BUILT; a trial is kept iff its pooled k-hat is finite and strictly smaller,
    otherwise reverted (a buffer swap); stop when neither is kept or after max_iters iterations.
    Returns a new MultiPathfinderResult: pool_transform = (scale, shift), moment_match_history = [(step, k-hat, accepted), ...]
    starting with ("start", k-hat of the pool as built, True), the PSIS result of the matched pool and `ndraws` (default: as many as
    the result holds) draws resampled from it.  summary(), quantiles(), covariance(), correlation(), lowrank_covariance(),
    run_diagnostics() and resample() of the returned result act on the matched pool.  The matching always starts from the pool as
    built, whatever map `result` carries, and is bit-identical for any number of engines.  Needs importance weights."""
    if result.psis_result is None:
        raise ValueError("moment_match needs a result with importance weights (importance=True)")
    engs = result.engines or [result.engine]
    runs = result.pathfinder_results
    npr = runs[0].ndraws_per_run
    S = len(runs) * npr
    mixture = getattr(result, "proposal", "component") == "mixture"
    base = dataclasses.replace(result, pool_transform=None, moment_match_history=None)
    owners, _, k = _rebuild_pool(base, True)                        # the pool as built and its pooled PSIS; the weights are on every engine
    d = owners[0][0].d

    def pooled_k():
        if mixture:
            ptr, n = engs[0].pool_mixture_ratios_dev()
            return engs[0].psis_dev(ptr, n, want_weights=False)["pareto_shape"]
        return _comm_for(engs).pool_psis()["pareto_shape"]

    scale, shift = np.ones(d), np.zeros(d)
    history = [("start", float(k), True)]
    weights_current = True                                          # the engines' PSIS weights are those of the current pool
    for _ in range(int(max_iters)):
        if not k > k_threshold:                                     # (a NaN k-hat stops too)
            break
        if not weights_current:
            pooled_k()
            weights_current = True
        sums0, sums = _moment_sums(owners, False), _moment_sums(owners, True)
        accepted = False
        for step in MOMENT_MATCH_STEPS:
            _, _, sc, sh = moment_match_step(step, sums0, sums, scale, shift)
            if not _map_ok(sc, sh):
                history.append((step, float("nan"), False))
                continue
            for eng, _ in owners:
                eng.pool_transform(sc, sh, want=False)
            k_new = pooled_k()
            if np.isfinite(k_new) and k_new < k:
                scale, shift, k, accepted = sc, sh, k_new, True
                history.append((step, float(k_new), True))
                break
            for eng, _ in owners:
                eng.pool_transform_revert()
            weights_current = False
            history.append((step, float(k_new), False))
        if not accepted:
            break
    moved = None if len(history) == 1 or not any(h[2] for h in history[1:]) else (scale, shift)
    rng = rng if rng is not None else result.rng
    ndraws = int(ndraws) if ndraws is not None else int(np.asarray(result.draws).shape[1])
    seed = int(rng.rand_u64(1)[0])
    if mixture:
        ptr, n = engs[0].pool_mixture_ratios_dev()
        res = engs[0].psis_dev(ptr, n)
        idx = engs[0].resample_indices(S, ndraws, importance=True, replace=replace, seed=seed)
        draws = engs[0].pool_gather(idx)
        w, lw = res["weights"], res["log_weights"]
    else:
        res, idx, draws = _comm_for(engs).psis_resample(ndraws, importance=True, replace=replace, seed=seed)
        w, lw = engs[0].psis_weights(S)
    psis_result = PSISResult(w, lw, res["pareto_shape"], res["tail_length"])
    return MultiPathfinderResult(result.input, result.rng, result.logp, result.fit_distribution, draws, idx // npr + 1, runs, psis_result,
                                 engs[0], npr, engs, getattr(result, "proposal", "component"), moved, history)
