"""Static HMC and NUTS started from a Pathfinder result, with the fitted Woodbury metric, on the device (include/pfmi.h:
pfmi_hmc_enqueue, pfmi_nuts_enqueue).

The reference's worked example docs/src/examples/initializing-hmc.md, third way: "use Pathfinder's metric estimate for sampling"
(AdvancedHMC.RankUpdateEuclideanMetric(result.fit_distribution.Sigma), ext/PathfinderAdvancedHMCExt.jl:17-23) -- here the chains run
where the fits already are.  `hmc`: a fixed number of leapfrog steps per transition, Metropolis correction, full momentum refresh.
`nuts`: multinomial NUTS, trees of at most 2^max_depth - 1 leapfrog steps.  Both share one driver (`_run`): the same starts, metric,
seeds and step-size adaptation.  The target must be a device closure with a gradient (DeviceCallbackTarget(..., grad_fn=...),
TorchDeviceTarget(..., grad=...)); one engine only.  On a BUILT-IN target (t_iso, t_diag, t_lowrank, t_funnel, any GaussTarget /
FunnelTarget) `hmc` takes the fused route instead (pfmi_hmc_fused_enqueue): the chain kernel evaluates logp and its gradient itself and
loops over a run's rounds in one launch.  All three modes of `hmc` run there, and so does `nuts` with fused=True
(pfmi_nuts_fused_enqueue); the metric windows run there as adapt_metric="fused" (pfmi_hmc_fused_metric_enqueue,
pfmi_nuts_fused_metric_enqueue); `chees` does not, and adapt_metric=True stays the closure route's.

The example's second way, "initialise a metric adaptation" from the fit, is adapt="device" with adapt_metric=True (include/pfmi.h:
pfmi_hmc_adapt_metric_enqueue): the warm-up also learns a per-coordinate scale c of every chain in Stan's windows, in the coordinates
whitened by the fit's factor, so that the chain samples with L diag(c)^2 L'.  A start from a poor fit no longer keeps that fit's metric."""
import sys
import types
from dataclasses import dataclass, field
from typing import Any

import numpy as np

from .core import Engine
from .hostrng import HostRNG
from .targets import KIND_FUNNEL, KIND_GAUSS

# Nesterov dual averaging of the step size (Hoffman & Gelman 2014, Algorithm 5 and section 3.2.1: their constants)
DA_GAMMA, DA_T0, DA_KAPPA = 0.05, 10.0, 0.75


def dual_averaging_init(step_size):
    """state of dual_averaging_update for initial step sizes `step_size` (any shape): (m, Hbar, log_eps_bar, mu = log(10 eps_0))"""
    e = np.asarray(step_size, dtype=np.float64)
    return (0, np.zeros_like(e), np.zeros_like(e), np.log(10.0 * e))


def dual_averaging_update(state, accept, target_accept=0.8):
    """One update of Nesterov's dual averaging on the statistic `accept` (here: a window's mean acceptance probability, per chain):
        Hbar_m        = (1 - 1/(m + t0)) Hbar_{m-1} + (target_accept - accept) / (m + t0)
        log eps_m     = mu - sqrt(m) / gamma * Hbar_m
        log epsbar_m  = m^-kappa log eps_m + (1 - m^-kappa) log epsbar_{m-1}
    with gamma = 0.05, t0 = 10, kappa = 0.75, mu = log(10 eps_0).  Pure: returns (new state, eps_m, epsbar_m); eps_m is the step size
    of the next window, epsbar_m the averaged one to sample with."""
    m, hbar, leb, mu = state
    m = m + 1
    a = np.asarray(accept, dtype=np.float64)
    hbar = (1.0 - 1.0 / (m + DA_T0)) * hbar + (target_accept - a) / (m + DA_T0)
    le = mu - np.sqrt(m) / DA_GAMMA * hbar
    w = m ** -DA_KAPPA
    leb = w * le + (1.0 - w) * leb
    return (m, hbar, leb, mu), np.exp(le), np.exp(leb)


CHAIN_KEYS = Engine.CHAIN_KEYS        # mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, rhat


@dataclass
class ChainSummary:
    """summarystats(chns) of the reference's worked examples (docs/src/examples/turing.md): per coordinate, and for logp in `lp`"""
    mean: np.ndarray                  # (d,) each
    sd: np.ndarray
    mcse_mean: np.ndarray
    ess_mean: np.ndarray
    ess_bulk: np.ndarray
    ess_tail: np.ndarray
    rhat: np.ndarray
    lp: dict                          # the same seven values of the logp series, as floats
    nchains: int = 0
    ndraws: int = 0

    def ok(self, rhat=1.01, ess_per_chain=100):
        """Vehtari et al. (2021): every R-hat below 1.01 and bulk and tail ESS of at least 100 per chain, logp included (NaN: not ok)"""
        need = ess_per_chain * self.nchains
        r = np.append(self.rhat, self.lp["rhat"])
        e = np.concatenate([self.ess_bulk, self.ess_tail, [self.lp["ess_bulk"], self.lp["ess_tail"]]])
        return bool(np.all(r < rhat) and np.all(e >= need))

    def __str__(self):
        lines = ["Chain diagnostics (rank-normalised split R-hat, ESS)", f"  chains: {self.nchains}", f"  draws per chain: {self.ndraws}",
                 f"  rhat: max {float(np.max(self.rhat)):.4f} (logp {self.lp['rhat']:.4f})",
                 f"  ess_bulk: min {float(np.min(self.ess_bulk)):.0f} (logp {self.lp['ess_bulk']:.0f})",
                 f"  ess_tail: min {float(np.min(self.ess_tail)):.0f} (logp {self.lp['ess_tail']:.0f})",
                 f"  mcse_mean / sd: max {float(np.max(self.mcse_mean / self.sd)):.3g}"]
        return "\n".join(lines)


def chain_diagnostics(draws, engine=None):
    """mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail and rhat (dict of (d,) arrays) of any (d, T, K) array of K chains of T draws, on
    the device; `engine` needs no target (None: a temporary Engine on GPU 0)"""
    if engine is not None:
        return engine.chain_diagnostics(draws)
    e = Engine(0)
    try:
        return e.chain_diagnostics(draws)
    finally:
        e.close()


@dataclass
class HMCResult:
    draws: np.ndarray                 # (d, ndraws, nchains)
    logp: np.ndarray                  # (nchains, ndraws)
    accept_prob: np.ndarray           # (nchains, ndraws)
    energy_error: np.ndarray          # (nchains, ndraws): H1 - H0 of every transition
    divergent: np.ndarray             # (nchains, ndraws) int32
    step_size: np.ndarray             # (nchains,): what the sampling phase used
    metric_points: np.ndarray         # (nchains,): the fit point whose factor is the chain's metric
    nleapfrog: int = 0
    nwarmup: int = 0
    engine: Any = field(repr=False, default=None)
    run: int = 0                      # engine.hmc_runs after this result's last hmc_enqueue (0: unknown)
    # adapt="device": the warm-up's traces (Engine.adapt_get: eps_trace, accept_trace, divergent, n_leapfrog (nchains, nwarmup), status)
    # adapt_metric=True / "fused": also window_ends (nwin,) and scale_trace (nchains, nwin, d) (Engine.adapt_metric_get)
    warmup: Any = field(default=None, kw_only=True)
    # adapt_metric=True / "fused": (nchains, d) the per-coordinate scale the sampling phase used on the fit's factor (None: the fitted metric itself)
    metric_scale: Any = field(default=None, kw_only=True)

    def summary(self):
        """ChainSummary of the draws and of logp.  While this result is still the engine's latest run the resident records are used; after
        another run (or once the library has forgotten the chains) the result's own host copy is uploaded: the same numbers either way."""
        from ._lib import PfmiError
        eng = self.engine
        live = eng is not None and getattr(eng, "ctx", None)
        out = None
        if live and self.run and eng.hmc_runs == self.run:
            try:
                out = eng.chain_diagnostics(with_lp=True)
            except PfmiError as ex:
                if getattr(ex, "code", 0) != -3:                      # PFMI_ERR_STATE: the chains were forgotten
                    raise
        if out is None:
            x = chain_diagnostics(self.draws, eng if live else None)
            lp = chain_diagnostics(self.logp.T[None, :, :], eng if live else None)
            out = {k: np.append(x[k], lp[k]) for k in CHAIN_KEYS}
        d, n, k = self.draws.shape
        return ChainSummary(*[out[q][:d] for q in CHAIN_KEYS], {q: float(out[q][d]) for q in CHAIN_KEYS}, k, n)

    def __str__(self):
        d, n, k = self.draws.shape
        lines = ["Static HMC result (fitted Woodbury metric)", f"  chains: {k}", f"  draws per chain: {n} (warm-up: {self.nwarmup})",
                 f"  leapfrog steps: {self.nleapfrog}",
                 f"  step size: {float(np.min(self.step_size)):.3g} .. {float(np.max(self.step_size)):.3g}",
                 f"  mean acceptance: {float(np.mean(self.accept_prob)):.2f}", f"  divergent transitions: {int(np.sum(self.divergent))}"]
        return "\n".join(lines)


def _starts_and_points(result):
    """(engine, draws (d, n), fit point of every draw, the fit token the points were made under)"""
    from .api import MultiPathfinderResult
    if isinstance(result, MultiPathfinderResult):
        engs = list(result.engines) if result.engines else [result.engine]
        if len(engs) > 1:
            raise ValueError("pfmi.hmc is limited to one engine: the chains need every run's fit on the GPU that runs them")
        dists = list(result.fit_distribution)
        pts = np.array([dists[int(c) - 1].point for c in np.asarray(result.draw_component_ids)], dtype=np.int64)
        return engs[0], np.asarray(result.draws), pts, dists[0].token
    dist = result.fit_distribution
    draws = np.asarray(result.draws)
    return dist.engine, draws, np.full(draws.shape[1], dist.point, dtype=np.int64), dist.token


def _check_adapt(adapt, auto, nwarmup, adapt_metric=False):
    if adapt not in ("windows", "device"):
        raise ValueError('adapt must be "windows" or "device"')
    if adapt_metric not in (False, True, "fused"):
        raise ValueError('adapt_metric must be False, True or "fused"')
    if adapt_metric and adapt != "device":
        raise ValueError('adapt_metric adapts the metric in the windows of the device warm-up: it needs adapt="device"')
    if adapt == "device" and not (auto and nwarmup >= 1):
        raise ValueError('adapt="device" adapts the step size during the warm-up: it needs step_size="auto" and nwarmup >= 1')
    return adapt == "device"


@dataclass
class NUTSResult(HMCResult):
    """the fields of HMCResult (nleapfrog is 0: the trajectory length is dynamic) and the trees' statistics"""
    tree_depth: np.ndarray = None     # (nchains, ndraws) int32: doublings of the transition, the discarded one included
    n_leapfrog: np.ndarray = None     # (nchains, ndraws) int32: leapfrog steps of the transition
    max_depth: int = 0

    def __str__(self):
        d, n, k = self.draws.shape
        lines = ["NUTS result (fitted Woodbury metric)", f"  chains: {k}", f"  draws per chain: {n} (warm-up: {self.nwarmup})",
                 f"  tree depth: mean {float(np.mean(self.tree_depth)):.2f}, max {int(np.max(self.tree_depth))} (limit {self.max_depth})",
                 f"  leapfrog steps per draw: {float(np.mean(self.n_leapfrog)):.1f}",
                 f"  step size: {float(np.min(self.step_size)):.3g} .. {float(np.max(self.step_size)):.3g}",
                 f"  mean acceptance: {float(np.mean(self.accept_prob)):.2f}", f"  divergent transitions: {int(np.sum(self.divergent))}"]
        return "\n".join(lines)


def _builtin(target):
    """the engine's target is one the library evaluates itself (Gaussian family, funnel): static HMC runs fused"""
    return getattr(target, "kind", None) in (KIND_GAUSS, KIND_FUNNEL)


def _chains(name, result, nchains, rng, check_param=None, adapt_metric=False, fused=False):
    """what every sampler here starts from: (engine, starts x0 (d, nchains), fit points, seeds) of `result`; check_param: the sampler's
    own argument check, made where it has always been made (after the engine's and the target's, before nchains')"""
    eng, starts, pts, token = _starts_and_points(result)
    if eng is None:
        raise ValueError(f"pfmi.{name} needs a result whose fits are still on an engine")
    eng.check_token(token, f"pfmi.{name}")
    metric_fused = isinstance(adapt_metric, str)          # "fused" (_check_adapt refuses any other string before anything is enqueued)
    if metric_fused and not _builtin(eng.target):
        raise ValueError(f"pfmi.{name}: adapt_metric=\"fused\" needs a built-in target (pfmi.t_lowrank, t_diag, t_iso, t_funnel); a device closure "
                         "target with a gradient adapts its metric with adapt_metric=True")
    if fused and not _builtin(eng.target):
        raise ValueError(f"pfmi.{name}: fused=True needs a built-in target (pfmi.t_lowrank, t_diag, t_iso, t_funnel); a device closure target "
                         "with a gradient runs with fused=False")
    if _builtin(eng.target):
        if name == "nuts" and (fused or metric_fused):
            if adapt_metric and not metric_fused:
                raise ValueError("pfmi.nuts: adapt_metric=True needs a device closure target with a gradient; fused=True on a built-in target "
                                 "samples with the fitted metric itself (adapt_metric=False) or adapts it with adapt_metric=\"fused\"")
        elif name != "hmc":
            raise ValueError(f"pfmi.{name} needs a device closure target with a gradient; on a built-in target static HMC is available "
                             "(pfmi.hmc: fixed step, adapt=\"windows\" and adapt=\"device\")")
        if adapt_metric and not metric_fused:
            raise ValueError("pfmi.hmc: adapt_metric=True needs a device closure target with a gradient; on a built-in target static HMC is "
                             "available with the fitted metric itself (adapt_metric=False) or with adapt_metric=\"fused\"")
    elif not getattr(eng.target, "has_device_gradient", False):
        raise ValueError(f"pfmi.{name} needs a device closure target with a gradient (host closures and device closures without a gradient "
                         "are not supported; on built-in targets static HMC is available through pfmi.hmc)")
    if check_param is not None:
        check_param()
    nchains = starts.shape[1] if nchains is None else int(nchains)
    if not 1 <= nchains <= starts.shape[1]:
        raise ValueError(f"nchains must be in 1 .. {starts.shape[1]} (the result's draws)")
    rng = rng if rng is not None else HostRNG(0)
    return eng, np.asfortranarray(starts[:, :nchains]), pts[:nchains], rng.rand_u64(nchains)


def _run(name, result, ndraws, nchains, nwarmup, step_size, param, rng, target_accept, window, adapt, adapt_metric=False, fused=False):
    """the driver behind hmc() and nuts(): `name` is the sampler ("hmc" / "nuts"), `param` its nleapfrog / max_depth"""
    is_nuts = name == "nuts"
    def check_param():
        if is_nuts and not 1 <= int(param) <= 10:
            raise ValueError("max_depth must be in 1 .. 10")

    eng, x0, pts, seeds = _chains(name, result, nchains, rng, check_param, adapt_metric, fused)
    d, nchains = x0.shape
    fused = _builtin(eng.target)                         # (static HMC, or NUTS with fused=True: _chains has refused everything else)
    if isinstance(adapt_metric, str):                    # "fused": the metric windows inside the fused kernels
        fenq = eng.nuts_fused_metric_enqueue if is_nuts else eng.hmc_fused_metric_enqueue
    else:
        fenq = eng.nuts_fused_enqueue if is_nuts else eng.hmc_fused_enqueue
    auto = isinstance(step_size, str)
    if auto and step_size != "auto":
        raise ValueError('step_size must be a number, an array of nchains numbers or "auto"')
    eps = np.full(nchains, d ** -0.25) if auto else np.broadcast_to(np.asarray(step_size, dtype=np.float64), (nchains,)).copy()
    enqueue, wait = (fenq if fused else eng.nuts_enqueue, eng.nuts_wait) if is_nuts else (fenq if fused else eng.hmc_enqueue, eng.hmc_wait)
    warm = scale = None
    if _check_adapt(adapt, auto, int(nwarmup), adapt_metric):
        if fused:
            fenq(pts, x0, seeds, eps, param, int(ndraws), int(nwarmup), target_accept)
        else:
            if adapt_metric:
                aenq = eng.nuts_adapt_metric_enqueue if is_nuts else eng.hmc_adapt_metric_enqueue
            else:
                aenq = eng.nuts_adapt_enqueue if is_nuts else eng.hmc_adapt_enqueue
            aenq(pts, x0, seeds, eps, param, int(nwarmup), int(ndraws), target_accept)
        wait()
        got, warm = eng.hmc_get(), eng.adapt_get()
        eps = warm.pop("step_size")
        if adapt_metric:
            warm.update(eng.adapt_metric_get())
            scale = warm["scale_trace"][:, -1].copy() if len(warm["window_ends"]) else np.ones((nchains, d))
    else:
        done, first = 0, True
        if nwarmup > 0:
            state = dual_averaging_init(eps)
            ebar = eps
            while done < nwarmup:
                n = min(int(window), nwarmup - done)
                enqueue(pts, x0, seeds, eps, param, n, cont=not first)
                wait()
                first = False
                done += n
                if auto:
                    acc = eng.hmc_get(draws=False)["accept_prob"].mean(axis=1)
                    state, eps, ebar = dual_averaging_update(state, acc, target_accept)
            if auto:
                eps = np.asarray(ebar, dtype=np.float64)
        enqueue(pts, x0, seeds, eps, param, int(ndraws), cont=not first)
        wait()
        got = eng.hmc_get()
        eps = np.array(eps)
    rows = (got["draws"], got["logp"], got["accept_prob"], got["energy_error"], got["divergent"], eps, np.array(pts))
    if is_nuts:
        depth, nleap = eng.nuts_get_stats()
        return NUTSResult(*rows, 0, int(nwarmup), eng, eng.hmc_runs, depth, nleap, int(param), warmup=warm, metric_scale=scale)
    return HMCResult(*rows, int(param), int(nwarmup), eng, eng.hmc_runs, warmup=warm, metric_scale=scale)


def hmc(result, ndraws, *, nchains=None, nwarmup=0, step_size="auto", nleapfrog=8, rng=None, target_accept=0.8, window=10, adapt="windows",
        adapt_metric=False):
    """`ndraws` transitions of `nchains` chains of static HMC from a PathfinderResult / MultiPathfinderResult.

    Chain c starts at result.draws[:, c] (resample(result, nchains, replace=False) first gives distinct starts) and uses the best fit of
    the run that draw came from as its metric.  step_size: a number, one per chain, or "auto": d^(-1/4), adapted per chain during the
    `nwarmup` warm-up transitions between windows of `window` transitions by dual averaging on the window's mean acceptance
    (dual_averaging_update); the warm-up draws are discarded and sampling uses the averaged step size.  adapt="device" (step_size="auto"
    only): the device updates every chain's step size after every warm-up transition (include/pfmi.h: pfmi_hmc_adapt_enqueue); warm-up and
    sampling are ONE enqueue, and the result's `warmup` holds the traces.  adapt_metric=True (adapt="device" only): the warm-up also adapts
    a per-coordinate scale of every chain on its fit's factor in Stan's windows (pfmi_hmc_adapt_metric_enqueue; no window below 20 warm-up
    transitions); `metric_scale` is the scale the sampling used, `warmup` also holds window_ends and scale_trace.

    On a built-in target (pfmi.t_lowrank, t_diag, t_iso, t_funnel) the run takes the fused route (pfmi_hmc_fused_enqueue) in all three
    modes -- fixed step, adapt="windows", adapt="device" -- and returns the same HMCResult; adapt_metric=True raises ValueError there.
    adapt_metric="fused" (adapt="device", built-in targets only) is the metric adaptation on that route: the windows run inside the fused
    kernel (pfmi_hmc_fused_metric_enqueue), and `metric_scale`, `warmup["window_ends"]` and `warmup["scale_trace"]` are filled as for
    adapt_metric=True on a closure target; it raises ValueError on a closure target."""
    return _run("hmc", result, ndraws, nchains, nwarmup, step_size, nleapfrog, rng, target_accept, window, adapt, adapt_metric)


def nuts(result, ndraws, *, nchains=None, nwarmup=0, step_size="auto", max_depth=10, rng=None, target_accept=0.8, window=10, adapt="windows",
         adapt_metric=False, fused=False):
    """`ndraws` transitions of `nchains` chains of multinomial NUTS from a PathfinderResult / MultiPathfinderResult: the starts, metrics,
    seeds and step-size rule of `hmc` (dual averaging between windows of `window` warm-up transitions on the windows' mean accept_prob,
    the mean over a tree's leaves of min(1, exp(H0 - H))), with trees of at most 2^max_depth - 1 leapfrog steps instead of a fixed count.
    adapt="device": as for `hmc`, one enqueue whose warm-up adapts on the device after every transition (pfmi_nuts_adapt_enqueue);
    adapt_metric=True: with the metric windows of `hmc` (pfmi_nuts_adapt_metric_enqueue).

    fused=True, on a built-in target (pfmi.t_lowrank, t_diag, t_iso, t_funnel): the run takes the fused route (pfmi_nuts_fused_enqueue: the
    chain kernel evaluates logp and its gradient itself and every chain builds its trees at its own pace) in all three modes -- fixed step,
    adapt="windows", adapt="device" -- and returns the same NUTSResult.  It raises ValueError with adapt_metric=True and on a closure
    target.  adapt_metric="fused" (adapt="device", built-in targets only) adapts the metric in windows inside the fused kernel
    (pfmi_nuts_fused_metric_enqueue) and implies the fused route, with or without fused=True.  The default of `fused` is False because pfmi.nuts on a built-in target has been pinned to raise; it will flip to the fused route on
    built-in targets once that pin may be touched."""
    return _run("nuts", result, ndraws, nchains, nwarmup, step_size, max_depth, rng, target_accept, window, adapt, adapt_metric,
                fused or isinstance(adapt_metric, str))


@dataclass
class CheesResult(HMCResult):
    """the fields of HMCResult (step_size: the one shared step size, repeated per chain; nleapfrog is 0: it is jittered) and what ChEES
    learned; `warmup` holds Engine.adapt_get's traces plus tau_trace, grad_trace, hmean_trace (nwarmup,) and status"""
    trajectory_length: float = 0.0
    n_leapfrog: np.ndarray = None     # (ndraws,) int32: leapfrog steps of every sampling transition, the same in all chains
    max_leapfrog: int = 0

    def __str__(self):
        d, n, k = self.draws.shape
        lines = ["ChEES-HMC result (fitted Woodbury metric)", f"  chains: {k}", f"  draws per chain: {n} (warm-up: {self.nwarmup})",
                 f"  trajectory length: {self.trajectory_length:.3g}", f"  step size: {float(self.step_size[0]):.3g}",
                 f"  leapfrog steps per draw: {float(np.mean(self.n_leapfrog)):.1f} (limit {self.max_leapfrog})",
                 f"  mean acceptance: {float(np.mean(self.accept_prob)):.2f}", f"  divergent transitions: {int(np.sum(self.divergent))}"]
        return "\n".join(lines)


def chees(result, ndraws, *, nchains=None, nwarmup=200, step_size="auto", max_leapfrog=64, rng=None, target_accept=0.651):
    """`ndraws` transitions of `nchains` chains of ChEES-HMC (Hoffman, Radul & Sountsov 2021) from a PathfinderResult /
    MultiPathfinderResult: the starts, metrics and seeds of `hmc`, but ONE step size and ONE trajectory length for all chains, both learned
    on the device during the `nwarmup` warm-up transitions -- the step size by dual averaging on the harmonic mean of the chains'
    acceptance, the trajectory length from the chains' spread -- so no leapfrog count has to be guessed and, unlike `nuts`, every closure
    call is a full round of all chains (include/pfmi.h: pfmi_chees_enqueue).  step_size: a number or "auto" (d^(-1/4)), the initial one;
    nwarmup = 0 samples with it and a trajectory of one step.  More chains give a better estimate: use all of the result's draws."""
    if not 1 <= int(max_leapfrog) <= Engine.CHEES_MAX_LEAPFROG:
        raise ValueError(f"max_leapfrog must be in 1 .. {Engine.CHEES_MAX_LEAPFROG}")
    if isinstance(step_size, str) and step_size != "auto":
        raise ValueError('step_size must be a number or "auto"')
    eng, x0, pts, seeds = _chains("chees", result, nchains, rng)
    d, nchains = x0.shape
    eps0 = d ** -0.25 if isinstance(step_size, str) else float(step_size)
    eng.chees_enqueue(pts, x0, seeds, eps0, 0.0, int(max_leapfrog), int(nwarmup), int(ndraws), target_accept)
    eng.chees_wait()
    got, ch = eng.hmc_get(), eng.chees_get()
    warm = None
    if nwarmup > 0:
        warm = eng.adapt_get()
        warm.pop("step_size")
        warm["status"] = ch["status"]
        warm.update({k: ch[k] for k in ("tau_trace", "grad_trace", "hmean_trace")})
    return CheesResult(got["draws"], got["logp"], got["accept_prob"], got["energy_error"], got["divergent"], np.full(nchains, ch["step_size"]),
                       np.array(pts), 0, int(nwarmup), eng, eng.hmc_runs, ch["traj_length"], ch["n_leapfrog"][int(nwarmup):].copy(),
                       int(max_leapfrog), warmup=warm)


class _CallableModule(types.ModuleType):
    """pfmi.hmc is both the module (pfmi.hmc.dual_averaging_update) and the call pfmi.hmc(result, ndraws, ...)"""

    def __call__(self, *args, **kwargs):
        return hmc(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
