"""pfmi -- host-side (Python) mirror of the Pathfinder hot-path API over libpfmi.so (MI355X / gfx950).

The product path has NO CPU fallback: importing this package is cheap, but creating an Engine
requires the built HIP library and a visible MI355X, and raises otherwise.
"""
from ._lib import PfmiError, build, lib  # noqa: F401
from .api import (DEFAULT_HISTORY_LENGTH, DEFAULT_NDRAWS_ELBO, ELBOEstimate, ImportanceCovariance, ImportanceSummary, LowRankCovariance, MixtureModel, MultiPathfinderResult,  # noqa: F401
                  MvNormal, PathfinderResult, PosDefException, PSISResult, RunDiagnostics, UniformSampler, WoodburyPDMat,
                  fit_mvnormals, importance_covariance, importance_lowrank_covariance, importance_quantiles, importance_run_diagnostics, importance_summary, maximize_elbo, moment_match, moment_match_step, multipathfinder, pathfinder, resample)
from .core import Comm, Engine, StaleHandleError  # noqa: F401
from . import hmc  # noqa: F401  (callable module: pfmi.hmc(result, ndraws, ...), pfmi.hmc.dual_averaging_update)
from .hmc import ChainSummary, CheesResult, HMCResult, NUTSResult, chain_diagnostics, chees, nuts  # noqa: F401
from .hostrng import HostRNG  # noqa: F401
from .optimize import OptimizationTrace, optimize_with_trace  # noqa: F401
from .targets import (CallbackTarget, DeviceCallbackTarget, HostFnTarget, TorchDeviceTarget, FunnelTarget, GaussTarget, t_diag, t_funnel, t_iso, t_lowrank)  # noqa: F401
