"""Engine: thin Python handle over a pfmi_ctx (one GPU, one stream).  All numerics run in
libpfmi.so on the MI355X; this file only marshals arrays across the C ABI."""
import ctypes as C
import os
import sys
import weakref

import numpy as np

from . import _lib
from ._lib import check

_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_u64p = C.POINTER(C.c_uint64)
RATIO_SOURCES = {"component": 0, "mixture": 1}     # include/pfmi.h PFMI_RATIOS_COMPONENT / PFMI_RATIOS_MIXTURE


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def adapt_windows(nwarmup):
    """the metric windows of a warm-up of `nwarmup` transitions (pfmi_adapt_windows, the host build of the device's rule): (init, term,
    ends) -- the first window's start, the transitions after the last window, the windows' exclusive ends (int64; empty below 20)"""
    init, term, n = C.c_int64(), C.c_int64(), C.c_int32()
    ends = np.zeros(32, dtype=np.int64)
    check(_lib.lib().pfmi_adapt_windows(int(nwarmup), C.byref(init), C.byref(term), ends.ctypes.data_as(_i64p), len(ends), C.byref(n)))
    return init.value, term.value, ends[:n.value].copy()


def _f64_of_shape(who, what, a, shape):
    """the optional argument `what` of Engine method `who` as a contiguous float64 array of `shape` (a name in it: any extent), None
    when it is None; ValueError otherwise"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != len(shape) or any(not isinstance(s, str) and n != s for n, s in zip(a.shape, shape)):
        want = ", ".join(str(s) for s in shape) + ("," if len(shape) == 1 else "")
        raise ValueError(f"{who}: {what} must have shape ({want})")
    return a


def _is_torch(x):
    """x is a torch tensor (without importing torch when the caller never did)"""
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor)


# ---- large result arrays live in page-locked memory (include/pfmi.h: pfmi_host_alloc) --------------------------------------------
# A result of tens of megabytes downloaded into an ordinary numpy array is copied by the runtime in 32 MB pieces, DMA and host copy one
# after the other (16 GB/s); into page-locked memory it is one DMA transfer (54 GB/s).  Allocating such memory costs milliseconds, so
# blocks are recycled: when the last array that views a block is garbage collected the block goes back to a small pool.
_PIN_MIN_BYTES = int(float(os.environ.get("PFMI_PIN_MIN_MB", "16")) * (1 << 20))      # (override: A/B runs of tests/probes)
_PIN_MAX_BYTES = int(float(os.environ.get("PFMI_PIN_MAX_MB", "512")) * (1 << 20))     # larger results go to ordinary (pageable) memory
_PIN_KEEP_BYTES = int(float(os.environ.get("PFMI_PIN_KEEP_MB", "1024")) * (1 << 20))  # page-locked bytes kept for reuse, all classes together
_PIN_GRAIN = 2 << 20                     # blocks are whole multiples of 2 MB (power-of-two classes wasted up to 2x)
_pin_free = {}                           # block size (bytes) -> [addresses]
_pin_kept = [0]                          # bytes currently parked in _pin_free


def _pin_release(cls_bytes, addr):
    if _pin_kept[0] + cls_bytes <= _PIN_KEEP_BYTES:
        _pin_free.setdefault(cls_bytes, []).append(addr)
        _pin_kept[0] += cls_bytes
    else:
        _lib.lib().pfmi_host_free(C.c_void_p(addr))


def result_empty(shape, dtype=np.float64):
    """np.empty(shape, order='F') for a result the library downloads into; page-locked when large (falls back to ordinary memory
    when page-locked memory is refused)"""
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    if nbytes < _PIN_MIN_BYTES or nbytes > _PIN_MAX_BYTES:     # (multi-GB page-locked blocks starve the host and take seconds to allocate)
        return np.empty(shape, dtype=dtype, order="F")
    cls_bytes = -(-nbytes // _PIN_GRAIN) * _PIN_GRAIN
    free = _pin_free.get(cls_bytes)
    if free:
        addr = free.pop()
        _pin_kept[0] -= cls_bytes
    else:
        p = C.c_void_p()
        if _lib.lib().pfmi_host_alloc(C.c_int64(cls_bytes), C.byref(p)) != 0 or not p.value:
            return np.empty(shape, dtype=dtype, order="F")
        addr = p.value
    buf = (C.c_char * nbytes).from_address(addr)
    weakref.finalize(buf, _pin_release, cls_bytes, addr).atexit = False     # (at exit the process's memory goes anyway)
    return np.frombuffer(buf, dtype=dtype).reshape(shape, order="F")


_LIVE_COMMS = weakref.WeakSet()          # a pfmi_comm holds raw pointers to its contexts: it must go before any of them does


class StaleHandleError(RuntimeError):
    """A lazy result handle (MvNormal, ELBOEstimate, trace, per-run draws) was used after the engine it points into was
    given new traces / refitted: the reference's results own their data, these handles only index device buffers."""


# Hinit of lbfgs_inverse_hessians (src/inverse_hessian.jl:25): the reference's default and the scaling its own test passes (test/inverse_hessian.jl:49)
HINIT = {"gilbert": 0, "gilbert_init": 0, 0: 0, "nocedal_wright": 1, "nocedal_wright_scaling": 1, 1: 1}


class Engine:
    def __init__(self, device=0):
        self.gen_traces = self.gen_fit = self.gen_pool = 0   # bumped by set_traces/optimize_batch, fit_batch, pool_build
        self.L = _lib.lib()
        self.ctx = C.c_void_p()
        check(self.L.pfmi_create(C.c_int32(device), C.byref(self.ctx)))
        self.device = device
        self.target = None
        self.K = self.P = self.d = 0
        self.offsets = None
        self.npoints = None
        self.J = 0
        self._hmc = None                          # (K, T) of the last hmc_enqueue that succeeded
        self._adapt = None                        # (K, W) of the adaptive run whose traces are resident (adapt_get)
        self._metric = None                       # (K, W, whitened rows kept) when that run had metric windows (adapt_metric_get)
        self._chees = None                        # (K, W, T, updates kept) of the last chees_enqueue that succeeded, while it is the latest run
        self.hmc_runs = 0                         # hmc_enqueue calls that succeeded (HMCResult.summary: is a result still the resident run?)

    def close(self):
        for cm in list(_LIVE_COMMS):                                    # every group this engine is a member of goes first
            if any(e is self for e in cm.engines):
                try:
                    cm.close()
                except Exception:
                    pass
        self.__dict__.pop("_comm_cache", None)
        if getattr(self, "ctx", None) is not None and self.ctx:
            self.L.pfmi_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise_target_error(self):
        """An exception raised by a Python `logp` closure inside the library's callback cannot cross the C frames: the closure's
        wrapper records it (and fills its output block with NaN); it is re-raised here, after the C call that invoked the closure."""
        ex = getattr(self.target, "pending_error", None)
        if ex is not None:
            self.target.pending_error = None
            raise ex

    # ---- generations of the device state lazy handles point into ------------------------------------
    def trace_token(self):
        return (self.gen_traces,)

    def fit_token(self):
        return (self.gen_traces, self.gen_fit)

    def check_token(self, token, what):
        cur = self.fit_token() if len(token) == 2 else self.trace_token()
        if self.ctx is None or token != cur:
            raise StaleHandleError(f"{what}: the engine holds a newer batch of traces / fits than this handle was made for "
                                   "(materialise results before reusing the engine, or use a separate Engine)")

    # ---- instrumentation -------------------------------------------------------------------------
    def sync(self):
        check(self.L.pfmi_sync(self.ctx))

    def timer_start(self):
        check(self.L.pfmi_timer_start(self.ctx))

    def timer_stop(self):
        ms = C.c_double()
        check(self.L.pfmi_timer_stop(self.ctx, C.byref(ms)))
        return ms.value

    def profile(self, enable=True):
        """True / 1: every stage host-synchronised; 2: event pairs left in the stream (read by kernel_time); False / 0: off"""
        check(self.L.pfmi_profile(self.ctx, C.c_int32(int(enable))))

    def kernel_time(self, name):
        ms, n = C.c_double(), C.c_int64()
        check(self.L.pfmi_kernel_time(self.ctx, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def defer(self, mode):
        """1: fit_status / elbo_batch_wait / psis_weights only QUEUE their downloads -- the arrays they return are filled by the next call
        that waits on this engine (sync, Comm.psis_resample_wait); 0: back to normal; -1: drop what is queued (after an error)"""
        check(self.L.pfmi_defer_downloads(self.ctx, C.c_int32(int(mode))))

    # ---- inputs -------------------------------------------------------------------------------------
    def set_target(self, target):
        self.target = target                      # keep parameter arrays / callbacks alive
        desc = target.descriptor()
        check(self.L.pfmi_set_target(self.ctx, C.byref(desc)))
        gp = target.gradient_pointer() if hasattr(target, "gradient_pointer") else None
        if gp is not None:                        # value-and-gradient closure: the L-BFGS runs on the device
            check(self.L.pfmi_set_target_gradient(self.ctx, C.c_void_p(gp[0]), gp[1]))

    def set_traces(self, thetas, grads):
        """thetas/grads: lists (one per path) of (L_k+1, d) arrays (point-major)."""
        npts = np.array([len(t) for t in thetas], dtype=np.int64)
        theta = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.float64) for t in thetas], axis=0))
        grad = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.float64) for g in grads], axis=0))
        assert theta.shape == grad.shape and theta.ndim == 2
        self.K, self.P, self.d = len(npts), int(npts.sum()), theta.shape[1]
        self.offsets = np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)
        self.npoints = None
        self.gen_traces += 1
        check(self.L.pfmi_set_traces(self.ctx, C.c_int32(self.K), npts.ctypes.data_as(_i64p), C.c_int32(self.d),
                                     _d(theta), _d(grad)))

    def optimize_batch(self, x0, history_length=6, maxiters=1000, g_tol=1e-8):
        """K L-BFGS optimisations on the device from x0 (K, d); the traces stay resident (as after set_traces).
        Returns npoints (K,)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        K, d = x0.shape
        assert self.target is not None and d == self.target.d
        npts = np.empty(K, dtype=np.int64)
        self.gen_traces += 1
        if getattr(self.target, "has_device_gradient", False):
            # closure target: the rounds call the Python closure from inside the C call; a recorded exception cancels and re-raises
            self.optimize_batch_enqueue(x0, history_length, maxiters, g_tol)
            return self.optimize_batch_wait()
        check(self.L.pfmi_optimize_batch(self.ctx, C.c_int32(K), _d(x0), C.c_int32(history_length), C.c_int32(maxiters),
                                         C.c_double(g_tol), npts.ctypes.data_as(_i64p)))
        self.K, self.P, self.d = K, int(npts.sum()), d
        self.offsets = np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)
        self.npoints = None
        return npts

    def optimize_batch_enqueue(self, x0, history_length=6, maxiters=1000, g_tol=1e-8):
        """first half of optimize_batch: uploads x0 and launches the K optimisations, does not wait"""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        K, d = x0.shape
        assert self.target is not None and d == self.target.d
        self.gen_traces += 1
        self._opt_K, self.K, self.P, self.d, self.offsets = K, K, 0, d, None
        self.npoints = None
        check(self.L.pfmi_optimize_batch_enqueue(self.ctx, C.c_int32(K), _d(x0), C.c_int32(history_length), C.c_int32(maxiters),
                                                 C.c_double(g_tol)))

    def optimize_batch_pump(self):
        """one non-blocking scheduling pass of a closure optimisation (calls the gradient closure for the rounds it launches); True once
        every path has finished.  An exception raised by a Python closure cancels the call and propagates."""
        fin = C.c_int32()
        rc = self.L.pfmi_optimize_batch_pump(self.ctx, C.byref(fin))
        if getattr(self.target, "pending_error", None) is not None:
            self.optimize_batch_cancel()
            self._raise_target_error()
        check(rc)
        return bool(fin.value)

    def optimize_batch_cancel(self):
        """give up an outstanding closure optimisation: drains this engine's stream; no-op otherwise"""
        check(self.L.pfmi_optimize_batch_cancel(self.ctx))

    def optimize_stats(self):
        """(rounds, closure columns) of the last closure optimisation"""
        r, n = C.c_int64(), C.c_int64()
        check(self.L.pfmi_optimize_stats(self.ctx, C.byref(r), C.byref(n)))
        return r.value, n.value

    def optimize_batch_wait(self):
        npts = np.empty(self._opt_K, dtype=np.int64)
        if getattr(self.target, "has_device_gradient", False):
            while not self.optimize_batch_pump():
                pass
        check(self.L.pfmi_optimize_batch_wait(self.ctx, npts.ctypes.data_as(_i64p)))
        self.P = int(npts.sum())
        self.offsets = np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)
        return npts

    # ---- streaming pipeline (include/pfmi.h: pfmi_stream_enqueue) -------------------------------------------------------------
    def stream_enqueue(self, x0, N, seeds, history_length=6, maxiters=1000, g_tol=1e-8, eps=1e-12):
        """optimise + fit + ELBO scan of K runs as ONE enqueued dataflow (the fits and scans of the trace points a path has already
        produced run while the paths are still being optimised).  Fixed-stride layout: trace point l of path k is slot
        k * (maxiters + 1) + l of every per-point array; seeds (K * (maxiters + 1),) is laid out the same way.  Only enqueues."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        K, d = x0.shape
        cap = int(maxiters) + 1
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            assert seeds.size == K * cap
        assert self.target is not None and d == self.target.d
        self.gen_traces += 1
        self.gen_fit += 1
        self.J = history_length
        self.K, self.P, self.d = K, K * cap, d
        self.offsets = np.arange(K + 1, dtype=np.int64) * cap
        self.npoints = None
        check(self.L.pfmi_stream_enqueue(self.ctx, C.c_int32(K), _d(x0), C.c_int32(history_length), C.c_int32(maxiters),
                                         C.c_double(g_tol), C.c_double(eps), C.c_int64(N),
                                         seeds.ctypes.data_as(_u64p) if seeds is not None else None))

    def stream_seeds(self, seeds):
        """the runs' predrawn seed streams (K * (maxiters + 1),) of a stream_enqueue(..., seeds=None): drawn while the optimiser already runs"""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert seeds.size == self.P
        check(self.L.pfmi_stream_seeds(self.ctx, seeds.ctypes.data_as(_u64p)))

    def stream_pump(self):
        """one scheduling pass of the pipeline (never blocks); True once its last segment has been launched.  A closure target's closures
        are called from inside this pass; an exception raised by one cancels the call and propagates."""
        fin = C.c_int32()
        rc = self.L.pfmi_stream_pump(self.ctx, C.byref(fin))
        if getattr(self.target, "pending_error", None) is not None:
            self.stream_cancel()
            self._raise_target_error()
        check(rc)
        return bool(fin.value)

    def stream_wait(self):
        """points per path of the last stream_enqueue (the first wait of that call)"""
        npts = np.empty(self.K, dtype=np.int64)
        if getattr(self.target, "has_device_gradient", False):
            while not self.stream_pump():               # (a closure that raises is re-raised here, not inside the C wait)
                pass
        check(self.L.pfmi_stream_wait(self.ctx, npts.ctypes.data_as(_i64p)))
        self.npoints = npts
        return npts

    def stream_cancel(self):
        """give up an outstanding stream_enqueue (a host failure between enqueue and wait): drains what is in flight; no-op otherwise"""
        check(self.L.pfmi_stream_cancel(self.ctx))

    def path_len(self, k):
        """trace points of path k (the streaming layout reserves maxiters + 1 slots per path and fills the first npoints[k])"""
        if getattr(self, "npoints", None) is not None:
            return int(self.npoints[k])
        return int(self.offsets[k + 1] - self.offsets[k])

    def get_trace(self, k, logp=True):
        n = self.path_len(k)
        theta, grad = np.empty((n, self.d)), np.empty((n, self.d))
        lp = np.empty(n) if logp else None
        check(self.L.pfmi_get_trace(self.ctx, C.c_int32(k), _d(theta), _d(lp) if logp else None, _d(grad)))
        return theta, lp, grad

    # ---- fit -------------------------------------------------------------------------------------------
    def fit_batch(self, history_length=6, eps=1e-12, hinit=None):
        """hinit: None (the context's default, gilbert_init unless set_hinit changed it), "gilbert" or "nocedal_wright" -- the `Hinit`
        keyword of lbfgs_inverse_hessians (src/inverse_hessian.jl:25)"""
        self.J = history_length
        self.gen_fit += 1
        if hinit is None:
            check(self.L.pfmi_fit_batch(self.ctx, C.c_int32(history_length), C.c_double(eps)))
        else:
            check(self.L.pfmi_fit_batch_ex(self.ctx, C.c_int32(history_length), C.c_double(eps), C.c_int32(HINIT[hinit])))

    def set_callback_threads(self, n):
        """the reference's `ntasks` for host closures (CallbackTarget): every staged block of draws is evaluated by n host threads on
        contiguous column ranges (pfmi_set_callback_threads; the closure must be thread-safe, src/multipath.jl:104-108).  A closure
        written in Python only gains where it releases the GIL (NumPy does inside its kernels)."""
        check(self.L.pfmi_set_callback_threads(self.ctx, C.c_int32(max(1, int(n)))))

    def set_hinit(self, hinit):
        """the context's default Hinit (pfmi_fit_batch and the streaming pipeline use it)"""
        check(self.L.pfmi_set_hinit(self.ctx, C.c_int32(HINIT[hinit])))

    def fit_status(self):
        status = np.empty(self.P, dtype=np.int32)
        jeff = np.empty(self.P, dtype=np.int32)
        logdet = np.empty(self.P)
        nrej = np.empty(self.K, dtype=np.int64)
        check(self.L.pfmi_get_fit_status(self.ctx, status.ctypes.data_as(_i32p), jeff.ctypes.data_as(_i32p),
                                         _d(logdet), nrej.ctypes.data_as(_i64p)))
        return status, jeff, logdet, nrej

    def get_fit(self, p, j):
        d, m = self.d, 2 * j
        k = min(d, m)
        out = dict(alpha=np.empty(d), B=np.zeros((d, m), order="F"), D=np.zeros((m, m), order="F"),
                   qr_factors=np.zeros((d, m), order="F"), T=np.zeros((k, k), order="F"),
                   V=np.zeros((k, k), order="F"), mu=np.empty(d))
        ld = C.c_double()
        check(self.L.pfmi_get_fit(self.ctx, C.c_int64(p), _d(out["alpha"]), _d(out["B"]), _d(out["D"]),
                                  _d(out["qr_factors"]), _d(out["T"]), _d(out["V"]), _d(out["mu"]), C.byref(ld)))
        out["logdet"] = ld.value
        out["j"] = j
        return out

    # ---- ELBO ---------------------------------------------------------------------------------------------
    def elbo_batch(self, N, seeds, u=None):
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert len(seeds) == self.P
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            assert u.size == self.P * self.d * N
        elbo, se = np.empty(self.P), np.empty(self.P)
        best = np.empty(self.K, dtype=np.int64)
        check(self.L.pfmi_elbo_batch(self.ctx, C.c_int64(N), seeds.ctypes.data_as(_u64p), _d(u), _d(elbo), _d(se),
                                     best.ctypes.data_as(_i64p)))
        self._raise_target_error()
        return elbo, se, best

    def elbo_batch_enqueue(self, N, seeds, u=None):
        """first half of elbo_batch: uploads the seeds, launches scan + reduction + per-path argmax, does not wait"""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert len(seeds) == self.P
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            assert u.size == self.P * self.d * N
        check(self.L.pfmi_elbo_batch_enqueue(self.ctx, C.c_int64(N), seeds.ctypes.data_as(_u64p), _d(u)))
        self._raise_target_error()

    def elbo_batch_wait(self):
        elbo, se = np.empty(self.P), np.empty(self.P)
        best = np.empty(self.K, dtype=np.int64)
        check(self.L.pfmi_elbo_batch_wait(self.ctx, _d(elbo), _d(se), best.ctypes.data_as(_i64p)))
        self._raise_target_error()
        return elbo, se, best

    def callback_stats_dev(self):
        nb = C.c_double()
        check(self.L.pfmi_callback_stats_dev(self.ctx, C.byref(nb)))
        return dict(bytes_in_hbm=nb.value)

    def callback_stats(self):
        sec, nb = C.c_double(), C.c_double()
        check(self.L.pfmi_callback_stats(self.ctx, C.byref(sec), C.byref(nb)))
        return dict(callback_seconds=sec.value, bytes_to_host=nb.value)

    def elbo_logs(self, p, N):
        lp, lq = np.empty(N), np.empty(N)
        check(self.L.pfmi_get_elbo_logs(self.ctx, C.c_int64(p), _d(lp), _d(lq)))
        return lp, lq

    def draws(self, p, seed, N, n0=0, u=None):
        """(X (d,N) column-major, logp, logq) of draws n0..n0+N-1 of fit p."""
        X = np.empty((self.d, N), order="F")
        lp, lq = np.empty(N), np.empty(N)
        if u is not None:
            u = np.asfortranarray(u, dtype=np.float64)
        check(self.L.pfmi_draws(self.ctx, C.c_int64(p), C.c_uint64(int(seed)), C.c_int64(n0), C.c_int64(N), _d(u),
                                _d(X), _d(lp), _d(lq)))
        self._raise_target_error()
        return X, lp, lq

    def logpdf(self, p, X):
        X = np.asfortranarray(X, dtype=np.float64)
        N = X.shape[1]
        out = np.empty(N)
        check(self.L.pfmi_logpdf(self.ctx, C.c_int64(p), C.c_int64(N), _d(X), _d(out)))
        return out

    def mixture_logpdf(self, points, X, componentwise=False):
        """Unnormalised log density of the uniform mixture of the fits `points` (repeats allowed) at the columns of X (d, N):
        lse[n] = log sum_k exp(logpdf(points[k], X[:, n])) -- no - log K, so that the sums of several engines combine --
        and, with componentwise=True, also comp (N, K) with comp[:, k] = logpdf(points[k], X).  X is a host array or a torch
        tensor of shape (d, N) in column-major order on this engine's device (then so are the results)."""
        pts = np.ascontiguousarray(points, dtype=np.int64).reshape(-1)
        K = len(pts)
        if _is_torch(X):
            import torch
            if X.device.type != "cuda" or X.device.index != self.device:
                raise ValueError(f"mixture_logpdf: X is on {X.device}, the engine on cuda:{self.device}")
            Xc = X.t().contiguous().t() if X.dim() == 2 else X   # column-major storage, (d, N) view
            if Xc.dtype != torch.float64 or Xc.dim() != 2 or Xc.shape[0] != self.d:
                raise ValueError(f"mixture_logpdf: X must be a float64 (d={self.d}, N) tensor")
            N = Xc.shape[1]
            lse = torch.empty(N, dtype=torch.float64, device=Xc.device)
            comp = torch.empty((K, N), dtype=torch.float64, device=Xc.device) if componentwise else None
            torch.cuda.current_stream(Xc.device).synchronize()  # X written by torch's stream before the ctx stream reads it
            check(self.L.pfmi_mixture_logpdf_dev(self.ctx, C.c_int32(K), pts.ctypes.data_as(_i64p), C.c_int64(N),
                                                 C.c_void_p(Xc.data_ptr()), C.c_void_p(lse.data_ptr()),
                                                 C.c_void_p(comp.data_ptr() if comp is not None else None)))
            self.sync()
            return (lse, comp.t()) if componentwise else lse
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("mixture_logpdf: X must be (d, N)")
        N = X.shape[1]
        lse = np.empty(N)
        comp = np.empty((N, K), order="F") if componentwise else None
        check(self.L.pfmi_mixture_logpdf(self.ctx, C.c_int32(K), pts.ctypes.data_as(_i64p), C.c_int64(N), _d(X), _d(lse),
                                         _d(comp)))
        return (lse, comp) if componentwise else lse

    # ---- remaining WoodburyPDMat operator surface -------------------------------------------------------
    OPS = dict(unwhiten=0, whiten=1, rmul=2, invunwhiten=3, mul=4, solve=5, quad=6, invquad=7)

    def woodbury_apply(self, p, op, X):
        """op in Engine.OPS applied to the columns of X (d, N); quad/invquad return N values."""
        X = np.asfortranarray(X, dtype=np.float64)
        vec = X.ndim == 1
        X2 = X.reshape(self.d, -1, order="F")
        N = X2.shape[1]
        code = self.OPS[op]
        out = np.empty(N) if code >= 6 else np.empty((self.d, N), order="F")
        check(self.L.pfmi_woodbury_apply(self.ctx, C.c_int64(p), C.c_int32(code), C.c_int64(N), _d(X2), _d(out)))
        if code >= 6:
            return out[0] if vec else out
        return out[:, 0].copy() if vec else out

    def woodbury_diag(self, p):
        out = np.empty(self.d)
        check(self.L.pfmi_woodbury_diag(self.ctx, C.c_int64(p), _d(out)))
        return out

    # ---- static HMC with a fitted metric (include/pfmi.h: pfmi_hmc_enqueue) ---------------------------------------------------
    HMC_CONTINUE, HMC_RECORD_PATH = 1, 2

    def _chain_enqueue(self, name, points, x0, seeds, step_size, param, ntransitions, flags, nwarmup=None, target_accept=None, metric=False):
        """the one enqueue of both samplers: pfmi_<name>_enqueue, or (nwarmup given) pfmi_<name>_adapt_enqueue (metric=True:
        pfmi_<name>_adapt_metric_enqueue), which take no x0 = None"""
        points = np.ascontiguousarray(points, dtype=np.int64)
        K = len(points)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        eps = np.ascontiguousarray(np.broadcast_to(np.asarray(step_size, dtype=np.float64), (K,)))
        assert seeds.shape == (K,)
        x0p = None
        if x0 is not None or nwarmup is not None:
            x0 = np.asfortranarray(x0, dtype=np.float64)
            assert x0.shape == (self.d, K), (x0.shape, self.d, K)
            x0p = _d(x0)
        head = (self.ctx, K, points.ctypes.data_as(_i64p), x0p, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), _d(eps), int(param))
        if nwarmup is None:
            rc = getattr(self.L, f"pfmi_{name}_enqueue")(*head, int(ntransitions), int(flags))
        else:
            fn = getattr(self.L, f"pfmi_{name}_adapt_metric_enqueue" if metric else f"pfmi_{name}_adapt_enqueue")
            rc = fn(*head, int(nwarmup), int(ntransitions), float(target_accept), int(flags))
        if getattr(self.target, "pending_error", None) is not None:
            self.sync()
            self._raise_target_error()
        check(rc)
        self._hmc = (K, int(ntransitions))
        self._chees = None
        if nwarmup is not None:
            self._adapt = (K, int(nwarmup))
            self._metric = (K, int(nwarmup), bool(flags & self.ADAPT_RECORD_WHITENED)) if metric else None
        elif not flags & self.HMC_CONTINUE:
            self._adapt = self._metric = None
        self.hmc_runs += 1

    def _chain_path(self, who, stats, get_path, round0, nrounds, events):
        """the recorded rounds round0 .. round0 + n - 1 of either sampler"""
        K, T = self._hmc_run(who)
        r, _ = stats()
        n = r - round0 if nrounds is None else nrounds
        X = np.empty((self.d, K, n), order="F")
        v = np.empty((self.d, K, n), order="F")
        o = np.empty((K * (self.d + 1), n), order="F")
        ev = (np.empty((n, K), dtype=self.NUTS_EVENT),) if events else ()
        check(get_path(self.ctx, round0, n, _d(X), _d(o), _d(v), *[e.ctypes.data_as(C.c_void_p) for e in ev]))
        return (X, o[:K].copy(), o[K:].reshape(self.d, K, n, order="F").copy(), v) + ev

    def hmc_enqueue(self, points, x0, seeds, step_size, nleapfrog, ntransitions, cont=False, record_path=False):
        """K chains of static HMC: chain k uses the metric of fit points[k], starts at x0[:, k] (d, K; ignored with cont=True, may be None),
        draws its momenta and accept uniforms from seeds[k] and steps by step_size[k].  Enqueues every round; does not wait.  A Python
        closure that raised is re-raised here."""
        flags = (self.HMC_CONTINUE if cont else 0) | (self.HMC_RECORD_PATH if record_path else 0)
        self._chain_enqueue("hmc", points, x0, seeds, step_size, nleapfrog, ntransitions, flags)

    def hmc_fused_enqueue(self, points, x0, seeds, step_size, nleapfrog, ntransitions, nwarmup=0, target_accept=0.8, cont=False,
                          record_path=False):
        """hmc_enqueue (nwarmup = 0) or hmc_adapt_enqueue (nwarmup >= 1: cont and record_path must be False) for an engine whose target
        is BUILT IN (Gaussian family, funnel): logp and its gradient are evaluated inside the chain kernel, one workgroup per chain
        loops over the rounds of a launch (include/pfmi.h: pfmi_hmc_fused_enqueue).  hmc_wait, hmc_get, hmc_path, adapt_get and
        chain_diagnostics serve the run; hmc_stats reports its evaluations and 0 closure columns.  Does not wait."""
        self._fused_enqueue("hmc_fused", points, x0, seeds, step_size, nleapfrog, ntransitions, nwarmup, target_accept, cont, record_path)

    def _fused_enqueue(self, name, points, x0, seeds, step_size, param, ntransitions, nwarmup, target_accept, cont, record_path, metric=False,
                       record_whitened=False):
        """the one enqueue of the fused routes: pfmi_<name>_enqueue (name: hmc_fused, nuts_fused, and with metric=True hmc_fused_metric,
        nuts_fused_metric, whose adaptive run has metric windows and takes record_whitened)"""
        points = np.ascontiguousarray(points, dtype=np.int64)
        K = len(points)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        eps = np.ascontiguousarray(np.broadcast_to(np.asarray(step_size, dtype=np.float64), (K,)))
        assert seeds.shape == (K,)
        x0p = None
        if x0 is not None:
            x0 = np.asfortranarray(x0, dtype=np.float64)
            assert x0.shape == (self.d, K), (x0.shape, self.d, K)
            x0p = _d(x0)
        flags = (self.HMC_CONTINUE if cont else 0) | (self.HMC_RECORD_PATH if record_path else 0) | (self.ADAPT_RECORD_WHITENED if record_whitened else 0)
        check(getattr(self.L, f"pfmi_{name}_enqueue")(self.ctx, K, points.ctypes.data_as(_i64p), x0p, seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      _d(eps), int(param), int(nwarmup), int(ntransitions), float(target_accept), flags))
        self._hmc = (K, int(ntransitions))
        self._chees = None
        if nwarmup:
            self._adapt, self._metric = (K, int(nwarmup)), ((K, int(nwarmup), bool(record_whitened)) if metric else None)
        elif not cont:
            self._adapt = self._metric = None
        self.hmc_runs += 1

    def hmc_fused_metric_enqueue(self, points, x0, seeds, step_size, nleapfrog, ntransitions, nwarmup=0, target_accept=0.8, cont=False,
                                 record_path=False, record_whitened=False):
        """hmc_fused_enqueue for chains that carry a per-coordinate scale, and hmc_adapt_metric_enqueue on a BUILT-IN target (include/pfmi.h:
        pfmi_hmc_fused_metric_enqueue).  nwarmup = 0: a plain run; a scale staged by chain_scale_set becomes the chains' resident one, and
        cont=True goes on with the one they carry (from an adaptive run, say).  nwarmup >= 1: a fresh adaptive run whose warm-up also
        adapts the scale in Stan's windows (cont and record_path must be False; record_whitened keeps the whitened rows); adapt_metric_get
        serves it as well.  Below 20 warm-up transitions there is no window: the run is hmc_fused_enqueue's.  Does not wait."""
        self._fused_enqueue("hmc_fused_metric", points, x0, seeds, step_size, nleapfrog, ntransitions, nwarmup, target_accept, cont, record_path,
                            metric=True, record_whitened=record_whitened)

    # ---- chain diagnostics (include/pfmi.h: pfmi_chain_diagnostics) ---------------------------------------------------------------
    CHAIN_SRC_HMC, CHAIN_SRC_HOST, CHAIN_WITH_LP = 0, 1, 1
    CHAIN_KEYS = ("mean", "sd", "mcse_mean", "ess_mean", "ess_bulk", "ess_tail", "rhat")

    def chain_diagnostics(self, draws=None, with_lp=False):
        """Rank-normalised split R-hat, bulk / tail ESS, mean, sd and MCSE per coordinate: dict of CHAIN_KEYS -> (d,) arrays.  draws: a
        (d, T, K) array of K chains of T draws, uploaded (no target or fit needed); None: the resident records of the last hmc_enqueue,
        with_lp=True appending the recorded logp series as entry d."""
        if draws is None:
            K, T = self._hmc_run("chain_diagnostics")
            n = self.d + (1 if with_lp else 0)
            src, ptr, dims = self.CHAIN_SRC_HMC, None, (0, 0, 0)
        else:
            if with_lp:
                raise ValueError("chain_diagnostics: with_lp needs the resident records (draws=None)")
            X = np.asfortranarray(draws, dtype=np.float64)
            if X.ndim != 3:
                raise ValueError("chain_diagnostics: draws must be a (d, T, K) array")
            n = X.shape[0]
            src, ptr, dims = self.CHAIN_SRC_HOST, _d(X), X.shape
        out = {k: np.empty(n) for k in self.CHAIN_KEYS}
        check(self.L.pfmi_chain_diagnostics(self.ctx, src, ptr, int(dims[0]), int(dims[1]), int(dims[2]), self.CHAIN_WITH_LP if with_lp else 0,
                                            *[_d(out[k]) for k in self.CHAIN_KEYS]))
        return out

    def _hmc_run(self, who):
        if self._hmc is None:
            raise _lib.PfmiError(f"{who}: no hmc_enqueue has succeeded on this engine")
        return self._hmc

    def hmc_wait(self):
        check(self.L.pfmi_hmc_wait(self.ctx))
        self._raise_target_error()

    def hmc_get(self, draws=True):
        """the last call's rows: dict of draws (d, T, K), logp, accept_prob, energy_error, divergent (K, T)"""
        K, T = self._hmc_run("hmc_get")
        out = {k: np.empty((K, T)) for k in ("logp", "accept_prob", "energy_error")}
        out["divergent"] = np.empty((K, T), dtype=np.int32)
        X = np.empty((self.d, T, K), order="F") if draws else None
        check(self.L.pfmi_hmc_get(self.ctx, _d(X) if draws else None, _d(out["logp"]), _d(out["accept_prob"]), _d(out["energy_error"]),
                                  out["divergent"].ctypes.data_as(C.POINTER(C.c_int32))))
        if draws:
            out["draws"] = X
        return out

    def hmc_path(self, round0=0, nrounds=None):
        """PFMI_HMC_RECORD_PATH: (X (d, K, n), logp (K, n), grad (d, K, n), v (d, K, n)) of rounds round0 .. round0 + n - 1"""
        return self._chain_path("hmc_path", self.hmc_stats, self.L.pfmi_hmc_get_path, round0, nrounds, False)

    def hmc_stats(self):
        """(rounds, closure columns) of the last hmc_enqueue"""
        r, n = C.c_int64(), C.c_int64()
        check(self.L.pfmi_hmc_stats(self.ctx, C.byref(r), C.byref(n)))
        return r.value, n.value

    # ---- NUTS with a fitted metric (include/pfmi.h: pfmi_nuts_enqueue) ---------------------------------------------------------------
    NUTS_CONTINUE, NUTS_RECORD_PATH = 1, 2
    # pfmi_nuts_event; flags: divergent 1, sub-tree turn 2, leaf taken 4, sub-tree done 8, tree taken 16, tree turn 32, max depth 64, end 128
    NUTS_EVENT = np.dtype([("t", np.int32), ("j", np.int32), ("n", np.int32), ("dir", np.int32), ("leaf", np.int32), ("flags", np.int32),
                           ("H_leaf", np.float64), ("logW_s", np.float64), ("logW", np.float64), ("H0", np.float64)])

    def nuts_enqueue(self, points, x0, seeds, step_size, max_depth, ntransitions, cont=False, record_path=False):
        """K chains of multinomial NUTS: the arguments of hmc_enqueue with max_depth (1 .. 10) in place of the leapfrog count.  Issues the first
        window of rounds and returns; nuts_pump / nuts_wait issue the rest.  A Python closure that raised is re-raised here."""
        flags = (self.NUTS_CONTINUE if cont else 0) | (self.NUTS_RECORD_PATH if record_path else 0)
        self._chain_enqueue("nuts", points, x0, seeds, step_size, max_depth, ntransitions, flags)

    def nuts_fused_enqueue(self, points, x0, seeds, step_size, max_depth, ntransitions, nwarmup=0, target_accept=0.8, cont=False,
                           record_path=False):
        """nuts_enqueue (nwarmup = 0) or nuts_adapt_enqueue (nwarmup >= 1: cont and record_path must be False) for an engine whose target
        is BUILT IN (Gaussian family, funnel): logp and its gradient are evaluated inside the chain kernel, one workgroup per chain
        builds its trees at its own pace over the trips of a launch (include/pfmi.h: pfmi_nuts_fused_enqueue).  nuts_pump, nuts_wait,
        nuts_get_stats, nuts_path, hmc_get, adapt_get and chain_diagnostics serve the run; nuts_stats reports the most trips a chain made
        and 0 closure columns.  Issues the first window of launches and returns."""
        self._fused_enqueue("nuts_fused", points, x0, seeds, step_size, max_depth, ntransitions, nwarmup, target_accept, cont, record_path)

    def nuts_fused_metric_enqueue(self, points, x0, seeds, step_size, max_depth, ntransitions, nwarmup=0, target_accept=0.8, cont=False,
                                  record_path=False, record_whitened=False):
        """nuts_fused_enqueue for chains that carry a per-coordinate scale, and nuts_adapt_metric_enqueue on a BUILT-IN target
        (include/pfmi.h: pfmi_nuts_fused_metric_enqueue): the arguments and rules of hmc_fused_metric_enqueue with max_depth in place of
        the leapfrog count; nuts_pump / nuts_wait issue the launches."""
        self._fused_enqueue("nuts_fused_metric", points, x0, seeds, step_size, max_depth, ntransitions, nwarmup, target_accept, cont, record_path,
                            metric=True, record_whitened=record_whitened)

    # ---- device-resident warm-up (include/pfmi.h: pfmi_hmc_adapt_enqueue, pfmi_nuts_adapt_enqueue) -----------------------------------
    ADAPT_KEPT_STEP = 1

    def hmc_adapt_enqueue(self, points, x0, seeds, step_size0, nleapfrog, nwarmup, ntransitions, target_accept=0.8, flags=0):
        """hmc_enqueue with `nwarmup` warm-up transitions in front whose step sizes are adapted on the device after every transition (dual
        averaging towards target_accept, from step_size0); the rows of hmc_get are the `ntransitions` sampling transitions.  One enqueue;
        does not wait.  flags must be 0."""
        self._chain_enqueue("hmc", points, x0, seeds, step_size0, nleapfrog, ntransitions, flags, nwarmup, target_accept)

    def nuts_adapt_enqueue(self, points, x0, seeds, step_size0, max_depth, nwarmup, ntransitions, target_accept=0.8, flags=0):
        """nuts_enqueue with `nwarmup` adaptive warm-up transitions in front (hmc_adapt_enqueue); nuts_pump / nuts_wait issue the rounds"""
        self._chain_enqueue("nuts", points, x0, seeds, step_size0, max_depth, ntransitions, flags, nwarmup, target_accept)

    # ---- windowed metric adaptation (include/pfmi.h: pfmi_chain_scale_set, pfmi_hmc_adapt_metric_enqueue, pfmi_nuts_adapt_metric_enqueue) ----
    ADAPT_NO_METRIC_WINDOW, ADAPT_KEPT_METRIC, ADAPT_RECORD_WHITENED, ADAPT_MAX_WINDOWS = 2, 4, 4, 32

    def chain_scale_set(self, scale):
        """stages the per-coordinate scale (K, d) of K chains for the next hmc_enqueue / nuts_enqueue (fresh or cont=True), where it becomes
        their resident scale: chain k then runs on the metric L diag(scale[k])^2 L'.  None clears the staging."""
        if scale is None:
            check(self.L.pfmi_chain_scale_set(self.ctx, 0, None))
            return
        c = np.ascontiguousarray(scale, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != self.d:
            raise ValueError(f"chain_scale_set: scale must be (K, {self.d})")
        check(self.L.pfmi_chain_scale_set(self.ctx, c.shape[0], _d(c)))

    def hmc_adapt_metric_enqueue(self, points, x0, seeds, step_size0, nleapfrog, nwarmup, ntransitions, target_accept=0.8, record_whitened=False):
        """hmc_adapt_enqueue whose warm-up also adapts every chain's per-coordinate scale in Stan's windows (include/pfmi.h); afterwards the
        adapted scale is the chains' resident one.  record_whitened keeps the whitened row of every window transition (adapt_metric_get)."""
        self._chain_enqueue("hmc", points, x0, seeds, step_size0, nleapfrog, ntransitions, self.ADAPT_RECORD_WHITENED if record_whitened else 0,
                            nwarmup, target_accept, metric=True)

    def nuts_adapt_metric_enqueue(self, points, x0, seeds, step_size0, max_depth, nwarmup, ntransitions, target_accept=0.8, record_whitened=False):
        """nuts_adapt_enqueue with the metric windows of hmc_adapt_metric_enqueue; nuts_pump / nuts_wait issue the rounds"""
        self._chain_enqueue("nuts", points, x0, seeds, step_size0, max_depth, ntransitions, self.ADAPT_RECORD_WHITENED if record_whitened else 0,
                            nwarmup, target_accept, metric=True)

    def adapt_metric_get(self):
        """the metric windows of the last hmc_adapt_metric_enqueue / nuts_adapt_metric_enqueue: dict of window_ends int64 (nwin,), scale_trace
        (K, nwin, d) the scale each window left, and with record_whitened `whitened` (K, n, d), the whitened rows of the n window transitions"""
        if self._metric is None:
            check(self.L.pfmi_adapt_metric_get(self.ctx, None, None, None, None))            # (PFMI_ERR_STATE: the library's message)
            raise _lib.PfmiError("adapt_metric_get: no run with metric windows was enqueued through this engine")
        K, W, rec = self._metric
        init, _, ends = adapt_windows(W)
        out = {"window_ends": ends, "scale_trace": np.empty((K, len(ends), self.d))}
        if rec and len(ends):
            out["whitened"] = np.empty((K, int(ends[-1]) - init, self.d))
        nwin, e = C.c_int32(), np.zeros(self.ADAPT_MAX_WINDOWS, dtype=np.int64)
        check(self.L.pfmi_adapt_metric_get(self.ctx, C.byref(nwin), e.ctypes.data_as(_i64p), _d(out["scale_trace"]),
                                           _d(out["whitened"]) if "whitened" in out else None))
        assert nwin.value == len(ends) and np.array_equal(e[:nwin.value], ends)
        return out

    def adapt_get(self):
        """the last adaptive run's warm-up: dict of step_size (K,) the sampling transitions' step sizes, eps_trace, accept_trace (K, W),
        divergent, n_leapfrog int32 (K, W) and status int32 (K,) (ADAPT_KEPT_STEP)"""
        if self._adapt is None:
            check(self.L.pfmi_adapt_get(self.ctx, None, None, None, None, None, None))       # (PFMI_ERR_STATE: the library's message)
            raise _lib.PfmiError("adapt_get: no adaptive run was enqueued through this engine")
        K, W = self._adapt
        i32p = C.POINTER(C.c_int32)
        out = {"step_size": np.empty(K), "eps_trace": np.empty((K, W)), "accept_trace": np.empty((K, W)),
               "divergent": np.empty((K, W), dtype=np.int32), "n_leapfrog": np.empty((K, W), dtype=np.int32), "status": np.empty(K, dtype=np.int32)}
        check(self.L.pfmi_adapt_get(self.ctx, _d(out["step_size"]), _d(out["eps_trace"]), _d(out["accept_trace"]),
                                    out["divergent"].ctypes.data_as(i32p), out["n_leapfrog"].ctypes.data_as(i32p), out["status"].ctypes.data_as(i32p)))
        return out

    def nuts_pump(self):
        """one scheduling pass; True once every chain has made its transitions"""
        fin = C.c_int32(0)
        check(self.L.pfmi_nuts_pump(self.ctx, C.byref(fin)))
        return bool(fin.value)

    def nuts_wait(self):
        check(self.L.pfmi_nuts_wait(self.ctx))
        self._raise_target_error()

    def nuts_get_stats(self):
        """(tree_depth, n_leapfrog) of the last call's transitions, int32 (K, T) each; the rows themselves: hmc_get"""
        K, T = self._hmc_run("nuts_get_stats")
        dep, nl = np.empty((K, T), dtype=np.int32), np.empty((K, T), dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        check(self.L.pfmi_nuts_get_stats(self.ctx, dep.ctypes.data_as(i32p), nl.ctypes.data_as(i32p)))
        return dep, nl

    def nuts_stats(self):
        """(rounds until the last chain went idle, closure columns: idle chains' and the rounds issued ahead included)"""
        r, n = C.c_int64(), C.c_int64()
        check(self.L.pfmi_nuts_stats(self.ctx, C.byref(r), C.byref(n)))
        return r.value, n.value

    def nuts_path(self, round0=0, nrounds=None):
        """PFMI_NUTS_RECORD_PATH: (X (d, K, n), logp (K, n), grad (d, K, n), v (d, K, n), events (n, K) of NUTS_EVENT) of rounds
        round0 .. round0 + n - 1; v is the synchronised momentum of the leaf the round finished"""
        return self._chain_path("nuts_path", self.nuts_stats, self.L.pfmi_nuts_get_path, round0, nrounds, True)

    # ---- ChEES-HMC (include/pfmi.h: pfmi_chees_enqueue) ----------------------------------------------------------------------------
    CHEES_CLAMPED, CHEES_KEPT_TRAJ, CHEES_RECORD_UPDATE, CHEES_MAX_LEAPFROG = 8, 16, 8, 1024

    def chees_enqueue(self, points, x0, seeds, step_size0, traj_length0, max_leapfrog, nwarmup, ntransitions, target_accept=0.651, cont=False,
                      record_path=False, record_update=False):
        """K chains of ChEES-HMC: static HMC's transitions with ONE step size and ONE jittered leapfrog count for all chains; the `nwarmup`
        warm-up transitions learn the step size (towards target_accept) and the trajectory length (from the chains' spread) on the device.
        traj_length0 = 0 starts from step_size0.  cont=True (nwarmup = 0 only) goes on from resident ChEES chains.  Issues the first window
        of rounds and returns; chees_pump / chees_wait issue the rest.  hmc_get, adapt_get, hmc_path and chain_diagnostics serve the run."""
        points = np.ascontiguousarray(points, dtype=np.int64)
        K = len(points)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert seeds.shape == (K,)
        x0p = None
        if x0 is not None:
            x0 = np.asfortranarray(x0, dtype=np.float64)
            assert x0.shape == (self.d, K), (x0.shape, self.d, K)
            x0p = _d(x0)
        flags = (self.HMC_CONTINUE if cont else 0) | (self.HMC_RECORD_PATH if record_path else 0) | (self.CHEES_RECORD_UPDATE if record_update else 0)
        rc = self.L.pfmi_chees_enqueue(self.ctx, K, points.ctypes.data_as(_i64p), x0p, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), float(step_size0),
                                       float(traj_length0), int(max_leapfrog), int(nwarmup), int(ntransitions), float(target_accept), flags)
        if getattr(self.target, "pending_error", None) is not None:
            self.sync()
            self._raise_target_error()
        check(rc)
        self._hmc = (K, int(ntransitions))
        self._chees = (K, int(nwarmup), int(ntransitions), bool(record_update) and nwarmup > 0)
        if nwarmup > 0:
            self._adapt, self._metric = (K, int(nwarmup)), None
        elif not cont:
            self._adapt = self._metric = None
        self.hmc_runs += 1

    def chees_pump(self):
        """one scheduling pass; True once every chain has made its transitions"""
        fin = C.c_int32(0)
        check(self.L.pfmi_chees_pump(self.ctx, C.byref(fin)))
        return bool(fin.value)

    def chees_wait(self):
        check(self.L.pfmi_chees_wait(self.ctx))
        self._raise_target_error()

    def chees_get(self):
        """the last chees_enqueue: dict of step_size, traj_length (the sampling values), tau_trace, grad_trace, hmean_trace (W,), n_leapfrog
        int32 (W + T,) and status (CHEES_CLAMPED, CHEES_KEPT_TRAJ, ADAPT_KEPT_STEP)"""
        if self._chees is None:
            check(self.L.pfmi_chees_get(self.ctx, None, None, None, None, None, None, None))     # (PFMI_ERR_STATE: the library's message)
            raise _lib.PfmiError("chees_get: no ChEES run was enqueued through this engine")
        K, W, T, _ = self._chees
        eps, tau, st = C.c_double(), C.c_double(), C.c_int32()
        out = {"tau_trace": np.empty(W), "grad_trace": np.empty(W), "hmean_trace": np.empty(W), "n_leapfrog": np.empty(W + T, dtype=np.int32)}
        check(self.L.pfmi_chees_get(self.ctx, C.byref(eps), C.byref(tau), _d(out["tau_trace"]), _d(out["grad_trace"]), _d(out["hmean_trace"]),
                                    out["n_leapfrog"].ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st)))
        out.update(step_size=eps.value, traj_length=tau.value, status=st.value)
        return out

    def chees_get_update(self, t0=0, n=None):
        """record_update=True: (x, xprop, vel), each (n, K, d), of the updates after warm-up transitions t0 .. t0 + n - 1"""
        if self._chees is None or not self._chees[3]:
            check(self.L.pfmi_chees_get_update(self.ctx, 0, 0, None, None, None))
            raise _lib.PfmiError("chees_get_update: the last chees_enqueue did not keep its updates")
        K, W, _, _ = self._chees
        n = W - t0 if n is None else n
        out = [np.empty((n, K, self.d)) for _ in range(3)]
        check(self.L.pfmi_chees_get_update(self.ctx, int(t0), int(n), *[_d(o) for o in out]))
        return tuple(out)

    def chees_path(self, round0=0, nrounds=None):
        """record_path=True: hmc_path's (X, logp, grad, v) of a ChEES run, rounds round0 .. round0 + n - 1 (n at most chees_stats' rounds)"""
        return self._chain_path("chees_path", self.chees_stats, self.L.pfmi_hmc_get_path, round0, nrounds, False)

    def chees_stats(self):
        """(rounds until the chains went idle = (fresh ? 1 : 0) + sum of n_leapfrog, closure columns: K per round issued)"""
        r, n = C.c_int64(), C.c_int64()
        check(self.L.pfmi_chees_stats(self.ctx, C.byref(r), C.byref(n)))
        return r.value, n.value

    # ---- pool / PSIS / resample -------------------------------------------------------------------------
    def pool_build(self, N_r, points, seeds):
        points = np.ascontiguousarray(points, dtype=np.int64)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        self.N_r = N_r
        self.gen_pool += 1
        check(self.L.pfmi_pool_build(self.ctx, C.c_int64(N_r), points.ctypes.data_as(_i64p),
                                     seeds.ctypes.data_as(_u64p)))
        self._raise_target_error()

    def pool_build_best(self, N_r, fail_seeds=None):
        """pool of the winners picked on the device from the last elbo_batch[_enqueue]; only enqueues"""
        if fail_seeds is not None:
            fail_seeds = np.ascontiguousarray(fail_seeds, dtype=np.uint64)
            assert len(fail_seeds) == self.K
        self.N_r = N_r
        self.gen_pool += 1
        check(self.L.pfmi_pool_build_best(self.ctx, C.c_int64(N_r),
                                          fail_seeds.ctypes.data_as(_u64p) if fail_seeds is not None else None))
        self._raise_target_error()

    def pool_winners(self):
        pts = np.empty(self.K, dtype=np.int64)
        seeds = np.empty(self.K, dtype=np.uint64)
        ok = np.empty(self.K, dtype=np.int32)
        check(self.L.pfmi_pool_winners(self.ctx, pts.ctypes.data_as(_i64p), seeds.ctypes.data_as(_u64p), ok.ctypes.data_as(_i32p)))
        return pts, seeds, ok.astype(bool)

    def psis_weights(self, S):
        w, lw = np.empty(S), np.empty(S)
        check(self.L.pfmi_psis_weights(self.ctx, C.c_int64(S), _d(w), _d(lw)))
        return w, lw

    def pool_get(self, draws=True):
        S = self.K * self.N_r
        X = result_empty((self.d, self.N_r, self.K)) if draws else None
        lr = np.empty(S)
        check(self.L.pfmi_pool_get(self.ctx, _d(X), _d(lr)))
        return X, lr

    def pool_moments(self, col_offset=0, importance=True, center=None):
        """Weighted moments of this engine's pool, reduced on the device (include/pfmi.h pfmi_pool_moments): per local run k and
        coordinate i, with t = x_i - center_i over the run's N_r draws, s1 = sum w t, s2 = sum w t^2, s2w = sum w^2 t^2 (each (K, d))
        and wsum (K, 2) = (sum w, sum w^2).  importance=True: w are the engine's current PSIS weights of global pool columns
        col_offset + k N_r + n (zero-weight columns are skipped); False: w = 1.  A run's rows have the same bits on whichever
        engine owns the run."""
        K, d = self.K, self.d
        center = _f64_of_shape("pool_moments", "center", center, (d,))
        wsum = np.empty((K, 2))
        s1, s2, s2w = np.empty((K, d)), np.empty((K, d)), np.empty((K, d))
        check(self.L.pfmi_pool_moments(self.ctx, int(col_offset), int(bool(importance)), _d(center), _d(wsum), _d(s1), _d(s2), _d(s2w)))
        return wsum, s1, s2, s2w

    def pool_cdf(self, col_offset, importance, thresholds, carry=None):
        """Weighted empirical CDF of this engine's pool at thresholds (nthr, d), 1 <= nthr <= 32, in one pass on the device
        (include/pfmi.h pfmi_pool_cdf): returns (wle, below, above, nanflag), the first three (nthr, d), nanflag (d,) int32.
        carry (nthr, d): the wle of the engines that own the earlier runs, added first; chaining engines in run order gives the bits
        of one engine that holds all the runs."""
        d = self.d
        thresholds = _f64_of_shape("pool_cdf", "thresholds", np.asarray(thresholds, dtype=np.float64), ("nthr", d))
        nthr = thresholds.shape[0]
        carry = _f64_of_shape("pool_cdf", "carry", carry, (nthr, d))
        wle, below, above = np.empty((nthr, d)), np.empty((nthr, d)), np.empty((nthr, d))
        nanflag = np.empty(d, dtype=np.int32)
        check(self.L.pfmi_pool_cdf(self.ctx, int(col_offset), int(bool(importance)), nthr, _d(thresholds), _d(carry), _d(wle), _d(below),
                                   _d(above), nanflag.ctypes.data_as(C.POINTER(C.c_int32))))
        return wle, below, above, nanflag

    def pool_cross(self, col_offset=0, importance=True, center=None, carry=None):
        """Weighted cross moments of this engine's pool in one pass on the device (include/pfmi.h pfmi_pool_cross): the (d, d) matrix
        C[i][j] = carry[i][j] + sum over the local runs, in run order, of sum_n (w t_i) t_j with t = x - center, weights and the
        zero-weight rule as in pool_moments.  Only i >= j is computed (and read from carry); the other triangle is its copy, so C is
        symmetric bit for bit.  carry (d, d): the C of the engines that own the earlier runs, added first; chaining engines in run
        order gives the bits of one engine that holds all the runs."""
        d = self.d
        center = _f64_of_shape("pool_cross", "center", center, (d,))
        carry = _f64_of_shape("pool_cross", "carry", carry, (d, d))
        out = np.empty((d, d))
        check(self.L.pfmi_pool_cross(self.ctx, int(col_offset), int(bool(importance)), _d(center), _d(carry), _d(out)))
        return out

    def pool_apply(self, col_offset=0, importance=True, center=None, V=None, carry=None, want_scores=False):
        """The weighted second moment of this engine's pool applied to the r <= 32 directions V (r, d) on the device, the (d, d) matrix
        never formed (include/pfmi.h pfmi_pool_apply): Y[j] = carry[j] + sum over the local runs, in run order, of sum_n (w t) z_j(n)
        with t = x - center and the scores z_j(n) = t(n) . V[j]; weights and the zero-weight rule as in pool_moments.  Returns Y (r, d),
        or (Y, scores (K N_r, r)) with want_scores.  A row of Y and a column of scores do not depend on r or on the other directions.
        carry (r, d): the Y of the engines that own the earlier runs, added first; chaining engines in run order gives the bits of one
        engine that holds all the runs."""
        d = self.d
        center = _f64_of_shape("pool_apply", "center", center, (d,))
        V = _f64_of_shape("pool_apply", "V", V, ("r", d))
        if V is None:
            raise ValueError("pool_apply: V must have shape (r, d)")
        r = V.shape[0]
        carry = _f64_of_shape("pool_apply", "carry", carry, (r, d))
        out = np.empty((r, d))
        scores = np.empty((self.K * self.N_r, r)) if want_scores else None
        check(self.L.pfmi_pool_apply(self.ctx, int(col_offset), int(bool(importance)), _d(center), r, _d(V), _d(carry), _d(out), _d(scores)))
        return (out, scores) if want_scores else out

    def pool_draws_dev(self):
        """(device pointer, count) of this engine's pool draws: d x K N_r doubles, column-major (pfmi_pool_draws_dev)"""
        p, n = C.c_void_p(), C.c_int64()
        check(self.L.pfmi_pool_draws_dev(self.ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def pool_log_ratios_dev(self):
        p, n = C.c_void_p(), C.c_int64()
        check(self.L.pfmi_pool_log_ratios_dev(self.ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def pool_mixture_ratios(self, want=True):
        """Mixture-proposal log ratios of this engine's pool, formed on the device (include/pfmi.h pfmi_pool_mixture_ratios): returns
        (log_mix, log_ratios), K N_r doubles each, log_mix = the log density of the uniform mixture of the pool's own K fits at every
        pool column and log_ratios = logp - log_mix.  pool_get()'s per-run ratios are left as they are.  want=False: nothing is
        downloaded (returns None); pool_mixture_ratios_dev() then gives the device pointer for psis_dev."""
        S = self.K * getattr(self, "N_r", 0)                # (no pool yet: the library says so)
        lm = np.empty(S) if want and S else None
        lr = np.empty(S) if want and S else None
        check(self.L.pfmi_pool_mixture_ratios(self.ctx, _d(lm), _d(lr)))
        return (lm, lr) if want else None

    def pool_mixture_ratios_dev(self):
        """(device pointer, count) of the log ratios of the last pool_mixture_ratios on the current pool"""
        p, n = C.c_void_p(), C.c_int64()
        check(self.L.pfmi_pool_mixture_ratios_dev(self.ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def pool_transform(self, scale=None, shift=None, want=True):
        """One affine map for every column of this engine's pool, and the target at the moved columns, in one pass on the device
        (include/pfmi.h pfmi_pool_transform): every column becomes fma(scale, x0, shift) with x0 the pool AS BUILT -- the map is
        cumulative, never applied on top of an earlier call -- and logp, logq (minus sum log scale), the log ratios and, when
        pool_mixture_ratios ran on the pool as built, the mixture ratios are those of the moved pool.  Every later pool pass, the
        gather and the communicator see the moved pool.  scale None: ones; shift None: zeros; both None: the pool as built is put
        back.  Returns (logp, log_ratios), K N_r doubles each, or None with want=False.  The engine's PSIS weights stay as they are."""
        d = self.d
        scale = _f64_of_shape("pool_transform", "scale", scale, (d,))
        shift = _f64_of_shape("pool_transform", "shift", shift, (d,))
        S = self.K * getattr(self, "N_r", 0)                # (no pool yet: the library says so)
        lp = np.empty(S) if want and S else None
        lr = np.empty(S) if want and S else None
        check(self.L.pfmi_pool_transform(self.ctx, _d(scale), _d(shift), _d(lp), _d(lr)))
        self._raise_target_error()
        return (lp, lr) if want else None

    def pool_transform_revert(self):
        """the state from before the last pool_transform back, without a pass (a rejected trial undone); nothing to undo: PfmiError"""
        check(self.L.pfmi_pool_transform_revert(self.ctx))

    def pool_psis_runs(self, source="component", want_weights=False):
        """PSIS of every run of this engine's pool on its own N_r log ratios, all runs in one launch (include/pfmi.h
        pfmi_pool_psis_runs): a dict of pareto_shape, tail_length, lse (logsumexp of the run's smoothed log ratios) and sumsq (sum of
        the run's squared normalised weights), each of length K, plus log_weights and weights (K, N_r), every run normalised on its
        own, with want_weights (None without).  source: "component" (pool_get()'s logp - logq) or "mixture" (the ratios of the last
        pool_mixture_ratios on this pool).  A run's numbers have the bits of psis() on the run's slice through the one-workgroup
        route and depend on nothing else; the engine's current PSIS result (psis_weights, resample_indices, the weighted pool
        passes) is left untouched."""
        if isinstance(source, str):
            if source not in RATIO_SOURCES:
                raise ValueError(f"source must be one of {tuple(RATIO_SOURCES)}, got {source!r}")
            source = RATIO_SOURCES[source]
        K, N_r = self.K, getattr(self, "N_r", 0)            # (no pool yet: the library says so)
        k, M = np.empty(K), np.empty(K, dtype=np.int64)
        lse, sumsq = np.empty(K), np.empty(K)
        lw = np.empty((K, N_r)) if want_weights and N_r else None
        w = np.empty((K, N_r)) if want_weights and N_r else None
        check(self.L.pfmi_pool_psis_runs(self.ctx, int(source), _d(k), M.ctypes.data_as(_i64p), _d(lse), _d(sumsq), _d(lw), _d(w)))
        return dict(pareto_shape=k, tail_length=M, lse=lse, sumsq=sumsq, log_weights=lw, weights=w)

    def psis(self, log_ratios, want_weights=True):
        lr = np.ascontiguousarray(log_ratios, dtype=np.float64)
        S = len(lr)
        w = np.empty(S) if want_weights else None
        lw = np.empty(S) if want_weights else None
        k, M = C.c_double(), C.c_int64()
        check(self.L.pfmi_psis(self.ctx, _d(lr), C.c_int64(S), _d(w), _d(lw), C.byref(k), C.byref(M)))
        return dict(weights=w, log_weights=lw, pareto_shape=k.value, tail_length=M.value)

    def psis_dev(self, dev_ptr, S, want_weights=True):
        w = np.empty(S) if want_weights else None
        lw = np.empty(S) if want_weights else None
        k, M = C.c_double(), C.c_int64()
        check(self.L.pfmi_psis_dev(self.ctx, C.c_void_p(dev_ptr), C.c_int64(S), _d(w), _d(lw), C.byref(k),
                                   C.byref(M)))
        return dict(weights=w, log_weights=lw, pareto_shape=k.value, tail_length=M.value)

    def resample_indices(self, S, ndraws, importance=True, replace=True, seed=0, uniforms=None):
        idx = np.empty(ndraws, dtype=np.int64)
        if uniforms is not None:
            uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        check(self.L.pfmi_resample_indices(self.ctx, C.c_int64(S), C.c_int64(ndraws), C.c_int32(int(importance)),
                                           C.c_int32(int(replace)), C.c_uint64(int(seed)), _d(uniforms),
                                           idx.ctypes.data_as(_i64p)))
        return idx

    def resample_indices_direct(self, S, uniforms):
        """StatsBase.direct_sample! on the current PSIS weights with host-drawn uniforms (0-based indices)."""
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        idx = np.empty(len(uniforms), dtype=np.int64)
        check(self.L.pfmi_resample_indices_direct(self.ctx, C.c_int64(S), C.c_int64(len(uniforms)), _d(uniforms),
                                                  idx.ctypes.data_as(_i64p)))
        return idx

    def pool_gather(self, idx, col_offset=0):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        out = result_empty((self.d, len(idx)))
        check(self.L.pfmi_pool_gather(self.ctx, C.c_int64(len(idx)), idx.ctypes.data_as(_i64p),
                                      C.c_int64(col_offset), _d(out)))
        return out

    # ---- raw device buffers (hosts that keep results on the GPU) ----------------------------------------------
    def malloc_dev(self, nbytes):
        p = C.c_void_p()
        check(self.L.pfmi_malloc_dev(self.ctx, C.c_int64(nbytes), C.byref(p)))
        return p.value

    def free_dev(self, ptr):
        check(self.L.pfmi_free_dev(self.ctx, C.c_void_p(ptr)))

    def memcpy_d2h(self, host_array, dev_ptr):
        check(self.L.pfmi_memcpy_d2h(self.ctx, host_array.ctypes.data_as(C.c_void_p), C.c_void_p(dev_ptr), C.c_int64(host_array.nbytes)))
        return host_array

    def memcpy_h2d(self, dev_ptr, host_array):
        host_array = np.ascontiguousarray(host_array)
        check(self.L.pfmi_memcpy_h2d(self.ctx, C.c_void_p(dev_ptr), host_array.ctypes.data_as(C.c_void_p), C.c_int64(host_array.nbytes)))

    def pool_gather_dev(self, idx, col_offset, dev_ptr):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        check(self.L.pfmi_pool_gather_dev(self.ctx, C.c_int64(len(idx)), idx.ctypes.data_as(_i64p),
                                          C.c_int64(col_offset), C.c_void_p(dev_ptr)))


class Comm:
    """pfmi_comm: the RCCL group behind the C ABI (csrc/comm_rccl.hip).  Comm.init_all(engines) -- one process, one Engine per
    GPU; Comm.init_rank(engine, world, rank, uid) -- one process per GPU, `uid` = Comm.unique_id() of rank 0 shipped by the
    launcher."""

    def __init__(self, handle, engines):
        self.h, self.engines, self.L = handle, list(engines), _lib.lib()
        _LIVE_COMMS.add(self)

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        check(_lib.lib().pfmi_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def init_all(cls, engines):
        arr = (C.c_void_p * len(engines))(*[e.ctx for e in engines])
        h = C.c_void_p()
        check(_lib.lib().pfmi_comm_init_all(C.c_int32(len(engines)), arr, C.byref(h)))
        return cls(h, engines)

    @classmethod
    def init_rank(cls, engine, world, rank, uid):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        h = C.c_void_p()
        check(_lib.lib().pfmi_comm_init_rank(engine.ctx, C.c_int32(world), C.c_int32(rank), buf, C.byref(h)))
        return cls(h, [engine])

    def info(self):
        w, n, v = C.c_int32(), C.c_int32(), C.c_int32()
        check(self.L.pfmi_comm_info(self.h, C.byref(w), C.byref(n), C.byref(v)))
        return dict(world=w.value, nlocal=n.value, rccl_version=v.value)

    def pool_psis(self):
        k, M = C.c_double(), C.c_int64()
        check(self.L.pfmi_comm_pool_psis(self.h, C.byref(k), C.byref(M)))
        return dict(pareto_shape=k.value, tail_length=M.value)

    def resample(self, ndraws, importance=True, replace=True, seed=0, uniforms=None, want_draws=True):
        d = self.engines[0].d
        idx = np.empty(ndraws, dtype=np.int64)
        out = result_empty((d, ndraws)) if want_draws else None
        if uniforms is not None:
            uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        check(self.L.pfmi_comm_resample(self.h, C.c_int64(ndraws), C.c_int32(int(importance)), C.c_int32(int(replace)),
                                        C.c_uint64(int(seed)), _d(uniforms), idx.ctypes.data_as(_i64p), _d(out)))
        return idx, out

    def psis_resample(self, ndraws, importance=True, replace=True, seed=0, uniforms=None, want_draws=True):
        """pooled PSIS + index selection + owner gather + all-reduce, enqueued on every local context, ONE synchronisation"""
        d = self.engines[0].d
        idx = np.empty(ndraws, dtype=np.int64)
        out = result_empty((d, ndraws)) if want_draws else None
        if uniforms is not None:
            uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        k, M = C.c_double(), C.c_int64()
        check(self.L.pfmi_comm_psis_resample(self.h, C.c_int64(ndraws), C.c_int32(int(importance)), C.c_int32(int(replace)),
                                             C.c_uint64(int(seed)), _d(uniforms), C.byref(k), C.byref(M),
                                             idx.ctypes.data_as(_i64p), _d(out)))
        return dict(pareto_shape=k.value, tail_length=M.value), idx, out

    def psis_resample_enqueue(self, ndraws, importance=True, replace=True, seed=0, uniforms=None):
        """first half of psis_resample: everything launched on every local context, no wait"""
        if uniforms is not None:
            uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        self._pr = (ndraws, uniforms)                   # (keeps the uniforms alive until the wait)
        check(self.L.pfmi_comm_psis_resample_enqueue(self.h, C.c_int64(ndraws), C.c_int32(int(importance)), C.c_int32(int(replace)),
                                                     C.c_uint64(int(seed)), _d(uniforms)))

    def psis_resample_wait(self, want_draws=True):
        """second half: the ONE host round trip (also delivers what the member engines queued under Engine.deferred())"""
        ndraws = self._pr[0]
        d = self.engines[0].d
        idx = np.empty(ndraws, dtype=np.int64)
        out = result_empty((d, ndraws)) if want_draws else None
        k, M = C.c_double(), C.c_int64()
        check(self.L.pfmi_comm_psis_resample_wait(self.h, C.byref(k), C.byref(M), idx.ctypes.data_as(_i64p), _d(out)))
        self._pr = None
        return dict(pareto_shape=k.value, tail_length=M.value), idx, out

    def close(self):
        if self.h:
            self.L.pfmi_comm_destroy(self.h)
            self.h = None
