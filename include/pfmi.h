/*
 * pfmi.h -- C ABI of libpfmi.so: the MI355X-native (gfx950, HIP) engine for the ELBO / sampling /
 * inverse-Hessian / PSIS-resampling hot path of Pathfinder.
 *
 * The reference (mlcolab/Pathfinder.jl v0.10.7) has no FFI boundary; the seam this library fills is
 * the four Julia call sites of the hot path:
 *     fit_mvnormals(points, gradients; history_length)            src/singlepath.jl:301-303
 *     maximize_elbo(rng, logp, fit_distributions[2:end], N, ntasks) src/singlepath.jl:306-308
 *     _compute_psis_result(logp, fit_distributions, draws)        src/multipath.jl:221, src/resample.jl:35
 *     _resample(rng, draws_per_component, psis_result, ndraws)    src/multipath.jl:225, src/resample.jl:42-44
 * Each entry point below cites the reference function it replaces.  INTEGRATION.md shows the
 * Julia `ccall` stubs a maintainer would add.
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; every pointer is a HOST pointer unless the
 *     function name ends in `_dev` (then it is a device pointer on the ctx's GPU);
 *   - all matrices are column-major Float64 (Julia's layout); trace points are stored point-major:
 *     theta[p*d + i] is coordinate i of point p (== hcat(points...) in Julia memory);
 *   - indices are 0-based here (the Julia wrapper adds 1);
 *   - the caller owns every host buffer; the library owns device memory inside the ctx and keeps
 *     no host pointer after a call returns; callbacks run on the calling thread during the call;
 *   - return value 0 = ok, < 0 = error (message: pfmi_last_error()); per-fit numerical failures
 *     (src/woodbury.jl:202,205 PosDefException) are reported in status[] and as NaN ELBOs, never
 *     as a process abort;
 *   - one ctx per host thread; a ctx owns one HIP stream on one GPU.
 */
#ifndef PFMI_H
#define PFMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pfmi_ctx pfmi_ctx;

/* return codes */
#define PFMI_OK 0
#define PFMI_ERR_ARG (-1)
#define PFMI_ERR_HIP (-2)
#define PFMI_ERR_STATE (-3)
#define PFMI_ERR_UNSUPPORTED (-4)
#define PFMI_ERR_NUMERIC (-5)
#define PFMI_ERR_COMM (-6)
#define PFMI_ERR_RETRY (-7)   /* transient: the enqueued step was discarded (e.g. the GPU is shared and an in-kernel hand-over timed out); enqueue it again */

/* per-fit status (src/woodbury.jl:189-190, 202, 205) */
#define PFMI_FIT_OK 0
#define PFMI_FIT_A_NOT_PD 1
#define PFMI_FIT_C_NOT_PD 2
#define PFMI_FIT_NONFINITE 3    /* reserved; not produced: no kernel sets it (a non-finite pair is rejected by the history walk instead) */
#define PFMI_FIT_ABSENT 4       /* streaming layout (pfmi_stream_enqueue): the path ended before this slot -- there is no such trace point */

/* target kinds: the hot path only ever sees logp(x) = -f(x) (src/singlepath.jl:186, src/multipath.jl:159) */
#define PFMI_TARGET_GAUSS 0          /* offset - 1/2 [ sum a_i e_i^2 - || G Wd' e ||^2 ], e = x - mean  */
#define PFMI_TARGET_FUNNEL 1         /* docs/src/examples/quickstart.md:229-234                         */
#define PFMI_TARGET_HOST_CALLBACK 2  /* arbitrary host closure, evaluated on a host copy of the draws    */
#define PFMI_TARGET_DEVICE_CALLBACK 3 /* arbitrary DEVICE closure: the draws never leave HBM               */

/* host callback: X is d x n column-major, out[n] receives logp of every column (src/elbo.jl:15) */
typedef void (*pfmi_logp_fn)(const double *X, int32_t d, int64_t n, double *out, void *user);
/* device callback (the reference's general `logp` closure, src/elbo.jl:15, src/resample.jl:90-92, kept on the GPU): X_dev is a
 * DEVICE pointer to d x n column-major draws in HBM, out_dev a DEVICE pointer to n doubles.  The function is called on the host and
 * must ENQUEUE its kernel(s) on `stream` (a hipStream_t of the ctx) and return without synchronising -- e.g. an AMDGPU.jl kernel
 * launch or a HIP launcher; the library orders its own work behind it on the same stream.  No PCIe traffic.  `stream` is NOT the same
 * on every call: an ELBO scan hands the blocks of fits to two streams in turn, so that the closure of one block runs beside the library's
 * draw writer of the next (round 6: 2.87 -> 3.27 TB/s of moved bytes with the example closure) -- the closure must use the stream it is
 * given and keep no per-call state in `user` that a concurrent call on the other stream could clobber.  (The gain comes from each kernel
 * filling the other's launch tails and idle memory pipe; a closure squeezed into the registers / LDS the writer leaves on a CU -- <= 96
 * vector registers, <= 24 KB -- was measured and is NOT worth its slower loads: write the closure for its own bandwidth.) */
typedef void (*pfmi_logp_dev_fn)(const double *X_dev, int32_t d, int64_t n, double *out_dev, void *stream, void *user);

typedef struct {
    int32_t kind;        /* PFMI_TARGET_*                                      */
    int32_t d;           /* dimension                                          */
    int32_t r;           /* GAUSS: rank of the low-rank part (0 = diagonal)    */
    int32_t reserved;
    const double *mean;  /* GAUSS: d                                           */
    const double *a;     /* GAUSS: d, diagonal precision part                  */
    const double *Wd;    /* GAUSS: d x r column-major (NULL if r == 0)         */
    const double *G;     /* GAUSS: r x r column-major, lower triangular        */
    double offset;       /* GAUSS: additive constant                           */
    pfmi_logp_fn fn;     /* HOST_CALLBACK                                      */
    void *user;          /* HOST_CALLBACK / DEVICE_CALLBACK                    */
    pfmi_logp_dev_fn dev_fn; /* DEVICE_CALLBACK                                */
} pfmi_target;

/* ---- library / context ----------------------------------------------------------------------- */
const char *pfmi_last_error(void);
int32_t pfmi_version(void);
int32_t pfmi_device_count(int32_t *count);
int32_t pfmi_create(int32_t device, pfmi_ctx **out);
int32_t pfmi_destroy(pfmi_ctx *ctx);   /* communicators that hold ctx are closed first: any finaliser order is safe */
int32_t pfmi_sync(pfmi_ctx *ctx);
/* Test / tuning hooks (kernel selection PFMI_ELBO_KERNEL / PFMI_FIT_KERNEL / PFMI_HISTORY_KERNEL / PFMI_PSIS_KERNEL / PFMI_QF_NO_TAIL,
 * PFMI_DEVCB_CHUNK_MB, PFMI_LBFGS_REJECT_EVERY, PFMI_HMC_FUSED_ROUNDS, PFMI_NUTS_FUSED_ROUNDS, the collective path's PFMI_RCCL_LIB / PFMI_COMM_ALLOW_SHARED_GPU / PFMI_COMM_FORCE_RCCL;
 * INTEGRATION.md section 3).  A hook is read from this explicit table, or from the environment variable of the same name ONLY when
 * the process was started with PFMI_DEBUG_HOOKS=1: a production process is never re-configured by a stray environment variable.
 * value == NULL unsets: the hook is then read from the environment again (under PFMI_DEBUG_HOOKS=1) or is off.  Process-global; set hooks before other threads use the library.  No reference counterpart. */
int32_t pfmi_debug_set(const char *key, const char *value);

/* device-time instrumentation (hipEvents on the ctx stream).  pfmi_timer_* bracket any sequence of
 * calls; pfmi_kernel_time returns accumulated time and launch count of one named kernel family
 * ("history", "fit", "elbo_draws" = ELBO scan, "elbo_draws_x" = draw launches that also write x, "elbo_reduce",
 * "psis", "psis_runs", "resample") since pfmi_profile(ctx, mode).  mode 1: the host waits after every stage (each stage starts on an idle
 * GPU: its figure includes the host's launch latency); mode 2: the event pairs stay in the stream and are read by
 * pfmi_kernel_time (which waits for them) -- the pipeline runs as it does unprofiled and a stage's figure is its kernels'
 * time; mode 0: off.
 * Two kinds of name are host-side counters, not stages: they are counted whatever the mode, since the ctx was created, and
 * report *milliseconds = 0.  "qf_handover_lost": scan pieces that gave up waiting for their fit's constants.
 * "qf:<KC>,<TGT>,<RPAD>,<NG>:<res|stream>:<cut>": scan calls that took this plan of the single-pass ELBO scan -- column padding
 * KC (4 .. 32), target kind TGT (0 none, 1 Gaussian, 2 funnel), target rank padding RPAD (0, 8, 16), NG 16-draw groups per
 * wave (1, 2), factor block resident in LDS or streamed in chunks, and cut "whole" (one workgroup per fit), "split" (few fits,
 * each cut into pieces), "tail-share" (one launch; the fits of the last partial round of CUs cut into pieces that share the
 * per-fit constants) or "tail-two" (the same tail as a second launch).
 * The three kernels that make draws are counted the same way, one count per kernel launch:
 * "xw:<KC>:<res|stream>:<whole|split>": the streaming draw writer -- column padding KC (4 .. 32), factor block resident in LDS
 * or streamed in chunks, one workgroup per fit ("whole") or each fit's draw groups cut over several ("split").
 * "mf:<KC>,<NBW>,<TGT>,<RPAD>:<x|nox>:<whole|split>": the two-pass MFMA kernel -- KC (4 .. 16), NBW 16-row blocks per wave
 * (1, 2, 4, 8), TGT / RPAD as above, draws written ("x") or only their log densities ("nox"), and the cut as for the writer.
 * "lane:<KPAD>,<TGT>,<RPAD>:<u|rng>:<x|nox>": the lane-per-draw kernel -- column padding KPAD (4 .. 64), normals supplied by
 * the caller ("u") or made by the in-kernel generator ("rng"), draws written or not.
 * The fit kernels likewise, one count per kernel launch (the stage name "fit" keeps its meaning):
 * "fit:reg:<KPAD>,<RPT>": the register-resident kernel (d <= 1024, history_length <= 8) -- column padding KPAD (4 .. 16), RPT
 * rows per thread (1: d <= 256, 2: d <= 512, 4: d <= 1024).
 * "fit:gen:<KPAD>": the general column-by-column kernel -- KPAD (4 .. 64): history_length >= 9 at d <= 1024, every shape the
 * large-d kernels decline, and PFMI_FIT_KERNEL=mem.
 * "fit:tsqr:<KPAD>": the TSQR kernel with Householder reconstruction (d > 1024) -- KPAD (8 .. 32).
 * "fit:panel:<KPAD>,<RPT>,<cols>": the left-looking panel kernel (d > 1024) -- KPAD (8 .. 32), RPT the bucket of rows per thread
 * (5, 10, 20, 32), cols the panel width (4; 2 in the last bucket).
 * The history walk likewise, one count per kernel launch (the stage name "history" keeps its meaning):
 * "hist:reg:<EPT>,<NT>": the register-set kernel -- EPT coordinates per thread and NT threads per path: 1,64 2,64 4,64 (d <= 64,
 * 128, 256), 2,256 4,256 (d <= 512, 1024), 2,1024 (d <= 2048), 12,1024 16,1024 (d <= 12 288, 16 384), and 4,1024 .. 10,1024 under
 * PFMI_HISTORY_KERNEL=prefetch (2048 < d <= 10 240).
 * "hist:lean:<EPT>": the lean kernel with 1 / alpha in LDS (2048 < d <= 10 240) -- EPT 4, 6, 8, 10.
 * "hist:mem": the memory-resident kernel (d > 16 384, and PFMI_HISTORY_KERNEL=mem).
 * The operator surface likewise, one count per kernel launch:
 * "woodbury:<KPAD>:<mode>": the lane-per-column kernel behind pfmi_woodbury_apply -- column padding KPAD (4 .. 64), mode 0 .. 3.
 * "woodbury_diag:<KPAD>": the kernel behind pfmi_woodbury_diag.
 * The fused static-HMC kernel (pfmi_hmc_fused_enqueue) has the stage name "hmc_fused" and, one count per kernel launch,
 * "hmc_fused:<KPAD>:<res|stream>:<f|g0|g8|g16>": column padding KPAD (4 .. 64), the chain's factor rows staged in LDS or streamed
 * from HBM, and the target -- the funnel, or the Gaussian family with rank padding 0, 8 or 16.  The fused NUTS kernel
 * (pfmi_nuts_fused_enqueue) likewise: stage "nuts_fused", counters "nuts_fused:<KPAD>:<res|stream>:<f|g0|g8|g16>"; the fused-metric
 * kernels (pfmi_*_fused_metric_enqueue): stages "hmc_fused_metric" / "nuts_fused_metric", counters "<stage>:<KPAD>:<res|stream>:<f|g0|g8|g16>". */
int32_t pfmi_timer_start(pfmi_ctx *ctx);
int32_t pfmi_timer_stop(pfmi_ctx *ctx, double *milliseconds);
int32_t pfmi_profile(pfmi_ctx *ctx, int32_t enable);
int32_t pfmi_kernel_time(pfmi_ctx *ctx, const char *name, double *milliseconds, int64_t *launches);

/* ---- inputs ------------------------------------------------------------------------------------ */
/* The target log density (what `logp` is in src/elbo.jl:12-20 and src/resample.jl:81-95). */
int32_t pfmi_set_target(pfmi_ctx *ctx, const pfmi_target *target);

/* K optimisation traces (OptimizationTrace.points / .gradients, src/optimize.jl:110-114), path k
 * has npoints[k] = L_k + 1 points; theta/grad hold all P = sum npoints points, point-major. */
int32_t pfmi_set_traces(pfmi_ctx *ctx, int32_t K, const int64_t *npoints, int32_t d,
                        const double *theta, const double *grad);

/* ---- trajectory generation on the device ---------------------------------- */
/* Plays optimize_with_trace (src/optimize.jl:35-121) for the BUILT-IN targets: runs K independent L-BFGS
 * optimisations of -logp from x0[k] (K x d, point-major), one persistent workgroup per path, and leaves the
 * traces resident in HBM exactly as pfmi_set_traces would (so pfmi_fit_batch follows without a host round trip).
 * This repo's own driver (two-loop recursion, strong-Wolfe line search, maxiters as src/optimize.jl:40, stop at
 * |grad|_inf <= g_tol); Optim.LBFGS + HagerZhang of the reference is third party: trajectory parity unpinned.
 * npoints[k] = L_k + 1 out.  Callback targets -> PFMI_ERR_UNSUPPORTED (optimise on the host, pfmi_set_traces), except a DEVICE_CALLBACK
 * target with a gradient closure (pfmi_set_target_gradient below). */
int32_t pfmi_optimize_batch(pfmi_ctx *ctx, int32_t K, const double *x0, int32_t history_length, int32_t maxiters,
                            double g_tol, int64_t *npoints);
/* The same in two halves, for ONE host thread that drives several contexts (one per GPU, src/multipath.jl:190-208 fans the runs
 * out over tasks): _enqueue uploads x0 and launches the optimisations without waiting, _wait blocks until this ctx's paths are done,
 * packs the traces and returns npoints[K].  pfmi_optimize_batch == _enqueue + _wait. */
int32_t pfmi_optimize_batch_enqueue(pfmi_ctx *ctx, int32_t K, const double *x0, int32_t history_length, int32_t maxiters,
                                    double g_tol);
int32_t pfmi_optimize_batch_wait(pfmi_ctx *ctx, int64_t *npoints);

/* ---- trajectory generation for a user closure (optional gradient of a DEVICE_CALLBACK target) ------------------------------------------ */
/* Attaches a value-and-gradient closure to the ctx's current DEVICE_CALLBACK target (any other kind: PFMI_ERR_ARG).  It has the
 * pfmi_logp_dev_fn signature with a wider output: out_dev[0..n) receives logp of each column and out_dev[n + j * d + i] receives
 * d logp / d x_i at column j (the d x n layout of X).  It enqueues on the stream it is given -- for the optimiser always the ctx's main
 * stream -- and returns without synchronising.  pfmi_set_target clears it.  With it, pfmi_optimize_batch / _enqueue / _wait accept the
 * target (history_length 1..32, d bounded by memory): the K paths run the same L-BFGS as for the built-in targets in ROUNDS -- one
 * library kernel advances every path by one function evaluation, then the closure is called once on all K trial points (d x K,
 * column-major, in HBM).  The traces end up resident exactly as for a built-in target.  _enqueue launches the first round only; the
 * closure is called on the thread that pumps (pfmi_optimize_batch_pump, or _wait, which pumps until done). */
int32_t pfmi_set_target_gradient(pfmi_ctx *ctx, pfmi_logp_dev_fn logp_grad_fn, void *user);
/* one non-blocking scheduling pass of a closure optimisation (modelled on pfmi_stream_pump; one host thread may drive several contexts):
 * keeps at most 4 rounds in flight and reads the rounds' published count of running paths.  *finished = 1 once it has read zero (or the
 * hard cap of maxiters * 55 + 1 rounds, the line search's evaluation budget, is reached); then call pfmi_optimize_batch_wait. */
int32_t pfmi_optimize_batch_pump(pfmi_ctx *ctx, int32_t *finished);
/* gives up an outstanding closure optimisation (e.g. the closure failed on the host): drains this ctx's stream and forgets the call; the
 * context stays usable.  No-op otherwise.  pfmi_set_target, pfmi_set_traces and pfmi_optimize_batch_enqueue do the same implicitly. */
int32_t pfmi_optimize_batch_cancel(pfmi_ctx *ctx);
/* rounds and columns handed to the closure in the last closure optimisation (0, 0 after a built-in one) */
int32_t pfmi_optimize_stats(pfmi_ctx *ctx, int64_t *rounds, int64_t *closure_columns);
/* OptimizationTrace of path k (src/optimize.jl:94-100): theta/grad (L_k+1) x d point-major, logp L_k+1; any may be
 * NULL.  logp is only available for traces made by pfmi_optimize_batch. */
int32_t pfmi_get_trace(pfmi_ctx *ctx, int32_t k, double *theta, double *logp, double *grad);

/* ---- streaming pipeline (round 5): optimise + fit + ELBO scan as ONE enqueued dataflow ---------------------------------------
 * What src/singlepath.jl:285-325 does for one run -- optimise (:285-297), fit_mvnormals (:301-303), maximize_elbo (:306-308) -- for K
 * runs at once, with the fits and scans of the trace points a path has ALREADY produced running while the paths are still being
 * optimised (the reference overlaps whole runs over tasks, src/multipath.jl:190-208).  Equivalent to, and bit-identical with,
 *     pfmi_optimize_batch(K, x0, J, maxiters, g_tol) ; pfmi_fit_batch(J, eps) ; pfmi_elbo_batch_enqueue(N, seeds')
 * except for the LAYOUT: trace point l of path k is slot  p = k * (maxiters + 1) + l  in every per-point array of the context (status,
 * j_eff, logdet, elbo, se, ... have K * (maxiters + 1) entries; the slots a path did not reach carry status PFMI_FIT_ABSENT / NaN), and
 * `seeds` holds the runs' predrawn seed streams: seeds[k * (maxiters + 1) + i], i = 0 .. maxiters, = the (i + 1)-th UInt64 a COPY of run k's
 * rng yields (src/elbo.jl:2 draws L of them AFTER the optimisation, when L is known; here maxiters + 1 are drawn up front and the host
 * advances the run's rng by the L the path turned out to have).  The ELBO estimate of fit l (l = 1 .. L, slot k * (maxiters + 1) + l)
 * uses value l - 1; a later pfmi_pool_build_best(ctx, N_r, NULL) gives a FAILED run the value behind the ones it consumed, index L (what
 * rand(rng, fit_distribution, ndraws) would start from, src/singlepath.jl:231-233).
 * The calling thread SCHEDULES the dataflow: the optimiser (one workgroup per path) publishes its progress into page-locked host memory,
 * pfmi_stream_pump / pfmi_stream_wait launch the walk, fits and scan of each segment of trace positions once every path has produced it -- no
 * kernel ever waits for another.  After pfmi_stream_wait: pfmi_pool_build_best / pfmi_comm_psis_resample as usual, pfmi_get_fit_status and
 * pfmi_elbo_batch_wait return the slot arrays.
 * Accepted targets: the built-in ones (d <= 16384), and DEVICE_CALLBACK targets with a gradient closure (pfmi_set_target_gradient; any d the
 * memory check admits) -- the producer is then the closure optimiser of pfmi_optimize_batch, whose rounds the pump issues.  history_length
 * <= 16 and room for the fixed-stride layout in both cases; PFMI_ERR_UNSUPPORTED otherwise (device closures without a gradient, host
 * closures, history_length 17 .. 32: use the three calls above). */
int32_t pfmi_stream_enqueue(pfmi_ctx *ctx, int32_t K, const double *x0, int32_t history_length, int32_t maxiters, double g_tol,
                            double eps, int64_t N, const uint64_t *seeds);
/* seeds may be NULL in pfmi_stream_enqueue: the optimiser starts at once and the host draws the streams while it runs; pfmi_stream_seeds
 * hands them over before the first pfmi_stream_pump / pfmi_stream_wait (nothing but the optimiser is launched until then). */
int32_t pfmi_stream_seeds(pfmi_ctx *ctx, const uint64_t *seeds);
/* pfmi_stream_pump: ONE scheduling pass of the calling thread (never blocks): launches the walk, fits and scan of the trace positions every
 * path has produced since the last pass; *finished = 1 once the last segment and the reduction are enqueued.  pfmi_stream_wait pumps until
 * then and returns the points per path -- it does NOT wait for the GPU.  A host that drives several contexts pumps them in turn.
 * A closure target's closures are called from INSIDE pfmi_stream_pump / pfmi_stream_wait, on the calling thread: the gradient closure once per
 * optimiser round, with the pipeline's optimiser stream as its `stream` argument (at most 4 rounds in flight, at most maxiters * 55 + 1
 * rounds); the value closure once per block of draws of a segment's ELBO scan, with that segment's scan stream -- the context's own stream
 * or its second scan stream, alternating.  A closure must only enqueue on the stream it is handed.  pfmi_optimize_stats counts the rounds.
 * A pass that fails ends the call; an error of the optimiser's stream or the watchdog leaves the call to be drained by the next
 * pfmi_stream_cancel / pfmi_stream_enqueue / pfmi_set_traces / pfmi_optimize_batch_enqueue (this context's streams, never the device). */
int32_t pfmi_stream_pump(pfmi_ctx *ctx, int32_t *finished);
int32_t pfmi_stream_wait(pfmi_ctx *ctx, int64_t *npoints);
/* Give up an outstanding streaming call -- for a host that failed between pfmi_stream_enqueue and pfmi_stream_wait (an exception while it
 * drew the seed streams or pumped another context; the reference's task-based fan-out simply propagates the exception, src/multipath.jl:190-208).
 * Drains what is in flight, forgets the half-made results; the context is usable again.  No call outstanding: no-op.  (pfmi_stream_enqueue,
 * pfmi_set_traces and pfmi_optimize_batch_enqueue do the same implicitly when they find a stale call or one an error exit left undrained.)
 * A host whose closure failed inside pfmi_stream_pump cancels here. */
int32_t pfmi_stream_cancel(pfmi_ctx *ctx);

/* ---- fit_mvnormals / lbfgs_inverse_hessians / pdfactorize --------------------------------------- */
/* replaces fit_mvnormals (src/mvnormal.jl:14-21) = lbfgs_inverse_hessians (src/inverse_hessian.jl:25-66)
 * + lbfgs_inverse_hessian (:98-133) + WoodburyPDMat/pdfactorize (src/woodbury.jl:259-263, 201-207)
 * + mu = theta + Sigma*grad, for every point of every trace, batched on the GPU. */
int32_t pfmi_fit_batch(pfmi_ctx *ctx, int32_t history_length, double eps);
/* The `Hinit` keyword of lbfgs_inverse_hessians (src/inverse_hessian.jl:25, forwarded by fit_mvnormals, src/mvnormal.jl:14-16): how the
 * diagonal H0 is updated at every ACCEPTED step (:55).  A Julia closure cannot cross the boundary; the two the reference itself uses can:
 *   PFMI_HINIT_GILBERT            gilbert_init (src/inverse_hessian.jl:5-10), the default;
 *   PFMI_HINIT_SCALAR_YS_OVER_YY  (alpha, s, y) -> fill(y's / y'y): the Nocedal-Wright scaling Optim.LBFGS starts from, which the
 *                                 reference's own test passes as Hinit (test/inverse_hessian.jl:49, :62-66: H * grad is then the step
 *                                 the optimiser took).
 * pfmi_fit_batch_ex = pfmi_fit_batch with Hinit for THIS call; pfmi_set_hinit sets the context's default (pfmi_fit_batch and the
 * streaming pipeline use it). */
#define PFMI_HINIT_GILBERT 0
#define PFMI_HINIT_SCALAR_YS_OVER_YY 1
int32_t pfmi_fit_batch_ex(pfmi_ctx *ctx, int32_t history_length, double eps, int32_t hinit);
int32_t pfmi_set_hinit(pfmi_ctx *ctx, int32_t hinit);

/* status[P], j_eff[P] (effective history length), logdet[P], n_rejected[K]; any may be NULL */
int32_t pfmi_get_fit_status(pfmi_ctx *ctx, int32_t *status, int32_t *j_eff, double *logdet,
                            int64_t *n_rejected);

/* Materialise one fitted MvNormal{WoodburyPDMat} (so the host can build Sigma.A/.B/.D/.F.{U,Q,V}):
 * alpha[d]; B[d*2j]; D[2j*2j]; qr_factors[d*2j] + T[k*k] = QRCompactWY of U' \ B (Householder
 * vectors below the diagonal, R above; T upper triangular); V[k*k] upper Cholesky; mu[d]; k = min(d,2j).
 * Any output may be NULL. */
int32_t pfmi_get_fit(pfmi_ctx *ctx, int64_t point, double *alpha, double *B, double *D,
                     double *qr_factors, double *T, double *V, double *mu, double *logdet);

/* ---- maximize_elbo / elbo_and_samples / rand_and_logpdf ------------------------------------------ */
/* replaces maximize_elbo (src/elbo.jl:1-10) over fit_distributions[2:end] of every path:
 * for each point p that is not the first of its path: N draws x = mu + L u (src/mvnormal.jl:24-39),
 * logq, logp, ELBO mean and standard error (src/elbo.jl:12-20); then the NaN-skipping first-max
 * argmax per path (src/utils.jl:55-72).
 * seeds[P]: per-fit UInt64 seed (src/elbo.jl:2), keys the counter-based generator;
 * u_host: NULL (production: normals generated in-kernel) or P*d*N doubles, block p = the d x N
 *         standard normals of fit p (parity mode; blocks of first points are ignored);
 * elbo[P], se[P] (NaN for first points / failed fits), best_iter[K] (1-based iteration index
 * like the reference's fit_iteration; 0 when the path has no iterations). */
int32_t pfmi_elbo_batch(pfmi_ctx *ctx, int64_t N, const uint64_t *seeds, const double *u_host,
                        double *elbo, double *se, int64_t *best_iter);

/* The same in two halves (one host thread, several GPUs; or a host that wants to overlap its own work with the scan):
 * _enqueue uploads the seeds and launches the scan, the reduction and the per-path argmax without waiting (HOST_CALLBACK targets
 * evaluate on the calling thread, so for them _enqueue does the whole job); _wait blocks and downloads.  elbo / se / best_iter may
 * be NULL.  pfmi_elbo_batch == _enqueue + _wait. */
int32_t pfmi_elbo_batch_enqueue(pfmi_ctx *ctx, int64_t N, const uint64_t *seeds, const double *u_host);
int32_t pfmi_elbo_batch_wait(pfmi_ctx *ctx, double *elbo, double *se, int64_t *best_iter);

/* The reference's `ntasks` for HOST_CALLBACK targets (src/elbo.jl:3-6 and src/resample.jl:85-92 evaluate `logp` over tasks through
 * src/utils.jl:33-49; "the log-density function must be thread-safe", src/multipath.jl:104-108): with nthreads > 1 every staged block of
 * draws is cut into nthreads contiguous column ranges and `fn` is called on each range from its own host thread (one of them the calling
 * thread) -- `fn` must then be re-entrant and callable from threads the library creates; `user` is shared.  The results do not depend on
 * nthreads (same columns, one value per column; test/singlepath.jl:173-203).  Default 1.  A closure that parallelises internally (the
 * Julia trampoline with Threads.@threads) leaves this at 1. */
int32_t pfmi_set_callback_threads(pfmi_ctx *ctx, int32_t nthreads);

/* HOST_CALLBACK targets only: wall time spent inside the user's callback and bytes of draws handed to it (device -> pinned host)
 * during the last pfmi_elbo_batch.  The draws of a block of fits are generated and downloaded while the host evaluates the
 * previous block, so elbo_batch time ~ max(callback time, generation + PCIe time). */
int32_t pfmi_callback_stats(pfmi_ctx *ctx, double *callback_seconds, double *bytes_to_host);
/* DEVICE_CALLBACK targets: bytes of draws materialised in HBM for the callback during the last pfmi_elbo_batch (written once by the
 * draw kernel, read once by the user's kernel: 16 d bytes per draw physically move) */
int32_t pfmi_callback_stats_dev(pfmi_ctx *ctx, double *bytes_in_hbm);

/* per-draw log densities of one fit from the last pfmi_elbo_batch: logp[N], logq[N] */
int32_t pfmi_get_elbo_logs(pfmi_ctx *ctx, int64_t point, double *logp, double *logq);

/* draws n0 .. n0+N-1 of fit `point` (ELBOEstimate.draws, src/elbo.jl:19; also rand(rng, dist, n),
 * src/singlepath.jl:226-233): X[d*N], logp[N], logq[N]; u_host NULL or d*N normals. */
int32_t pfmi_draws(pfmi_ctx *ctx, int64_t point, uint64_t seed, int64_t n0, int64_t N,
                   const double *u_host, double *X, double *logp, double *logq);

/* Distributions.logpdf(MvNormal(mu_p, Sigma_p), X) for arbitrary X[d*N] through the factor
 * (src/resample.jl:85-89 -> src/woodbury.jl:378-382,158-165) */
int32_t pfmi_logpdf(pfmi_ctx *ctx, int64_t point, int64_t N, const double *X, double *out);

/* Distributions.logpdf(MixtureModel(components), X) without the log K, and componentwise_logpdf, for the uniform mixture of the
 * fits points[0..K-1] (repeats allowed) of this ctx:  comp[n + N k] = logpdf(fit points[k], X[:, n]) exactly as pfmi_logpdf defines
 * it (NaN for a fit whose status is not PFMI_FIT_OK), lse[n] = log sum_k exp(comp[n + N k]) in component order (NaN if any
 * component is NaN, -inf if all are -inf).  X[d*N] column-major; comp may be NULL (not wanted).  The host entry uploads X once for
 * all K components.  Not fitted: PFMI_ERR_STATE; K < 1, N < 1, a point outside [0, P) or NULL X / lse: PFMI_ERR_ARG. */
int32_t pfmi_mixture_logpdf(pfmi_ctx *ctx, int32_t K, const int64_t *points, int64_t N, const double *X, double *lse,
                            double *comp);
/* the same with X / lse / comp in device memory of the ctx's GPU, enqueued on the ctx stream: the caller orders the writes of X
 * before the call and calls pfmi_sync before reading lse / comp (points is a host array, read during the call). */
int32_t pfmi_mixture_logpdf_dev(pfmi_ctx *ctx, int32_t K, const int64_t *points, int64_t N, const void *X_dev, void *lse_dev,
                                void *comp_dev);

/* ---- remaining WoodburyPDMat / PDMats operator surface of a fitted covariance -------------- */
/* What the HMC integrations call on a fitted metric (ext/PathfinderAdvancedHMCExt.jl:17-23,
 * ext/PathfinderDynamicHMCExt.jl:7-15).  X is d x N column-major; out is d x N, or N values for the quadratic forms. */
#define PFMI_OP_UNWHITEN 0     /* unwhiten!(r, W, x) = L x            src/woodbury.jl:401-406, 136-143 */
#define PFMI_OP_WHITEN 1       /* whiten!(r, W, x)   = L \ x          src/woodbury.jl:410-415, 158-165 */
#define PFMI_OP_RMUL 2         /* R x  (lmul!(R, x))                  src/woodbury.jl:129-135          */
#define PFMI_OP_INVUNWHITEN 3  /* invunwhiten!(r, W, x) = R \ x       src/woodbury.jl:417-422, 151-157 */
#define PFMI_OP_MUL 4          /* mul!(y, W, x) = L (R x)             src/woodbury.jl:340-349, 64-68   */
#define PFMI_OP_SOLVE 5        /* W \ x = R \ (L \ x)                src/woodbury.jl:344, 70-74       */
#define PFMI_OP_QUAD 6         /* quad(W, x)    = |R x|^2 per column  src/woodbury.jl:384-397          */
#define PFMI_OP_INVQUAD 7      /* invquad(W, x) = |L \ x|^2           src/woodbury.jl:369-382          */
/* A fit whose status is not PFMI_FIT_OK has no factor: every entry of out (d x N, or the N quadratic forms) is NaN, whatever X holds,
 * as pfmi_mixture_logpdf reports such a component.  For a PFMI_FIT_OK fit a column of out depends on that column of X alone (one lane
 * per column): an all-zero column gives exact zeros (+0.0 for the quadratic forms) and a non-finite entry stays in its own column.
 * Launches are counted per instantiation under "woodbury:<KPAD>:<mode>" (pfmi_kernel_time; host-side counters like "hmc:..", ms = 0):
 * mode 0 unwhiten, 1 whiten, 2 R x, 3 invunwhiten; MUL = mode 2 then 0, SOLVE = mode 1 then 3, QUAD = mode 2, INVQUAD = mode 1. */
int32_t pfmi_woodbury_apply(pfmi_ctx *ctx, int64_t point, int32_t op, int64_t N, const double *X, double *out);
/* diag(W) = diag(A) + rowwise b' D b   (src/woodbury.jl:326-329); diag[d].  b is recomputed from the trace (theta, grad, the fit's
 * hist_src), not read from the stored B.  Every entry is NaN for a fit whose status is not PFMI_FIT_OK, as pfmi_woodbury_apply.
 * Counted under "woodbury_diag:<KPAD>". */
int32_t pfmi_woodbury_diag(pfmi_ctx *ctx, int64_t point, double *diag);

/* ---- static HMC with a fitted metric, for gradient closures ------------------------------------------------------------ */
/* "Use Pathfinder's metric estimate for sampling" (docs/src/examples/initializing-hmc.md, third way;
 * AdvancedHMC.RankUpdateEuclideanMetric(result.fit_distribution.Sigma), ext/PathfinderAdvancedHMCExt.jl:17-23), kept on the device: K
 * independent chains of static HMC -- nleapfrog leapfrog steps per transition, Metropolis correction, full momentum refresh; no NUTS.
 * Chain k uses the Woodbury factor of fit points[k] as its metric and the ctx's DEVICE_CALLBACK target with its gradient closure
 * (pfmi_set_target_gradient); built-in targets, host closures and device closures without a gradient: PFMI_ERR_UNSUPPORTED.
 *
 * The transition.  Sigma = L R, R = L' (L = PFMI_OP_UNWHITEN, R = PFMI_OP_RMUL); the momentum is carried whitened, v = R p ~ N(0, I).
 * Per chain: the point x, lp = logp(x), wg = R grad logp(x), v, the trial point x~, the transition counter t.  Transition t with step size
 * e, Lf = nleapfrog and the chain's seed s:
 *   1. v <- the d standard normals of draw index t under seed s (the library's generator, stream 0);  H0 = -lp + |v|^2 / 2
 *   2. v <- v + (e/2) wg;  x~ <- x + e L v
 *   3. for i = 1 .. Lf: the closure gives (lp~, g~) at x~, w~ = R g~;  i < Lf: v <- v + e w~, x~ <- x~ + e L v;  i = Lf: v <- v + (e/2) w~
 *   4. H1 = -lp~ + |v|^2 / 2,  a = min(1, exp(H0 - H1)).  A non-finite lp~, g~ or H1, or H1 - H0 > 1000: a = 0 and the transition is
 *      divergent; the trial never enters the state (nothing non-finite is ever stored in x, lp, wg)
 *   5. u = (rand_u64(s, t, stream 3) >> 11) 2^-53 (pfmi_host_rand_u64's generator);  accept iff u < a:  (x, lp, wg) <- (x~, lp~, w~)
 *   6. row t records x, lp, a, H1 - H0 (DBL_MAX when it is not finite) and the divergent flag.
 * The closure cannot be called from a kernel, so a run is 1 + T Lf ROUNDS (the first evaluates the start points): one call of the closure
 * on all K trial points (d x K, with the ctx's stream as its `stream`), then one launch of the step kernel, one workgroup per chain.  The
 * round count is known up front: _enqueue issues every round from the calling thread and returns without waiting.  A chain's output
 * depends on its own inputs alone (not on K, not on the other chains).
 * x0: d x K column-major start points; seeds, step_size: K values; points: K fit points (0-based, any path). */
#define PFMI_HMC_CONTINUE 1      /* go on from the chains' resident states and counters; x0 ignored (may be NULL) */
#define PFMI_HMC_RECORD_PATH 2   /* keep every round's X, closure output and v (tests / diagnostics) */
/* PFMI_ERR_STATE: not fitted, or CONTINUE without K resident chains.  PFMI_ERR_UNSUPPORTED: no gradient closure.  PFMI_ERR_ARG: K < 1, a
 * point outside [0, P), a step size that is not positive and finite, nleapfrog < 1, ntransitions < 1, a NULL required pointer.
 * PFMI_ERR_NUMERIC: a point whose fit status is not PFMI_FIT_OK.  An error drains this ctx's stream before returning.  pfmi_set_target,
 * pfmi_set_target_gradient, pfmi_set_traces, a new fit, pfmi_optimize_batch_enqueue and pfmi_stream_enqueue forget the chains.
 * Stage names under pfmi_profile: "hmc" (the step kernel), "hmc_closure" (the closure's kernels); "hmc:<KPAD>:<res|stream>" counts the step
 * launches of one plan -- column padding KPAD (4 .. 64), the chain's factor rows staged in LDS or streamed from HBM. */
int32_t pfmi_hmc_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                         int32_t nleapfrog, int64_t ntransitions, int32_t flags);
/* waits for the rounds (AbstractMCMC's sample loop has returned).  PFMI_ERR_NUMERIC: a start point with a non-finite log density or
 * gradient (the chains are forgotten).  PFMI_ERR_STATE without a run. */
int32_t pfmi_hmc_wait(pfmi_ctx *ctx);
/* The last call's T = ntransitions rows of every chain (the chain of AdvancedHMC.sample, docs/src/examples/initializing-hmc.md): draws
 * (d, T, K) column-major like the pool; logp, accept_prob, energy_error, divergent [K][T].  Any may be NULL.  Waits. */
int32_t pfmi_hmc_get(pfmi_ctx *ctx, double *draws, double *logp, double *accept_prob, double *energy_error, int32_t *divergent);
/* device pointer to those draws (K T columns of d doubles; valid until the next pfmi_hmc_enqueue); *count = K T */
int32_t pfmi_hmc_draws_dev(pfmi_ctx *ctx, void **dev_ptr, int64_t *count);
/* PFMI_HMC_RECORD_PATH: rounds round0 .. round0 + nrounds - 1 of the last call -- X (d, K, nrounds) the closure's input of the round,
 * closure_out (K + d K, nrounds) its output (logp [K], then grad (d, K)), v (d, K, nrounds) the whitened momenta after the round's launch.
 * Any may be NULL.  No reference counterpart (AdvancedHMC keeps no leapfrog path). */
int32_t pfmi_hmc_get_path(pfmi_ctx *ctx, int64_t round0, int64_t nrounds, double *X, double *closure_out, double *v);
/* rounds and columns handed to the closure by the last pfmi_hmc_enqueue (pfmi_optimize_stats' counterpart) */
int32_t pfmi_hmc_stats(pfmi_ctx *ctx, int64_t *rounds, int64_t *closure_columns);

/* ---- NUTS with a fitted metric, for gradient closures ------------------------------------------------------------------------ */
/* The sampler the reference's worked example hands Pathfinder's metric to (docs/src/examples/initializing-hmc.md,
 * ext/PathfinderAdvancedHMCExt.jl, ext/PathfinderDynamicHMCExt.jl): K independent chains of multinomial NUTS (Betancourt 2017) with the
 * iterative tree builder (checkpoints instead of recursion), on the device, with the metric, the whitened momentum, the target and the
 * points of pfmi_hmc_enqueue.  No trajectory length to choose: transition t doubles its trajectory until it turns.
 *   v0 = the normals of draw t under the chain's seed, H0 = -lp + |v0|^2 / 2; the tree is the leaf (x, v0), log-weight 0, rho = v0.
 *   Doubling j = 0, 1, ..: dir = +1 iff the top bit of rand_u64(s, 16 t + j, stream 4); a sub-tree of 2^j leaves grows from the tree's end
 *   in that direction by leapfrog steps of size dir e.  Leaf n (0-based) with momentum v, energy H = -lp~ + |v|^2 / 2, lw = H0 - H:
 *     - divergent (non-finite lp~, g~ or H, or H - H0 > 1000): the sub-tree is discarded and the transition ends;
 *     - rho_s += v; the leaf replaces the sub-tree's candidate iff u < exp(lw - logaddexp(logW_s, lw)), u = (rand_u64(s, 1024 t + m,
 *       stream 6) >> 11) 2^-53 with m the leaves made before it in this transition; logW_s <- logaddexp(logW_s, lw);
 *     - imax = popcount(n >> 1); an even n stores (v, rho_s) as checkpoint imax; an odd n checks the checkpoints imax down to
 *       imax - (trailing one-bits of n) + 1: with rho_sub = rho_s - rho_ck[i] + v_ck[i], a turn when rho_sub . v_ck[i] <= 0 or
 *       rho_sub . v <= 0: the sub-tree is discarded and the transition ends.
 *   A completed sub-tree's candidate replaces the tree's iff u < exp(logW_s - logW), u from rand_u64(s, 16 t + j, stream 5); then
 *   logW <- logaddexp(logW, logW_s), rho += rho_s; the transition ends when rho . v- <= 0 or rho . v+ <= 0 (the momenta at the two ends), or
 *   when j + 1 == max_depth.  The tree's candidate becomes the state and row t.
 * Rows (shared with static HMC: pfmi_hmc_get, pfmi_hmc_draws_dev and pfmi_chain_diagnostics(PFMI_CHAIN_SRC_HMC) serve a NUTS run after its
 * wait): accept_prob is the mean over the transition's leaves of min(1, exp(H0 - H_leaf)) (a divergent leaf counts 0), energy_error is
 * H(selected) - H0, divergent as above.
 * One ROUND is one call of the closure on all K columns and one launch of the step kernel: one leapfrog step of every running chain.  The
 * round count is not known up front: _enqueue issues a first window of rounds and returns; pfmi_nuts_pump issues more, a bounded window
 * ahead of the last progress word read from the device, never beyond the cap (fresh ? 1 : 0) + T (2^max_depth - 1).  Chains run
 * asynchronously: one that ends a transition opens its next in the same launch; one that has made its T transitions idles (its column of X
 * stays its state: the closure is still called on it).  A chain's output depends on its own inputs alone.
 * Errors are pfmi_hmc_enqueue's; also PFMI_ERR_ARG for max_depth outside 1 .. 10, PFMI_ERR_STATE for CONTINUE on static-HMC chains (and
 * PFMI_HMC_CONTINUE on NUTS chains), PFMI_ERR_UNSUPPORTED when the buffers (with RECORD_PATH: one path row per round of the cap) do not fit.
 * Stage names: "nuts", "nuts_closure"; "nuts:<KPAD>:<res|stream>" counts the step launches of one plan. */
#define PFMI_NUTS_CONTINUE 1
#define PFMI_NUTS_RECORD_PATH 2
int32_t pfmi_nuts_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                          int32_t max_depth, int64_t ntransitions, int32_t flags);
/* one scheduling pass from the calling thread: never blocks.  *finished = 1 once every chain has made its transitions. */
int32_t pfmi_nuts_pump(pfmi_ctx *ctx, int32_t *finished);
/* pumps until finished, then waits for the stream.  PFMI_ERR_NUMERIC: a start point with a non-finite log density or gradient (the chains
 * are forgotten).  PFMI_ERR_STATE without a NUTS run. */
int32_t pfmi_nuts_wait(pfmi_ctx *ctx);
/* tree_depth (doublings made, the discarded one included) and n_leapfrog (leaves made) of the last call's transitions, int32 [K][T] */
int32_t pfmi_nuts_get_stats(pfmi_ctx *ctx, int32_t *tree_depth, int32_t *n_leapfrog);
/* what one round decided for one chain (PFMI_NUTS_RECORD_PATH); t = -1: the round evaluated the start point, or the chain was idle */
typedef struct {
    int32_t t, j, n, dir;           /* transition, doubling, leaf of the sub-tree, direction */
    int32_t leaf, flags;            /* leaves made before this one in the transition; PFMI_NUTS_EV_* */
    double H_leaf, logW_s, logW, H0;/* the leaf's energy; both log weights after the round's updates; the tree's root energy */
} pfmi_nuts_event;
#define PFMI_NUTS_EV_DIVERGENT 1
#define PFMI_NUTS_EV_SUBTREE_TURN 2
#define PFMI_NUTS_EV_LEAF_TAKEN 4      /* the leaf replaced the sub-tree's candidate */
#define PFMI_NUTS_EV_SUBTREE_DONE 8    /* the sub-tree was completed and merged */
#define PFMI_NUTS_EV_TREE_TAKEN 16     /* its candidate replaced the tree's */
#define PFMI_NUTS_EV_TREE_TURN 32
#define PFMI_NUTS_EV_MAX_DEPTH 64
#define PFMI_NUTS_EV_END 128           /* the transition ended in this round */
/* PFMI_NUTS_RECORD_PATH: rounds round0 .. round0 + nrounds - 1 of the last call (nrounds at most pfmi_nuts_stats' rounds): X and
 * closure_out as pfmi_hmc_get_path gives them; v (d, K, nrounds) the synchronised whitened momentum of the leaf the round finished (0 in the
 * start round); events [nrounds][K].  Columns of idle chains are not written.  Any may be NULL. */
int32_t pfmi_nuts_get_path(pfmi_ctx *ctx, int64_t round0, int64_t nrounds, double *X, double *closure_out, double *v, pfmi_nuts_event *events);
/* rounds until the last chain went idle, and the columns handed to the closure: K per round issued, idle chains' columns and the rounds
 * issued ahead of the last progress word included */
int32_t pfmi_nuts_stats(pfmi_ctx *ctx, int64_t *rounds, int64_t *closure_columns);

/* ---- device-resident warm-up: step-size adaptation inside static HMC and NUTS ---------------------------------------------------- */
/* What the samplers the reference hands the metric to do during warm-up (AdvancedHMC's StepSizeAdaptor / StanHMCAdaptor, DynamicHMC's
 * dual averaging): the step size of every chain is updated after EVERY warm-up transition, here by the launch that ends the transition,
 * so that one enqueue runs nwarmup = W warm-up and ntransitions = T sampling transitions back to back with no host round trip in between.
 * Nesterov dual averaging (Hoffman & Gelman 2014, Algorithm 5; gamma = 0.05, t0 = 10, kappa = 0.75), per chain and per transition.  a_t is
 * the acceptance statistic of warm-up transition t (0-based, t < W) -- exactly the row's accept_prob, so 0 for a divergent transition.  With
 * m = t + 1, the target delta = target_accept and mu = log(10 eps_0):
 *     Hbar <- (1 - 1/(m + t0)) Hbar + (delta - a_t)/(m + t0)        Hbar_0 = 0
 *     le    = mu - (sqrt(m)/gamma) Hbar
 *     w     = m^(-3/4) = 1 / (sqrt(m) sqrt(sqrt(m)))                (no pow)
 *     leb  <- w le + (1 - w) leb                                     leb_0 = 0
 * Transition t + 1 uses exp(le) while t + 1 < W; every transition t >= W uses exp(leb_W).  An update that yields a step size that is zero
 * or not finite leaves the chain the step size it has and sets PFMI_ADAPT_KEPT_STEP in the chain's status.  There is no initial step-size
 * search and no clamp.
 * Rows: the warm-up transitions write none.  pfmi_hmc_get, pfmi_hmc_draws_dev, pfmi_nuts_get_stats and pfmi_chain_diagnostics(SRC_HMC) see
 * the T sampling transitions W .. W + T - 1 as rows 0 .. T - 1; the random numbers of transition t are those of transition t of a plain
 * run.  A later plain PFMI_HMC_CONTINUE / PFMI_NUTS_CONTINUE goes on from transition W + T with the step sizes it is given.
 * flags must be 0 (an adaptive run is a fresh run; no CONTINUE, no RECORD_PATH): anything else, nwarmup < 1 or target_accept outside (0, 1)
 * is PFMI_ERR_ARG; every other error is that of pfmi_hmc_enqueue / pfmi_nuts_enqueue.  Every error, a refused argument included, drains
 * this ctx's stream and leaves no chains and no traces behind.  Waiting and reading stay pfmi_hmc_wait,
 * pfmi_nuts_pump / pfmi_nuts_wait and pfmi_hmc_get; the NUTS cap is 1 + (W + T) (2^max_depth - 1) rounds.
 * Stage names: "hmc_adapt", "hmc_adapt_closure", "nuts_adapt", "nuts_adapt_closure"; "hmc_adapt:<KPAD>:<res|stream>" and
 * "nuts_adapt:<KPAD>:<res|stream>" count the launches of one plan of the warm kernels (the plain runs' counters are untouched). */
#define PFMI_ADAPT_KEPT_STEP 1   /* status bit: an update gave a step size that was zero or not finite; the chain kept its previous one */
int32_t pfmi_hmc_adapt_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds,
                               const double *step_size0, int32_t nleapfrog, int64_t nwarmup, int64_t ntransitions, double target_accept,
                               int32_t flags);
int32_t pfmi_nuts_adapt_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds,
                                const double *step_size0, int32_t max_depth, int64_t nwarmup, int64_t ntransitions, double target_accept,
                                int32_t flags);
/* ---- static HMC on the built-in targets: whole runs in one persistent kernel ------------------------------------------------ */
/* pfmi_hmc_enqueue and pfmi_hmc_adapt_enqueue for a ctx whose target is PFMI_TARGET_GAUSS (any rank) or PFMI_TARGET_FUNNEL.  The library
 * knows the density, so nothing is cut into closure rounds: one workgroup per chain evaluates logp and its gradient in the kernel and loops
 * over the rounds, with the chain's factor rows staged in LDS once per launch.  No launch makes more than 1024 rounds (csrc/hmc_rows.h:
 * HM_FUSED_ROUNDS; the hook PFMI_HMC_FUSED_ROUNDS of pfmi_debug_set overrides it): a longer call is several launches that re-enter from the
 * chains' resident state -- in mid-trajectory too -- and give the same bits whatever the cut.  No kernel waits for another.
 * nwarmup == 0: the transition of pfmi_hmc_enqueue, steps 1 - 6 above, with the in-kernel value and gradient in the closure's place: the
 * same normals, acceptance uniform, divergence rule and rows; flags: PFMI_HMC_CONTINUE, PFMI_HMC_RECORD_PATH; target_accept is ignored.
 * nwarmup >= 1: the run of pfmi_hmc_adapt_enqueue (dual averaging after every warm-up transition, the traces of pfmi_adapt_get, exp(leb)
 * for sampling); flags must be 0 and target_accept in (0, 1).  nwarmup < 0: PFMI_ERR_ARG.
 * The run is a static-HMC run in the same buffers and layouts: pfmi_hmc_wait, pfmi_hmc_get, pfmi_hmc_draws_dev, pfmi_hmc_get_path (the
 * closure_out rows hold the in-kernel value and gradient), pfmi_adapt_get and pfmi_chain_diagnostics(PFMI_CHAIN_SRC_HMC) serve it;
 * pfmi_hmc_stats reports rounds = (fresh ? 1 : 0) + (nwarmup + ntransitions) nleapfrog evaluations and closure_columns = 0.
 * Errors are those of pfmi_hmc_enqueue / pfmi_hmc_adapt_enqueue, in their order and with the drain-on-error rule, except that
 * PFMI_ERR_UNSUPPORTED is returned for any callback target (a DEVICE_CALLBACK target with a gradient closure runs through pfmi_hmc_enqueue)
 * and for a staged scale (pfmi_chain_scale_set: pfmi_hmc_fused_metric_enqueue takes it).
 * NUTS on a built-in target is pfmi_nuts_fused_enqueue below; the metric windows and scaled chains are pfmi_hmc_fused_metric_enqueue.
 * Out of scope: ChEES; pfmi_hmc_enqueue, pfmi_nuts_enqueue, the adaptive enqueues and pfmi_chees_enqueue are unchanged and still refuse a built-in target.
 * Stage name "hmc_fused"; plan counters "hmc_fused:<KPAD>:<res|stream>:<f|g0|g8|g16>" (pfmi_kernel_time). */
int32_t pfmi_hmc_fused_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds,
                               const double *step_size, int32_t nleapfrog, int64_t nwarmup, int64_t ntransitions, double target_accept,
                               int32_t flags);
/* ---- NUTS on the built-in targets: whole runs in one persistent kernel ------------------------------------------------------- */
/* pfmi_nuts_enqueue and pfmi_nuts_adapt_enqueue for a ctx whose target is PFMI_TARGET_GAUSS (any rank) or PFMI_TARGET_FUNNEL.  One
 * workgroup per chain loops over TRIPS: it evaluates logp and its gradient at the trial point in the kernel, then makes the NUTS round
 * of pfmi_nuts_enqueue (one leaf of the tree, its checkpoints and decisions, the end of a transition, the opening of the next and the
 * drift to the next trial point), with the chain's factor rows staged in LDS once per launch.  A chain builds its trees at its own pace
 * and leaves the launch when it has made its transitions.  No launch makes more than 1024 trips per chain (csrc/hmc_rows.h:
 * HM_FUSED_ROUNDS; the hook PFMI_NUTS_FUSED_ROUNDS of pfmi_debug_set overrides it): a longer call is several launches that re-enter from
 * the chains' resident state -- in mid-tree too -- and give the same bits whatever the cut.  No kernel waits for another.
 * nwarmup == 0: the transition of pfmi_nuts_enqueue with the in-kernel value and gradient in the closure's place: the same normals,
 * directions, uniforms (stream for stream, counter for counter), divergence rule and rows; flags: PFMI_NUTS_CONTINUE,
 * PFMI_NUTS_RECORD_PATH; target_accept is ignored.  The opening trip of a CONTINUE evaluates nothing and writes no path row.
 * nwarmup >= 1: the run of pfmi_nuts_adapt_enqueue; flags must be 0 and target_accept in (0, 1).  nwarmup < 0: PFMI_ERR_ARG.
 * The device decides how many launches a call takes, so they are pumped like the closure route's rounds: pfmi_nuts_enqueue's window of
 * launches ahead of the last progress word read (launch << 32 | chains still running), at most
 * ceil(((fresh ? 1 : 0) + (nwarmup + ntransitions) (2^max_depth - 1)) / cap) launches; a run that fits one launch is exactly one.
 * The run is a NUTS run in the same buffers and layouts: pfmi_nuts_wait, pfmi_nuts_pump, pfmi_nuts_get_stats, pfmi_nuts_get_path,
 * pfmi_hmc_get, pfmi_hmc_draws_dev, pfmi_adapt_get and pfmi_chain_diagnostics(PFMI_CHAIN_SRC_HMC) serve it.  pfmi_nuts_stats reports
 * rounds = the most trips a chain made (a fresh call: 1 + the largest per-chain sum of n_leapfrog) and closure_columns = 0.  A path row
 * is a TRIP of the chain, not a launch: pfmi_nuts_get_path takes rows [0, rounds), the closure_out rows hold the in-kernel value and
 * gradient, and a chain's rows beyond its own trips keep event t = -1.
 * Errors are those of pfmi_nuts_enqueue / pfmi_nuts_adapt_enqueue, in their order and with the drain-on-error rule, except that
 * PFMI_ERR_UNSUPPORTED is returned for any callback target (a DEVICE_CALLBACK target with a gradient closure runs through
 * pfmi_nuts_enqueue) and for a staged scale or resident scaled chains (pfmi_nuts_fused_metric_enqueue takes them).  PFMI_NUTS_CONTINUE on the
 * chains of another sampler -- pfmi_hmc_fused_enqueue's included -- is PFMI_ERR_STATE, with max_depth above the chains' PFMI_ERR_ARG.
 * Fused and closure NUTS calls never meet on the same resident chains: replacing the target forgets the chains.
 * Out of scope: ChEES (its chains talk to each other); the metric windows and scaled chains are pfmi_nuts_fused_metric_enqueue.
 * Stage name "nuts_fused"; plan counters "nuts_fused:<KPAD>:<res|stream>:<f|g0|g8|g16>", one count per launch (pfmi_kernel_time). */
int32_t pfmi_nuts_fused_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds,
                                const double *step_size, int32_t max_depth, int64_t nwarmup, int64_t ntransitions, double target_accept,
                                int32_t flags);
/* The last adaptive run: step_size [K] the one its sampling transitions used (a later plain CONTINUE with step sizes of the caller's own
 * does not change what is reported here); eps_trace, accept_trace [K][W] the step size warm-up transition
 * t used and its a_t; divergent, n_leapfrog int32 [K][W]; status [K] (PFMI_ADAPT_*).  Any may be NULL.  Waits for the stream (a NUTS run
 * must be finished: pfmi_nuts_wait).  PFMI_ERR_STATE without an adaptive run: whatever forgets the chains forgets the traces. */
int32_t pfmi_adapt_get(pfmi_ctx *ctx, double *step_size, double *eps_trace, double *accept_trace, int32_t *divergent, int32_t *n_leapfrog,
                       int32_t *status);
/* The host build of the update the warm kernels run (one source, csrc/adapt.h): n updates on accept[0 .. n - 1] from eps0.  eps [n + 1]:
 * eps[0] = eps0, eps[m] the step size after m updates (exp(le_m), or eps[m - 1] where that is zero or not finite); eps_bar [n] (may be
 * NULL): exp(leb_m) at index m - 1.  Needs no GPU and no ctx. */
int32_t pfmi_host_dual_averaging(int64_t n, double eps0, double target_accept, const double *accept, double *eps, double *eps_bar);

/* ---- device-resident warm-up: windowed metric adaptation on the Woodbury factor ---------------------------------------------------- */
/* The second way the reference's worked example hands a Pathfinder result to HMC (docs/src/examples/initializing-hmc.md: "initialise a
 * metric adaptation" from the fitted covariance), as Stan's windowed adaptation, AdvancedHMC's StanHMCAdaptor and DynamicHMC's
 * default_warmup_stages run it, carried out in the coordinates whitened by the fit's factor.  Chain k keeps the factor of its fit point,
 * Sigma_p = L R, and in addition a per-coordinate SCALE c_k (d positive doubles):
 *     Sigma_k = L diag(c_k)^2 L'            a kick is v += e c . (R g), a drift x += e L (c . v)
 * The momentum stays whitened, v ~ N(0, I), and nothing else of a transition changes; c = 1 is the fitted metric.
 * The windows of W = nwarmup warm-up transitions (one rule for host and device, csrc/adapt.h; pfmi_adapt_windows):
 *     W < 20     no window: the run is pfmi_*_adapt_enqueue's and PFMI_ADAPT_NO_METRIC_WINDOW is set in every chain's status.
 *     otherwise  init = 75, term = 50, base = 25; if init + base + term > W: init = floor(0.15 W), term = floor(0.10 W),
 *                base = W - init - term.  end = W - term.  Windows are consecutive from init; one of nominal size s that starts at e ends at
 *                e + s, or at `end` if e + s + 2 s - 1 >= end; the next nominal size is 2 s.  (Stan's rule, except that the first window
 *                takes the stretch test of the others.)
 * After every transition of a window, accepted or not, the chain forms u = L \ (x - x0) -- PFMI_OP_WHITEN with the FIT's factor, so that
 * an estimate replaces the scale and does not compound it; x0 its start point -- and every coordinate takes one Welford update of its
 * running mean and M2.  At the end of a window of n transitions
 *     D_i = (n / (n + 5)) M2_i / (n - 1) + 5 / (n + 5),        c_i = sqrt(D_i)
 * (shrinkage towards 1, the fitted metric).  If any D_i is not finite or not positive the chain keeps its scale and
 * PFMI_ADAPT_KEPT_METRIC is set.  The Welford state is cleared and the dual averaging restarts: m = 0, Hbar = leb = 0, mu = log(10 eps),
 * eps the step size the ordinary update after this transition proposes (which the next transition uses).  The `term` transitions after
 * the last window adapt the step size alone; sampling uses exp(leb) as in pfmi_*_adapt_enqueue.
 * Stage names: "hmc_metric", "hmc_metric_closure", "nuts_metric", "nuts_metric_closure"; "hmc_metric:<KPAD>:<res|stream>" and
 * "nuts_metric:<KPAD>:<res|stream>" count the launches of one plan of the metric kernels, which step every chain that carries a scale, in
 * a plain run or an adaptive one (the counters of the plain and the _adapt plans are untouched). */
#define PFMI_ADAPT_NO_METRIC_WINDOW 2   /* status bit: nwarmup < 20, the warm-up adapted the step size alone */
#define PFMI_ADAPT_KEPT_METRIC 4        /* status bit: a window gave a variance that was not positive and finite; the chain kept its scale */
#define PFMI_ADAPT_RECORD_WHITENED 4    /* flag: keep the u of every window transition (tests / diagnostics, as PFMI_HMC_RECORD_PATH is) */
#define PFMI_ADAPT_MAX_WINDOWS 32       /* no nwarmup below 2^31 has more windows */
/* Stages scale [K][d] for the next pfmi_hmc_enqueue / pfmi_nuts_enqueue (or adaptive enqueue) with that K, a fresh run or a CONTINUE,
 * where it becomes the chains' resident scale.  A CONTINUE without a staged scale keeps the resident one; a fresh run without one has
 * none and launches the plain kernels.  scale NULL clears the staging.  PFMI_ERR_ARG: a value that is not positive and finite, K < 1
 * (as a refused enqueue, this drains the ctx's stream and leaves no chains); an enqueue whose K is not the staged K returns PFMI_ERR_ARG.
 * Whatever forgets the chains forgets the scale, staged or resident. */
int32_t pfmi_chain_scale_set(pfmi_ctx *ctx, int32_t K, const double *scale);
/* pfmi_hmc_adapt_enqueue / pfmi_nuts_adapt_enqueue with the metric windows above.  The chains start from a staged scale, or from c = 1.
 * flags: 0 or PFMI_ADAPT_RECORD_WHITENED (PFMI_ERR_UNSUPPORTED when the rows do not fit).  Errors and the drain-on-error rule are those
 * of pfmi_*_adapt_enqueue; nwarmup >= 2^31 is PFMI_ERR_UNSUPPORTED.  After the run the resident scale is the last window's: a later plain
 * CONTINUE samples with the adapted metric.  pfmi_adapt_get serves the step-size traces over all W transitions (a restart shows as the
 * step size the update before it proposed), the final step size and the status bits. */
int32_t pfmi_hmc_adapt_metric_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds,
                                      const double *step_size0, int32_t nleapfrog, int64_t nwarmup, int64_t ntransitions,
                                      double target_accept, int32_t flags);
int32_t pfmi_nuts_adapt_metric_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds,
                                       const double *step_size0, int32_t max_depth, int64_t nwarmup, int64_t ntransitions,
                                       double target_accept, int32_t flags);
/* The last run of those two: *nwindows; ends [nwindows] (room for PFMI_ADAPT_MAX_WINDOWS, or for what pfmi_adapt_windows gives) the
 * windows' exclusive ends; scale_trace [K][nwindows][d] the scale each window left (the kept one under PFMI_ADAPT_KEPT_METRIC); whitened
 * [K][ends[nwindows - 1] - init][d] the u of every window transition (PFMI_ERR_STATE if the run did not record them).  Any may be NULL.
 * Waits as pfmi_adapt_get does.  PFMI_ERR_STATE without such a run. */
int32_t pfmi_adapt_metric_get(pfmi_ctx *ctx, int32_t *nwindows, int64_t *ends, double *scale_trace, double *whitened);
/* ---- the scale and the metric windows on the built-in targets: whole runs in one persistent kernel ----------------------------- */
/* pfmi_hmc_fused_enqueue / pfmi_nuts_fused_enqueue for chains that carry a per-coordinate scale, and the metric windows above, for a ctx
 * whose target is PFMI_TARGET_GAUSS or PFMI_TARGET_FUNNEL: the loops of the fused kernels around the round of the metric kernels
 * (csrc/hmc_fused_metric_kernel.hip, csrc/nuts_fused_metric_kernel.hip).  The end of a window writes the chain's scale and the next kick
 * reads it inside ONE launch; whatever the cut into launches (HM_FUSED_ROUNDS and its hooks, as they are), the bits are the same.
 * nwarmup == 0: a plain run; flags: PFMI_*_CONTINUE, PFMI_*_RECORD_PATH.  A scale staged by pfmi_chain_scale_set becomes the chains'
 *   resident one, a CONTINUE goes on with the one the chains carry; chains that carry a scale are stepped by the fused-metric kernels,
 *   chains without one by the fused kernels.  With a staged scale of ones the draws are the bits of pfmi_*_fused_enqueue.
 * nwarmup >= 1: a fresh adaptive run with the metric windows of pfmi_*_adapt_metric_enqueue (same windows, same rule, same restarts of
 *   the dual averaging, same status bits, a staged scale is the start scale); flags: 0 or PFMI_ADAPT_RECORD_WHITENED; target_accept in
 *   (0, 1).  nwarmup < 20 without a staged scale has no window: the run is pfmi_*_fused_enqueue's step-size warm-up, on the fused kernels,
 *   with PFMI_ADAPT_NO_METRIC_WINDOW set.  nwarmup < 0: PFMI_ERR_ARG.
 * Checks, their order, the drain-on-error rule, the launches' schedule (NUTS: pumped) and everything that serves the run are those of
 * pfmi_hmc_fused_enqueue / pfmi_nuts_fused_enqueue, plus pfmi_adapt_metric_get for a run with nwarmup >= 1.  A callback target is
 * PFMI_ERR_UNSUPPORTED (a DEVICE_CALLBACK target with a gradient closure runs through pfmi_hmc_adapt_metric_enqueue /
 * pfmi_nuts_adapt_metric_enqueue, or pfmi_chain_scale_set in front of pfmi_hmc_enqueue / pfmi_nuts_enqueue).  pfmi_hmc_fused_enqueue and
 * pfmi_nuts_fused_enqueue keep refusing a staged scale and a CONTINUE of chains that carry one.  Out of scope: ChEES.
 * Stage names "hmc_fused_metric", "nuts_fused_metric"; plan counters "hmc_fused_metric:<KPAD>:<res|stream>:<f|g0|g8|g16>" and
 * "nuts_fused_metric:...", one count per launch (pfmi_kernel_time). */
int32_t pfmi_hmc_fused_metric_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds,
                                      const double *step_size, int32_t nleapfrog, int64_t nwarmup, int64_t ntransitions,
                                      double target_accept, int32_t flags);
int32_t pfmi_nuts_fused_metric_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds,
                                       const double *step_size, int32_t max_depth, int64_t nwarmup, int64_t ntransitions,
                                       double target_accept, int32_t flags);
/* Host builds of the device's sources (csrc/adapt.h), as pfmi_host_dual_averaging is; no GPU, no ctx.
 * pfmi_adapt_windows: the windows of nwarmup transitions -- *init the first window's start, *term the transitions after the last,
 * ends [*nwindows] (nwarmup < 20: no window, *init = nwarmup, *term = 0).  PFMI_ERR_ARG: nwarmup < 1, a NULL pointer, cap too small.
 * pfmi_host_metric_update: the scale a window of n >= 2 rows u [n][d] leaves -- scale_out = sqrt(D), or scale_in with *status =
 * PFMI_ADAPT_KEPT_METRIC when a D_i is not positive and finite. */
int32_t pfmi_adapt_windows(int64_t nwarmup, int64_t *init, int64_t *term, int64_t *ends, int32_t cap, int32_t *nwindows);
int32_t pfmi_host_metric_update(int64_t n, int32_t d, const double *u, const double *scale_in, double *scale_out, int32_t *status);

/* ---- ChEES-HMC: a shared step size and a trajectory length learned across the chains ------------------------------------------------- */
/* Hoffman, Radul & Sountsov (2021), for many chains resident on one device.  Every transition is pfmi_hmc_enqueue's (steps 1 - 6 above,
 * the same generators, streams and draw indices, chain k on its own fit point's factor) with ONE step size e and ONE leapfrog count for
 * all chains, so the chains run in lockstep and no closure column is wasted; what static HMC makes the caller guess, the trajectory
 * length tau, is learned during the warm-up from a statistic ACROSS the chains.  The rule (one source for host and device, csrc/adapt.h):
 *   transition t (0-based, over warm-up and sampling, carried across CONTINUE):  h_t = the base-2 radical inverse of t + 1 (the 32-bit
 *   integer bit-reversed, times 2^-32: 1/2, 1/4, 3/4, 1/8, ...);  n = ceil((h_t tau) / e);  L_t = min(max(n, 1), max_leapfrog);  n >
 *   max_leapfrog sets PFMI_CHEES_CLAMPED.
 *   After warm-up transition t < W, with x_k the state before it, x'_k the trial point at its end, a_k its accept_prob (0 when divergent)
 *   and u'_k = L_k v'_k the x-space velocity at its end (v'_k the whitened momentum after the last half kick) -- sums over chains in chain
 *   order, chains with a_k = 0 LEFT OUT (their x' may be non-finite), sums over coordinates fixed-order block sums:
 *     A = sum_k a_k;  xbar_i = (sum_k x_k,i) / K;  xbar'_i = (sum_k a_k x'_k,i) / A
 *     p_k = sum_i (x_k,i - xbar_i)^2;  q_k = sum_i (x'_k,i - xbar'_i)^2;  r_k = sum_i (x'_k,i - xbar'_i) u'_k,i
 *     g = h_t tau (sum_k a_k (q_k - p_k) r_k) / A                       (the gradient of the ChEES criterion with respect to log tau)
 *     hm = 0 if any a_k = 0, else K / sum_k (1 / a_k);  the dual averaging of pfmi_hmc_adapt_enqueue on hm gives le, leb, m;  e+ = exp(le)
 *     A > 0 and g finite:  s <- 0.95 s + 0.05 g^2,  b <- 0.95 b (b_0 = 1),  lt = log tau + 0.025 g / (sqrt(s / (1 - b)) + 1e-8)   (Adam)
 *     else                 lt = log tau and PFMI_CHEES_KEPT_TRAJ is set
 *     w = m^(-3/4);  ltb <- w lt + (1 - w) ltb (ltb_0 = 0);  tau+ = min(max(exp(lt), e+), max_leapfrog e+)
 *   (a value that is not positive and finite keeps tau and sets PFMI_CHEES_KEPT_TRAJ; a step size likewise: PFMI_ADAPT_KEPT_STEP).  After
 *   t = W - 1 sampling uses e = exp(leb) and tau = min(max(exp(ltb), e), max_leapfrog e); the sampling transitions keep the jitter h_t.
 * step_size0: the one initial step size; traj_length0: the initial tau, 0 for step_size0.  nwarmup = 0 samples with both as given.
 * flags: PFMI_HMC_CONTINUE (nwarmup = 0 only, ChEES chains only: t goes on), PFMI_HMC_RECORD_PATH (one row per round, room for the cap),
 * PFMI_CHEES_RECORD_UPDATE (keeps x, x' and u' of every update: pfmi_chees_get_update).
 * Rounds: (fresh ? 1 : 0) + sum_t L_t, decided on the device; the cap is (fresh ? 1 : 0) + (W + T) max_leapfrog.  _enqueue issues a first
 * window and returns, pfmi_chees_pump / pfmi_chees_wait are pfmi_nuts_pump / pfmi_nuts_wait's counterparts (one pump serves both).  Rounds
 * issued ahead of the progress word idle.  Two equal runs give equal bits.
 * The warm-up fills the traces of pfmi_hmc_adapt_enqueue (eps: the shared step size, accept: a_k, n_leapfrog: L_t), so pfmi_adapt_get,
 * pfmi_hmc_get, pfmi_hmc_draws_dev, pfmi_hmc_get_path and pfmi_chain_diagnostics(PFMI_CHAIN_SRC_HMC) serve a ChEES run after its wait.
 * Errors are pfmi_hmc_enqueue's; also PFMI_ERR_ARG for max_leapfrog outside 1 .. 1024, target_accept outside (0, 1), traj_length0 < 0 or
 * not finite, nwarmup < 0, CONTINUE with nwarmup > 0; PFMI_ERR_UNSUPPORTED for a staged scale (pfmi_chain_scale_set) and for
 * nwarmup + ntransitions >= 2^31; PFMI_ERR_STATE for CONTINUE on static-HMC or NUTS chains (and their CONTINUE on ChEES chains).  Every
 * error drains this ctx's stream and leaves no chains and no traces behind.
 * Stage names: "chees" (the step kernel), "chees_closure", "chees_update" (the update's launches and the one that opens the next
 * trajectory); "chees:<KPAD>:<res|stream>" counts the step launches of one plan. */
#define PFMI_CHEES_CLAMPED 8         /* status bit: a transition wanted more than max_leapfrog steps */
#define PFMI_CHEES_KEPT_TRAJ 16      /* status bit: an update kept the trajectory length (no accepted proposal, or a value not finite) */
#define PFMI_CHEES_RECORD_UPDATE 8   /* flag */
#define PFMI_CHEES_MAX_LEAPFROG 1024
int32_t pfmi_chees_enqueue(pfmi_ctx *ctx, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, double step_size0,
                           double traj_length0, int32_t max_leapfrog, int64_t nwarmup, int64_t ntransitions, double target_accept,
                           int32_t flags);
int32_t pfmi_chees_pump(pfmi_ctx *ctx, int32_t *finished);
int32_t pfmi_chees_wait(pfmi_ctx *ctx);
/* The last ChEES call (finished): *step_size and *traj_length its sampling values; tau_trace, grad_trace, hmean_trace [W]: the tau
 * transition t used, g and hm of its update; n_leapfrog int32 [W + T]: L_t of the call's transitions; *status: PFMI_CHEES_* and
 * PFMI_ADAPT_KEPT_STEP.  Any may be NULL.  Waits. */
int32_t pfmi_chees_get(pfmi_ctx *ctx, double *step_size, double *traj_length, double *tau_trace, double *grad_trace, double *hmean_trace,
                       int32_t *n_leapfrog, int32_t *status);
/* PFMI_CHEES_RECORD_UPDATE: x, x' and u' [n][K][d] of the updates after warm-up transitions t0 .. t0 + n - 1.  Any may be NULL. */
int32_t pfmi_chees_get_update(pfmi_ctx *ctx, int64_t t0, int64_t n, double *x, double *xprop, double *vel);
/* rounds until the chains went idle = (fresh ? 1 : 0) + sum L_t, and the columns handed to the closure: K per round issued */
int32_t pfmi_chees_stats(pfmi_ctx *ctx, int64_t *rounds, int64_t *closure_columns);
/* Host builds of the rule (csrc/adapt.h); no GPU, no ctx.  pfmi_host_chees_leapfrog: L_t (*clamped, may be NULL: n > max_leapfrog).
 * pfmi_host_chees_update: one update on x, xprop, vel [K][d] and accept [K] with jitter h; last != 0: the update after the last warm-up
 * transition.  state in/out; grad and hmean are outputs. */
typedef struct {
    double step_size, traj_length, s, b, ltb;      /* b starts at 1, s and ltb at 0 */
    double hbar, leb, mu, delta;                   /* the dual averaging: mu = log(10 step_size0), delta = target_accept */
    int32_t m, status;
    double grad, hmean;
} pfmi_chees_state;
int32_t pfmi_host_chees_leapfrog(int64_t t, double traj_length, double step_size, int32_t max_leapfrog, int32_t *clamped);
int32_t pfmi_host_chees_update(int32_t K, int32_t d, const double *x, const double *xprop, const double *vel, const double *accept, double h,
                               int32_t max_leapfrog, int32_t last, pfmi_chees_state *state);

/* ---- chain diagnostics: rank-normalised split R-hat and ESS ------------------------------------------------------------------- */
/* The table the reference's worked examples end every chain run with (summarystats(chns), docs/src/examples/turing.md,
 * initializing-hmc.md): mean, sd, mcse, ess_bulk, ess_tail, rhat per coordinate, computed where the draws are.  Definitions: Vehtari,
 * Gelman, Simpson, Carpenter, Buerkner (2021).  Per coordinate, x[k][t] with K >= 1 chains of T >= 8 draws:
 *   split     n = T / 2, M = 2 K; split chain 2k = x[k][0:n], 2k + 1 = x[k][T-n:T] (odd T: the middle draw is in neither); S' = M n
 *   series y  chain means ybar_m; gamma_m(t) = (1/n) sum_{i < n-t} (y[m][i] - ybar_m)(y[m][i+t] - ybar_m); W = n/(n-1) mean_m gamma_m(0);
 *             var+ = (n-1)/n W + var_m(ybar_m, ddof 1); Rhat(y) = sqrt(var+ / W); rho_t = 1 - (W - mean_m gamma_m(t)) / var+, rho_0 = 1
 *   ESS(y)    Geyer: P_j = rho_2j + rho_2j+1 while 2j + 1 <= n - 2; J the first j with P_j <= 0 (or the number of pairs); P'_j the running
 *             minimum; tau = -1 + 2 sum_{j<J} P'_j + max(rho_2J, 0) (no last term when the pairs ran out); tau >= 1 / log10(S');
 *             ESS = S' / tau
 *   z(x)      the normal quantile (Wichura's AS 241, PPND16) of (r - 3/8) / (S' + 1/4), r the rank among the S' values that survive
 *             the split, ties given their average rank;  fold(x) = |x - median|;  I_p(x) = [x <= q_p]; median and q_p are type 7
 *   outputs   mean, sd (ddof 1) over all K T draws; ess_mean = ESS(x); mcse_mean = sd / sqrt(ess_mean); ess_bulk = ESS(z(x));
 *             ess_tail = min(ESS(I_0.05), ESS(I_0.95)); rhat = max(Rhat(z(x)), Rhat(z(fold(x))))
 * A coordinate with a non-finite draw: NaN in every output.  W = 0 (a constant series or indicator): NaN for that ESS / R-hat.
 * Neither is an error.  A chain (or coordinate) whose values are all equal has exactly that value as its mean, so W = 0 is exact.  Every sum is formed in a fixed order: two calls give equal bits. */
#define PFMI_CHAIN_SRC_HMC 0     /* the ctx's resident HMC records; draws NULL; d, T, K the run's values or all 0 */
#define PFMI_CHAIN_SRC_HOST 1    /* draws: host array [K][T][d] (pfmi_hmc_get's layout), uploaded on the ctx stream; any ctx, no target or fit needed */
#define PFMI_CHAIN_WITH_LP 1     /* SRC_HMC only: every output has one more entry, at index d, for the recorded logp series */
/* Outputs: d (+ 1) doubles each; any may be NULL.  Waits.  The HMC records and PFMI_HMC_CONTINUE are untouched.  PFMI_ERR_ARG: T < 8,
 * K < 1, d < 1, an unknown source or flag, WITH_LP with SRC_HOST, SRC_HMC with draws or with d, T, K that are not the run's.
 * PFMI_ERR_STATE: SRC_HMC without a resident run (what forgets the chains: pfmi_hmc_enqueue).  PFMI_ERR_UNSUPPORTED: the workspace
 * (about 8 (4 d K T) bytes) does not fit in free device memory; the message states the bytes.  Ranks are counted against sorted tiles
 * of 2048 values, O((K T)^2 / 2048 log 2048) per coordinate (profiles/chain_diagnostics.md).  Stage names under pfmi_profile:
 * "chain_diag_transpose", "chain_diag_moments", "chain_diag_rank", "chain_diag_ess", "chain_diag_final"; "chain_diag:count:<one|tiled>"
 * counts the calls whose S' values fit one such tile or take several. */
int32_t pfmi_chain_diagnostics(pfmi_ctx *ctx, int32_t source, const double *draws, int32_t d, int64_t T, int32_t K, int32_t flags,
                               double *mean, double *sd, double *mcse_mean, double *ess_mean, double *ess_bulk, double *ess_tail,
                               double *rhat);

/* ---- pooling, _compute_psis_result, _resample ---------------------------------------------------- */
/* draws_per_component = stack(draws) (src/multipath.jl:217): for path k take N_r draws of fit
 * `points[k]` with seed seeds[k] into the device-resident pool (d, N_r, K) and
 * log_ratios[k*N_r + n] = logp - logq (src/resample.jl:81-95; n fastest, k slowest). */
int32_t pfmi_pool_build(pfmi_ctx *ctx, int64_t N_r, const int64_t *points, const uint64_t *seeds);
/* The same with the winners picked ON THE DEVICE from the last pfmi_elbo_batch[_enqueue] -- no host round trip between the scan and
 * the pool: for path k the fit is fit_distributions[fit_iteration + 1] (src/singlepath.jl:224) = point off[k] + best_iter[k]; a
 * successful path (L > 0, ELBO finite and != -Inf, src/singlepath.jl:309-314) reuses its ELBO draws, i.e. the seed of the winning
 * fit (src/singlepath.jl:226-230, N_r > N_e continues the same counter); a failed path draws afresh with fail_seeds[k]
 * (rand(rng, fit_distribution, ndraws), src/singlepath.jl:231-233; fail_seeds NULL: the seed of the fit is used there too).
 * Only enqueues.  pfmi_pool_winners reads back what was used (blocks): points[K], seeds[K], success[K]; any may be NULL. */
int32_t pfmi_pool_build_best(pfmi_ctx *ctx, int64_t N_r, const uint64_t *fail_seeds);
int32_t pfmi_pool_winners(pfmi_ctx *ctx, int64_t *points, uint64_t *seeds, int32_t *success);
int32_t pfmi_pool_get(pfmi_ctx *ctx, double *draws, double *log_ratios);
/* Weighted moments of the pool on the device, per local run k and coordinate i (run-major outputs, any of them may be NULL).  With
 * t = x_i - center[i] (center NULL: 0) and the sums over the N_r draws n of run k:
 *   s1[k*d + i] = sum w t      s2[k*d + i] = sum w t^2      s2w[k*d + i] = sum w^2 t^2      wsum[2k], wsum[2k + 1] = sum w, sum w^2
 * importance != 0: w = the ctx's current PSIS weight of global pool column col_offset + k*N_r + n (pfmi_psis / pfmi_comm_pool_psis;
 * replicated on every GPU); a column whose weight is exactly 0 is skipped, whatever it holds (a non-finite draw there contributes
 * nothing).  importance == 0: w = 1 and nothing is skipped (a non-finite draw gives a non-finite sum).
 * Ordering guarantee: no atomics, and the order in which the terms of one run are added depends on (d, N_r) only -- not on K, col_offset
 * or the run's position -- so a run's sums have the same bits on whichever ctx owns it, and two calls return identical results.
 * No pool: PFMI_ERR_STATE; importance != 0 without a PSIS result covering [col_offset, col_offset + K*N_r): PFMI_ERR_STATE;
 * col_offset < 0: PFMI_ERR_ARG. */
int32_t pfmi_pool_moments(pfmi_ctx *ctx, int64_t col_offset, int32_t importance, const double *center, double *wsum, double *s1,
                          double *s2, double *s2w);
/* Weighted empirical CDF of the pool on the device at nthr thresholds per coordinate, T[j*d + i] (1 <= nthr <= 32; any doubles,
 * +-inf included).  Counted columns and their weights w are those of pfmi_pool_moments: importance != 0 takes the ctx's PSIS weight of
 * global pool column col_offset + k*N_r + n and skips a column whose weight is exactly 0 whatever it holds; importance == 0 takes
 * w = 1 and skips nothing.  Per threshold j and coordinate i, over the counted columns of the ctx's runs (any output may be NULL):
 *   wle[j*d + i]   = sum of w over the columns with x_i <= T     below[j*d + i] = max of the x_i <= T, -inf if there is none
 *   nanflag[i]     = 1 if a counted column holds a NaN in row i  above[j*d + i] = min of the x_i >  T, +inf if there is none
 * A NaN compares false on both sides: it enters neither wle, below nor above.
 * Ordering guarantee: no atomics; the terms of one run are added in an order that depends on (d, N_r) only, the runs are added in run
 * order on top of wle_in[nthr*d] (NULL: zeros), which is added first.  So contexts chained in run order, each passing its wle to the
 * next as wle_in, return the bits of one context that holds all the runs; below / above / nanflag of the parts combine exactly by
 * max / min / or.
 * THE QUANTILE built on it (pfmi.importance_quantiles): with U_i(v) = sum of w over the counted columns of the GLOBAL pool with
 * x_i <= v and W the total counted weight, the weighted type-1 (inverted-CDF) quantile of coordinate i at probability p is the
 * smallest pool value v of row i with U_i(v) >= p * W (that double product, formed once on the host); if no value satisfies it
 * (rounding at p = 1) the largest counted value; NaN if nanflag[i] or W == 0.  Always an element of the pool, never an interpolation.
 * No pool: PFMI_ERR_STATE; importance != 0 without a PSIS result covering [col_offset, col_offset + K*N_r): PFMI_ERR_STATE;
 * col_offset < 0, nthr outside [1, 32] or thresholds NULL: PFMI_ERR_ARG. */
int32_t pfmi_pool_cdf(pfmi_ctx *ctx, int64_t col_offset, int32_t importance, int32_t nthr, const double *thresholds,
                      const double *wle_in, double *wle, double *below, double *above, int32_t *nanflag);
/* Weighted cross moments of the pool on the device: the d x d matrix C, row i at c_out + i*d.  With t_i = x_i - center[i] (center NULL:
 * 0), over the N_r draws n of the ctx's runs k and for i >= j:
 *   C[i][j] = c_in[i*d + j] + sum_k (in run order) sum_n (w t_i) t_j              (c_in NULL: zeros)
 * each term being fl(w * fl(x_i - center[i])) times fl(x_j - center[j]), accumulated by a fused multiply-add.  Columns and weights w
 * are those of pfmi_pool_moments: importance != 0 takes the ctx's PSIS weight of global pool column col_offset + k*N_r + n and skips a
 * column whose weight is exactly 0 whatever it holds (a non-finite draw there contributes nothing); importance == 0 takes w = 1 and
 * skips nothing.  A NaN in row r of a counted column makes exactly row r and column r of C NaN.
 * Symmetry guarantee: only entries with i >= j are computed (and only those of c_in are read); C[j][i] is written as a copy of C[i][j],
 * so the two triangles have the same bits ((w t_i) t_j and (w t_j) t_i round differently).
 * Ordering guarantee: no atomics; the terms of one run are added in an order that depends on (d, N_r) only -- not on K, col_offset, the
 * run's position or the device; the runs are added in run order on top of c_in, which is added first.  So contexts chained in run order,
 * each passing its c_out to the next as c_in, return the bits of one context that holds all the runs.
 * d is not capped (entries are addressed with size_t); the device buffer of d*d doubles failing to allocate: PFMI_ERR_HIP.
 * No pool: PFMI_ERR_STATE; importance != 0 without a PSIS result covering [col_offset, col_offset + K*N_r): PFMI_ERR_STATE;
 * col_offset < 0 or c_out NULL: PFMI_ERR_ARG. */
int32_t pfmi_pool_cross(pfmi_ctx *ctx, int64_t col_offset, int32_t importance, const double *center, const double *c_in, double *c_out);
/* The weighted second moment of the pool applied to a thin block of r vectors on the device, without forming the d x d matrix
 * (1 <= r <= PFMI_POOL_APPLY_MAX_R): what a subspace iteration for the top eigenpairs of the pooled covariance needs, at 4 d r flops per
 * draw instead of d^2.  Directions v[j*d + i], j < r.  With t_i(n) = fl(x_i(n) - center[i]) (center NULL: 0), over the N_r draws n of the
 * ctx's runs k:
 *   scores[(k*N_r + n)*r + j] = z_j(n) = sum_i t_i(n) * v[j*d + i]                      (0 for every j when the column is skipped)
 *   y_out[j*d + i]            = y_in[j*d + i] + sum_k (in run order) sum_n fl(w t_i(n)) * z_j(n)          (y_in NULL: zeros)
 * so that row j of y_out is (sum_n (w t) t') v_j.  Both contractions run on the f64 matrix cores, every product accumulated by a fused
 * multiply-add.  y_out is required; scores is a host buffer of K*N_r*r doubles, or NULL for no download.  Columns and weights w are
 * those of pfmi_pool_moments: importance != 0 takes the ctx's PSIS weight of global pool column col_offset + k*N_r + n and skips a column
 * whose weight is exactly 0 whatever it holds: it is not read, its scores are exact zeros and it adds nothing to y_out (a NaN anywhere in
 * it is invisible); importance == 0 takes w = 1 and skips nothing.  A NaN in a counted column makes that column's r scores NaN, and
 * with them every entry of y_out.
 * Independence of the block: z_j(n) and row j of y_out have the same bits whatever r is and whatever the other directions hold
 * (direction 3 of an r = 32 call equals direction 0 of an r = 1 call given that one vector).
 * Ordering of scores: a score depends on its column, its direction, center and d only -- not on K, N_r, col_offset, the run's position
 * or the device.
 * Ordering of apply (the guarantee of pfmi_pool_cross): no atomics; the terms of one run are added in an order that depends on (d, N_r)
 * only -- not on K, col_offset, the run's position or the device; the runs' sums are added in run order on top of y_in, which is added
 * first.  So contexts chained in run order, each passing its y_out to the next as y_in, return the bits of one context that holds all
 * the runs.
 * No pool: PFMI_ERR_STATE; importance != 0 without a PSIS result covering [col_offset, col_offset + K*N_r): PFMI_ERR_STATE;
 * col_offset < 0, r outside [1, PFMI_POOL_APPLY_MAX_R], v or y_out NULL: PFMI_ERR_ARG. */
#define PFMI_POOL_APPLY_MAX_R 32
int32_t pfmi_pool_apply(pfmi_ctx *ctx, int64_t col_offset, int32_t importance, const double *center, int32_t r, const double *v,
                        const double *y_in, double *y_out, double *scores);
/* device pointer to the local pool's draws (d x K_local*N_r doubles, column-major, a column per draw; count = their number), for hosts
 * that keep the pool on the GPU.  The stream is idle on return.  Valid until the next pfmi_pool_build* on this ctx. */
int32_t pfmi_pool_draws_dev(pfmi_ctx *ctx, void **dev_ptr, int64_t *count);
/* device pointer to the local log-ratio shard (K_local * N_r doubles) for the RCCL all-gather */
int32_t pfmi_pool_log_ratios_dev(pfmi_ctx *ctx, void **dev_ptr, int64_t *count);

/* Mixture-proposal log ratios of the pool on the device.  The pool is a stratified sample of the uniform mixture qbar = (1/K) sum_k q_k of
 * the K fits it was drawn from (the points of pfmi_pool_build / _build_best, in run order); for every pool column g = k*N_r + n:
 *   log_mix[g]    = log sum_k exp(logpdf(fit k, x_g)) - log K     components in run order; NaN if any component is NaN (a failed fit),
 *                                                                 -inf if all are -inf (the rules of pfmi_mixture_logpdf)
 *   log_ratios[g] = logp[g] - log_mix[g]                          logp: the target values pfmi_pool_build stored with the pool
 * -- the deterministic-mixture (balance-heuristic) weights of multiple importance sampling, in place of logp - logq of the run that drew
 * the column (pfmi_pool_get, which this call leaves untouched).  Host outputs of K*N_r doubles each, either may be NULL; blocks.
 * At d <= 1024 log_mix has the bits of pfmi_mixture_logpdf_dev on pfmi_pool_draws_dev minus log K (the double log(K) of the host's libm);
 * at d > 1024 with history_length <= 16 the components come from a row-tiled matrix-core kernel and agree with it to rounding.
 * Ordering guarantee: a column's value depends on the column, the K fits and d only -- not on its position in the pool, on N_r, or on how
 * the call cuts the pool into chunks.
 * No pool: PFMI_ERR_STATE; a column padding the kernels do not cover: PFMI_ERR_UNSUPPORTED. */
int32_t pfmi_pool_mixture_ratios(pfmi_ctx *ctx, double *log_mix, double *log_ratios);
/* device pointer to the log ratios of the last pfmi_pool_mixture_ratios (K_local * N_r doubles), for pfmi_psis_dev.  The stream is idle on
 * return.  Valid until the next pfmi_pool_build* on this ctx; no pfmi_pool_mixture_ratios on the current pool: PFMI_ERR_STATE. */
int32_t pfmi_pool_mixture_ratios_dev(pfmi_ctx *ctx, void **dev_ptr, int64_t *count);

/* One affine map for every column of the pool, and the target at the moved columns: the pass of importance-weighted moment matching
 * (Paananen, Piironen, Buerkner, Vehtari 2021).  With x0 the pool AS BUILT by pfmi_pool_build[_best], every column becomes
 *   x' = fma(scale, x0, shift)   (elementwise over the d rows; scale[d] all > 0 and finite, shift[d] finite)
 * The map is CUMULATIVE: it is always applied to x0, never on top of an earlier call, so the bits do not depend on the calls before
 * and a rebuilt pool plus one call reproduces them.  In the same pass logp(x') is formed for the built-in targets (host and device
 * closures are called on the moved pool as pfmi_pool_build calls them), then
 *   logq' = logq0 - sum_i log scale_i      (every run's proposal under the same map; the sum is taken once on the host, in index order)
 *   log ratio' = logp' - logq'
 * and, when pfmi_pool_mixture_ratios ran on the pool as built, mixture ratio' = logp' - (log qbar0 - sum_i log scale_i).
 * After the call the ctx's pool IS the moved pool: pfmi_pool_get, pfmi_pool_moments / _cdf / _cross / _apply, pfmi_pool_psis_runs, the
 * gather, pfmi_pool_*_dev (pointers fetched AFTER the call) and the communicator's PSIS and resampling see it without change.  The
 * state before the call is kept for pfmi_pool_transform_revert.  A column whose run's fit failed keeps NaN densities.
 * scale == NULL: all ones; shift == NULL: zeros; both NULL: the pool as built is put back (no pass).
 * logp_out, log_ratios_out: K_local * N_r doubles, either may be NULL.  The ctx's PSIS weights are not touched.
 * Ordering guarantee: the terms of a column's logp are added in an order that depends on d alone.
 * While the pool is moved pfmi_pool_mixture_ratios returns PFMI_ERR_STATE (put the pool as built back first).
 * No pool: PFMI_ERR_STATE; a scale that is not positive and finite or a shift that is not finite: PFMI_ERR_ARG, the pool is left as
 * it was -- a refused call changes NOTHING, including what pfmi_pool_transform_revert would undo: a revert after it still puts back the
 * state from before the last call that succeeded.  A new pfmi_pool_build* drops all transform state.  Stage names under pfmi_profile:
 * "pool_transform" (the pass), "pool_transform_ratio".  Memory: the pool as built and the state before the last call stay resident
 * (up to three pools) while the pool is one that was transformed; the next pfmi_pool_build* of a pool of ANOTHER size frees the two
 * spare sets (a rebuild of the same size, as the summaries of a moment-matched result do, keeps them and allocates nothing). */
int32_t pfmi_pool_transform(pfmi_ctx *ctx, const double *scale, const double *shift, double *logp_out, double *log_ratios_out);
/* Puts the state from before the last pfmi_pool_transform back (a buffer swap, no pass): how a rejected trial is undone.  A second
 * revert in a row, a revert with nothing to undo or without a pool: PFMI_ERR_STATE.  The ctx's PSIS weights are not touched. */
int32_t pfmi_pool_transform_revert(pfmi_ctx *ctx);

/* Per-run Pareto diagnostics of the pool: PSIS.psis of every run's own N_r log ratios, all K runs in one launch (one workgroup per
 * run).  source selects the ratios: */
#define PFMI_RATIOS_COMPONENT 0   /* logp - logq of the run that drew the column (pfmi_pool_get) */
#define PFMI_RATIOS_MIXTURE   1   /* logp - log qbar (the last pfmi_pool_mixture_ratios on this pool) */
/* For run k, over lr[k*N_r .. (k+1)*N_r):
 *   pareto_k[k]   k-hat of the run; NaN where PSIS does not smooth (a tail of fewer than 5, a non-finite value in the tail, ...)
 *   tail_len[k]   M = min(cld(N_r, 5), ceil(3 sqrt(N_r)))
 *   lse[k]        logsumexp of the run's smoothed log ratios: lse[k] - log(N_r) estimates the log evidence from this run alone
 *   sumsq[k]      sum_n w_n^2 of the run's normalised weights (1 / sumsq is the run's effective sample size); NaN if any w_n is NaN
 *   log_weights, weights   K*N_r each, every run normalised on its own (each run's weights sum to 1)
 * Host outputs of K, K, K, K, K*N_r, K*N_r entries; any may be NULL (all NULL: the pass still runs); blocks.
 * Guarantees: pareto_k, tail_len, log_weights and weights of a run have the bits of pfmi_psis on the run's slice taken through the
 * one-workgroup route (both call one device function), and lse is the constant that route subtracted; sumsq is added in an order that
 * depends on N_r only.  A run's outputs depend on its N_r ratios alone -- not on K, on the run's position in the pool, or on the device --
 * so the diagnostics of a pool sharded over several contexts are the per-context results concatenated, and no communicator is involved.
 * The context's current PSIS result (pfmi_psis / pfmi_psis_dev / pfmi_comm_pool_psis: what pfmi_psis_weights, pfmi_resample_indices and
 * the importance-weighted pool passes read) is neither read nor written: the call has buffers of its own.
 * No pool: PFMI_ERR_STATE; PFMI_RATIOS_MIXTURE without pfmi_pool_mixture_ratios on the current pool: PFMI_ERR_STATE; any other source:
 * PFMI_ERR_ARG; N_r whose tail M + 1 exceeds 4096 (N_r > 1 863 225): PFMI_ERR_UNSUPPORTED.  Stage name under pfmi_profile: "psis_runs". */
int32_t pfmi_pool_psis_runs(pfmi_ctx *ctx, int32_t source, double *pareto_k, int64_t *tail_len, double *lse, double *sumsq,
                            double *log_weights, double *weights);   /* K, K, K, K, K*N_r, K*N_r; any may be NULL; blocks */

/* PSIS.psis(log_ratios) (src/resample.jl:78): log_ratios_dev is a DEVICE buffer of S doubles (the
 * all-gathered pool), weights are kept device-resident; host outputs may be NULL. */
int32_t pfmi_psis_dev(pfmi_ctx *ctx, const void *log_ratios_dev, int64_t S, double *weights,
                      double *log_weights, double *pareto_k, int64_t *tail_len);
int32_t pfmi_psis(pfmi_ctx *ctx, const double *log_ratios, int64_t S, double *weights,
                  double *log_weights, double *pareto_k, int64_t *tail_len);
/* the ctx's current PSIS result (PSISResult.weights / .log_weights, S doubles each; either may be NULL) -- for hosts that leave
 * the vectors on the device until somebody looks at them */
int32_t pfmi_psis_weights(pfmi_ctx *ctx, int64_t S, double *weights, double *log_weights);

/* _resample index selection (src/resample.jl:58-66): ndraws indices into 0..S-1.
 * importance != 0: weighted by the ctx's current PSIS weights; == 0: uniform (psis_result === nothing).
 * replace: with / without replacement.  uniforms: NULL (Philox(seed)) or ndraws doubles in [0,1). */
int32_t pfmi_resample_indices(pfmi_ctx *ctx, int64_t S, int64_t ndraws, int32_t importance,
                              int32_t replace, uint64_t seed, const double *uniforms, int64_t *idx);

/* StatsBase-compatible index selection for hosts that must match a live Julia run bit for bit: exactly
 * StatsBase.direct_sample!(rng, 1:S, ProbabilityWeights(weights, 1), x) (the weighted branch of src/resample.jl:61-66 ->
 * StatsBase.sample(rng, wv): t = rand(rng) * 1; i = 1; cw = w[1]; while cw < t && i < S: i += 1; cw += w[i]) on the ctx's
 * current PSIS weights, with the running sum accumulated sequentially in fp64 like the Julia loop and uniforms[t] = the
 * host's rand(rng) values in [0, 1).  idx is 0-based.  (pfmi_resample_indices is this library's own fixed-point
 * inverse-CDF sampler: deterministic for any launch geometry / GPU count, but not StatsBase's algorithm.) */
int32_t pfmi_resample_indices_direct(pfmi_ctx *ctx, int64_t S, int64_t ndraws, const double *uniforms, int64_t *idx);

/* draws = draws_all[:, inds] (src/resample.jl:68).  Global pool column g = k_global*N_r + n is owned by this ctx iff
 * col_offset <= g < col_offset + K_local*N_r.  Host variant: every index must be owned (PFMI_ERR_ARG otherwise -- a
 * stale or out-of-range index is an error, never a silent zero column).  draws[d*ndraws]. */
int32_t pfmi_pool_gather(pfmi_ctx *ctx, int64_t ndraws, const int64_t *idx, int64_t col_offset,
                         double *draws);
/* variant into a DEVICE buffer for hosts that assemble a result themselves: columns not owned are written as zeros (a sum over the
 * ranks' buffers is then the result; pfmi_comm_* itself moves only the owned columns) */
int32_t pfmi_pool_gather_dev(pfmi_ctx *ctx, int64_t ndraws, const int64_t *idx, int64_t col_offset,
                             void *draws_dev);

/* ---- multi-GPU: the pooled stage over paths sharded across GPUs (RCCL over xGMI) ----------------------------------- */
/* Runs are independent until pooling (src/multipath.jl:190-208); draws_per_component = stack(draws), _compute_psis_result and
 * _resample (src/multipath.jl:215-225) see every run.  Each GPU owns a contiguous block of paths (its ctx was fed only those
 * traces; pool order stays k-major, src/resample.jl:93) and has called pfmi_pool_build.  The blocks may have DIFFERENT lengths (any nruns
 * over any number of GPUs, src/multipath.jl:131-146: e.g. 20 runs over 8 GPUs = 3 3 3 3 2 2 2 2); draws per run and dimension must agree.
 * A pfmi_comm joins the contexts:
 *   pfmi_comm_init_all   ONE host process drives G contexts, one per GPU (ncclCommInitAll) -- a single Julia / C caller;
 *   pfmi_comm_init_rank  one process per GPU: every process passes the same 128-byte id (pfmi_comm_unique_id on rank 0,
 *                        shipped by the host's launcher) -- e.g. under torch.distributed.run or MPI.
 * The result is identical for every G (extension of the ntasks invariance of test/multipath.jl:107-140). */
typedef struct pfmi_comm pfmi_comm;
int32_t pfmi_comm_unique_id(uint8_t *id128);
int32_t pfmi_comm_init_all(int32_t ngpus, pfmi_ctx *const *ctxs, pfmi_comm **out);
int32_t pfmi_comm_init_rank(pfmi_ctx *ctx, int32_t world, int32_t rank, const uint8_t *id128, pfmi_comm **out);
int32_t pfmi_comm_destroy(pfmi_comm *comm);
/* world = ranks RCCL itself reports (ncclCommCount), nlocal = contexts driven by this process, rccl_version = ncclGetVersion */
int32_t pfmi_comm_info(pfmi_comm *comm, int32_t *world, int32_t *nlocal, int32_t *rccl_version);
/* _compute_psis_result over all runs (src/multipath.jl:221): ONE all-gather of the fp64 log-ratio shards (K_r * N_r doubles from GPU r;
 * unequal shards travel padded to the largest one and are compacted back to the pool order), then PSIS.psis replicated on every GPU
 * (weights stay device resident). */
int32_t pfmi_comm_pool_psis(pfmi_comm *comm, double *pareto_k, int64_t *tail_len);
/* _resample over all runs (src/multipath.jl:225, src/resample.jl:58-72): index selection replicated on every GPU (same
 * arguments as pfmi_resample_indices; identical indices by construction, checked); the selected columns reach the caller by
 * OWNER-ONLY transfers -- no GPU other than the one that owns a column touches it, no rank allocates d x ndraws unless it returns it:
 *   pfmi_comm_init_all   every GPU stores the columns it owns straight into draws[d * ndraws] (zero-copy when `draws` is page-locked
 *                        memory from pfmi_host_alloc; through a page-locked staging block of the communicator + one host copy otherwise);
 *   pfmi_comm_init_rank  the owners send their columns to RANK 0 (ncclSend / ncclRecv of exactly the owned columns): `draws` is filled
 *                        on rank 0 only -- pass NULL on the other ranks (a non-NULL array there comes back all-NaN, never stale); idx,
 *                        pareto_k, tail_len are replicated and valid on every rank.  Costs one extra host round trip (the transfers are
 *                        sized from the indices).
 * idx: global 0-based pool columns (component id = idx / N_r). */
int32_t pfmi_comm_resample(pfmi_comm *comm, int64_t ndraws, int32_t importance, int32_t replace, uint64_t seed,
                           const double *uniforms, int64_t *idx, double *draws);
/* Both stages in one call: [all-gather + PSIS when importance != 0] -> index selection -> owner-only transfer of the selected columns;
 * under pfmi_comm_init_all everything is enqueued on every local context before the ONE wait, so a single host thread keeps all its
 * GPUs busy (src/multipath.jl:221-225).  A world of one context needs no RCCL at all (the single-GPU hot path takes this route too).
 * pareto_k / tail_len are NaN / 0 when importance == 0.
 * One process per GPU (pfmi_comm_init_rank): every rank must make the same sequence of pfmi_comm_* calls; a PFMI_ERR_* from any of
 * them is fatal for the whole group -- the ranks first agree on their shard size and local status, so a local precondition failure
 * or a size mismatch is reported on EVERY rank instead of leaving the others blocked in a collective. */
int32_t pfmi_comm_psis_resample(pfmi_comm *comm, int64_t ndraws, int32_t importance, int32_t replace, uint64_t seed,
                                const double *uniforms, double *pareto_k, int64_t *tail_len, int64_t *idx, double *draws);
/* The same in two halves: _enqueue launches all-gather, PSIS and index selection; _wait adds the owner-only transfers into `draws` (known
 * only now) and is the host round trip.  Between the two the caller may queue downloads on the member contexts with pfmi_defer_downloads:
 * _wait delivers them too.  (The library's own staged downloads of this stage are never affected by the caller's defer mode.) */
int32_t pfmi_comm_psis_resample_enqueue(pfmi_comm *comm, int64_t ndraws, int32_t importance, int32_t replace, uint64_t seed, const double *uniforms);
int32_t pfmi_comm_psis_resample_wait(pfmi_comm *comm, double *pareto_k, int64_t *tail_len, int64_t *idx, double *draws);
/* pfmi_defer_downloads(ctx, 1): from now on the download-only entry points -- pfmi_get_fit_status, pfmi_elbo_batch_wait, pfmi_psis_weights --
 * queue their copies behind whatever is enqueued and return at once; the destination arrays are filled (and a PFMI_ERR_RETRY of the scan
 * is reported) by the NEXT entry point that waits on this context (pfmi_sync, pfmi_comm_psis_resample_wait, ...): one host round trip for
 * all of them.  The arrays must stay valid until then.  (ctx, 0): back to normal, what is queued stays queued.  (ctx, -1): drop everything
 * queued (after a failure between queueing and waiting).  A queued download delivers the values of the call it was queued for: entry
 * points that enqueue work rewriting those results issue the pending copies first, in stream order. */
int32_t pfmi_defer_downloads(pfmi_ctx *ctx, int32_t mode);

/* ---- host utility --------------------------------------------------------------------------------------------------- */
/* The counter-based generator the Python / C host mirrors use for the reference's seed hierarchy (run_seeds =
 * rand!(rng, UInt64[nruns]) src/multipath.jl:162; seeds = rand!(rng, UInt64[L]) src/elbo.jl:2): out[i] = low 64 bits of
 * Philox4x32-10(counter (t0 + i, stream), key seed).  Host code only (a Julia host uses its own rng instead). */
int32_t pfmi_host_rand_u64(uint64_t seed, uint64_t t0, int64_t n, uint32_t stream, uint64_t *out);
/* m generators in one call: out[j * n + i] = value i of generator (seeds[j], first counter t0[j]) */
int32_t pfmi_host_rand_u64_multi(int32_t m, const uint64_t *seeds, const uint64_t *t0, int64_t n, uint32_t stream, uint64_t *out);

/* ---- device utilities for hosts that keep buffers on the GPU (bench, multi-GPU) ---------------- */
int32_t pfmi_malloc_dev(pfmi_ctx *ctx, int64_t bytes, void **dev_ptr);
int32_t pfmi_free_dev(pfmi_ctx *ctx, void *dev_ptr);
int32_t pfmi_memcpy_h2d(pfmi_ctx *ctx, void *dev_dst, const void *host_src, int64_t bytes);
int32_t pfmi_memcpy_d2h(pfmi_ctx *ctx, void *host_dst, const void *dev_src, int64_t bytes);

/* Page-locked host memory for LARGE result buffers (the draws of pfmi_pool_gather / pfmi_comm_resample / pfmi_comm_psis_resample, the
 * pool of pfmi_pool_get).  Every entry point accepts any host pointer; into ordinary (pageable) memory the runtime copies a large result
 * in 32 MB pieces through its own staging buffer, DMA and host copy one after the other (measured 16 GB/s: 9.7 ms for the 160 MB of draws
 * of a d = 10^4, ndraws = 2000 call), into a buffer from pfmi_host_alloc it is one DMA transfer at the link rate (54 GB/s).  Below ~16 MB
 * there is nothing to gain (measured at 8 MB).  Allocation costs milliseconds: recycle the buffers (the Python host keeps a pool). */
int32_t pfmi_host_alloc(int64_t bytes, void **host_ptr);
int32_t pfmi_host_free(void *host_ptr);

#ifdef __cplusplus
}
#endif
#endif /* PFMI_H */
