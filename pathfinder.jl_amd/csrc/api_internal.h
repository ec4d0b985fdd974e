// api_internal.h -- what the api_*.hip translation units (the extern "C" boundary of include/pfmi.h) share: the entry-point prologues,
// the drains of calls that were never waited for, and the ONE statement of every buffer layout and sizing rule more than one entry
// point relies on.  Each function is defined in the component it belongs to (named behind its declaration).
#pragma once
#include "pfmi_common.h"
#include "adapt.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

#define PF_CTX(c)                                                          \
    do {                                                                   \
        PF_CHECK((c) != nullptr, PFMI_ERR_ARG, "null pfmi_ctx");           \
        PF_HIP(hipSetDevice((c)->device));                                 \
        pf_download_forget(c);                                             \
    } while (0)
// Entry points that enqueue work which REWRITES (or may reallocate) result buffers: the staged downloads still pending -- entries queued under
// pfmi_defer_downloads survive several entry points, and their copy is only issued by the gather kernel of the next wait -- are issued NOW, in
// stream order in front of the new work, so that they deliver the values of the call they were queued for (a source must be a
// snapshot at queueing time, as it was when every download was its own stream-ordered copy).  No pending entry: no launch.
#define PF_CTX_MUT(c)                                                      \
    do {                                                                   \
        PF_CTX(c);                                                         \
        PF_TRY(pf_dl_flush(c));                                            \
    } while (0)

// a download the caller reads on return: queued like every other one, then the wait that delivers it
inline int32_t d2h(pfmi_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return PFMI_OK;
    PF_TRY(pf_download(c, dst, src, bytes));
    return pf_stream_sync(c);
}

struct StreamSwap {                       // the launch helpers enqueue on c->stream: point it at a side stream for the scope
    pfmi_ctx *c; hipStream_t keep; int slot; bool seg;
    StreamSwap(pfmi_ctx *c_, hipStream_t s, int qf_slot = 0, bool seg_mode = false) : c(c_), keep(c_->stream), slot(c_->qf_slot), seg(c_->qf_seg_mode) {
        c->stream = s; c->qf_slot = qf_slot; c->qf_seg_mode = seg_mode;
    }
    ~StreamSwap() { c->stream = keep; c->qf_slot = slot; c->qf_seg_mode = seg; }
};

// what a new trace invalidates (entry points that clear another set of flags spell theirs out)
inline void results_reset(pfmi_ctx *c) { c->fitted = false; c->elbo_done = false; c->pooled = false; c->have_trace_lp = false; }

// ---- api_ctx.hip
void stream_abandon(pfmi_ctx *c);          // drain and forget a streaming call that was never waited for
void lbc_abandon(pfmi_ctx *c);             // the same for a packed closure optimisation
void hmc_forget(pfmi_ctx *c);              // drain an HMC call that was never waited for and forget the chains (api_hmc.hip)
// ---- api_hmc.hip, api_nuts.hip: the enqueues behind the plain and the adaptive entry points (api_adapt.hip).  W = 0: a plain run.
// W >= 1: a fresh run whose first W transitions adapt the step size towards the acceptance `delta` and record no rows.  metric (W >= 1):
// CHAIN_METRIC_WINDOWS: the warm-up also adapts the per-coordinate scale in windows (adapt.h); CHAIN_METRIC_RECORD: and keeps every u.
enum { CHAIN_METRIC_NONE = 0, CHAIN_METRIC_WINDOWS = 1, CHAIN_METRIC_RECORD = 2 };
int32_t hmc_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                    int32_t nleapfrog, int64_t T, int32_t flags, int64_t W, double delta, int metric = CHAIN_METRIC_NONE);
int32_t nuts_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                     int32_t max_depth, int64_t T, int32_t flags, int64_t W, double delta, int metric = CHAIN_METRIC_NONE);
// ---- api_hmc.hip: the one enqueue path of both samplers.
struct ChainKind { const char *name, *NAME, *other; int kind; };       // "hmc" / "HMC" / the other sampler's name / HmcState::kind
// One buffer of a sampler call and its size, stated once; the memory estimate and the `ensure`s both walk the list of them.
// CHAIN_BUF: the chains' own, kept by a CONTINUE.  CALL_BUF: rewritten by every call.  PATH_BUF: RECORD_PATH only, `bytes` per round.
enum { CHAIN_BUF, CALL_BUF, PATH_BUF };
struct ChainBuf { DevBuf *buf; size_t bytes; int scope; bool est = true; };      // est: counted in the estimate
struct ChainCall {                                       // what both enqueues are given
    int32_t K; const int64_t *points; const double *x0; const uint64_t *seeds; const double *step_size; int64_t T; int32_t flags; int64_t W; double delta;
    int metric = CHAIN_METRIC_NONE;
};
// The shared checks in the order the entry points have always made them (messages under "<name>_enqueue:"): fit, target and null
// arguments; then the sampler checks its own parameter; flags, points, step sizes and what a CONTINUE needs; then the sampler's own
// CONTINUE checks.
int32_t chain_check_target(pfmi_ctx *c, const ChainKind &S, const ChainCall &A);
int32_t chain_check_chains(pfmi_ctx *c, const ChainKind &S, const ChainCall &A);
// Checks that every chain's fit succeeded, sizes `bufs` plus the common buffers for rounds = (fresh ? 1 : 0) + (W + T) per_transition
// against the free memory and grows them, quiets the call before (drain: pumps a NUTS run to its end), uploads, and sets the HmcState
// fields both samplers have.  A scale staged by pfmi_chain_scale_set becomes the chains' resident one (c->hmc.scaled: the caller launches
// the metric kernels); a run with metric windows starts from it, or from ones.  The caller launches init / reopen and issues the rounds.
int32_t chain_begin(pfmi_ctx *c, const ChainKind &S, const ChainCall &A, int64_t per_transition, const char *need_detail,
                    std::vector<ChainBuf> bufs, int32_t (*drain)(pfmi_ctx *), int64_t *rounds_out);
// The one pump of the samplers whose round count the device decides (NUTS, ChEES): `closure_stage` names the closure's stage of the run,
// `round` issues what follows the closure in a round -- the launches that consume its answer, with their own stage names -- as round number
// `round` (published with the progress word c->nt_status: round << 32 | low, low = 0 once every chain is idle) and path row `prow`.
// closure_stage null: a pump without a closure (nuts_fused_pump, api_nuts_fused.hip): a round is `round` alone and no column is counted.
struct ChainPump { const char *name; const char *(*closure_stage)(const HmcState &); int32_t (*round)(pfmi_ctx *c, int64_t round, int64_t prow); };
const ChainPump &nuts_fused_pump();                      // api_nuts_fused.hip: a round is one launch of up to HmcState::fused_cap evaluations
int32_t nuts_drain(pfmi_ctx *c);                         // api_nuts.hip: pumps the NUTS run on the ctx (closure rounds or fused launches) to its end
int32_t chain_issue_rounds(pfmi_ctx *c, const ChainPump &P);            // what may be in flight; sets H.finished
int32_t chain_pump_pass(pfmi_ctx *c, const ChainPump &P, int32_t *finished);      // one pass: never blocks
int32_t chain_drain(pfmi_ctx *c, const ChainPump &P);                   // pump to the end
int32_t chain_refused(pfmi_ctx *c, int32_t rc);           // rc != OK: drain, no run, no chains, no traces; returns rc
int32_t chain_dead_check(pfmi_ctx *c, const char *name, const std::vector<int32_t> &dead);         // the waits: a dead start point is PFMI_ERR_NUMERIC
int32_t chain_path_download(pfmi_ctx *c, int64_t round0, int64_t nrounds, double *X, double *closure_out, double *v);     // queued, not waited for
int32_t adapt_reset(pfmi_ctx *c, int32_t K, int64_t W, const double *step_size, double delta, int32_t status0);     // api_adapt.hip: states and traces of a fresh adaptive run
// api_adapt.hip: the windows of a run with A.metric set (H.metric_run, nwin, win_*, rec_u) and its hm_metric buffer in `bufs`; then, once the
// buffers are there, the scale (staged, or ones in front of metric windows) and the window table, with the Welford state cleared
struct MetricPlan { int nwin = 0; int64_t init = 0, ends[32] = {}; std::vector<double> scale; };      // scale: the staged one, taken
int32_t metric_plan(pfmi_ctx *c, const ChainCall &A, std::vector<ChainBuf> &bufs, MetricPlan &P);
int32_t metric_begin(pfmi_ctx *c, const ChainCall &A, const MetricPlan &P);
size_t adapt_bytes(int32_t K, int64_t W);
// api_adapt.hip: what every adaptive enqueue checks first (flags among `allowed`, nwarmup >= 1, target_accept in (0, 1))
int32_t adapt_args(const char *who, int64_t W, double delta, int32_t flags, int32_t allowed = 0);
// a plain CONTINUE is about to replace hm_eps: keep the adaptive run's final step sizes for pfmi_adapt_get (stream-ordered copy, once)
int32_t adapt_keep_step_sizes(pfmi_ctx *c);
int32_t ensure_pinned(pfmi_ctx *c, size_t x_bytes, size_t lp_bytes);

// ---- api_inputs.hip
// the packed layout of K paths with counts[k] >= 1 points each: off / path_of on the host and the device, K, d, P
int32_t set_packed_layout(pfmi_ctx *c, int32_t K, int32_t d, const int64_t *counts);
// the optimisers' fixed-stride staging trace [K][cap] (theta, grad, logp, point counts) and their starting points
int32_t staging_reserve(pfmi_ctx *c, int32_t K, size_t cap, int32_t d);
void lbc_begin(pfmi_ctx *c, int32_t K, int32_t J, int32_t maxiters, double g_tol, int32_t *prog);
int32_t lbc_issue_rounds(pfmi_ctx *c, hipStream_t s);

// ---- api_fit.hip
// the per-point fit state of P points (slots) in K paths at column padding kpad; clears hist_src on the ctx stream
int32_t fit_reserve(pfmi_ctx *c, size_t P, int32_t K, size_t d, int32_t J, int32_t kpad);

// ---- api_elbo.hip
int32_t elbo_reserve(pfmi_ctx *c, size_t P, int32_t K, int64_t N);       // the ELBO tables: logp / logq [P][N], elbo / se [P], best_iter [K]
int64_t devcb_chunk_fits(const pfmi_ctx *c, int64_t per_fit_doubles, int64_t nf, int64_t N);
// One block of a DEVICE_CALLBACK scan on stream `ss` (the ctx stream for the scope: StreamSwap): the draws of the `n` fits list[i] with
// seeds[i] (parity mode: the normals d_u, ustride apart) into bx, the user's closure on them into blp, its rows scattered into the
// point-indexed logp table (a failed fit's rows become NaN there).
int32_t devcb_scan_block(pfmi_ctx *c, hipStream_t ss, const int32_t *list, const uint64_t *seeds, int64_t n, int64_t N, const double *d_u,
                         int64_t ustride, double *bx, double *blp);
int32_t callback_logp(pfmi_ctx *c, const double *d_x, int64_t n, double *d_lp);
int32_t devcb_logp(pfmi_ctx *c, const double *d_x, int64_t n, double *d_lp, const int32_t *d_points, int64_t npts, int64_t N);
