// api_inputs.hip -- what a run starts from: the target, the traces (handed over, or made on the device by pfmi_optimize_batch*), and the
// driver of the closure optimiser.
#include "api_internal.h"

int32_t set_packed_layout(pfmi_ctx *c, int32_t K, int32_t d, const int64_t *counts) {
    c->off.assign((size_t)K + 1, 0);
    for (int k = 0; k < K; ++k) c->off[k + 1] = c->off[k] + counts[k];
    const int64_t P = c->off[K];
    PF_CHECK(P < (1ll << 31), PFMI_ERR_UNSUPPORTED, "too many trace points");
    c->path_of.resize((size_t)P);
    for (int k = 0; k < K; ++k)
        for (int64_t p = c->off[k]; p < c->off[k + 1]; ++p) c->path_of[(size_t)p] = k;
    c->K = K; c->d = d; c->P = P; c->virt = false;
    PF_TRY(c->d_off.ensure(sizeof(int64_t) * (K + 1)));
    PF_TRY(c->d_path_of.ensure(sizeof(int32_t) * P));
    PF_TRY(pf_upload(c, c->d_off.p, c->off.data(), sizeof(int64_t) * (K + 1)));
    return pf_upload(c, c->d_path_of.p, c->path_of.data(), sizeof(int32_t) * P);
}

int32_t staging_reserve(pfmi_ctx *c, int32_t K, size_t cap, int32_t d) {
    PF_TRY(c->st_theta.ensure(sizeof(double) * K * cap * d));
    PF_TRY(c->st_grad.ensure(sizeof(double) * K * cap * d));
    PF_TRY(c->st_lp.ensure(sizeof(double) * K * cap));
    PF_TRY(c->st_npts.ensure(sizeof(int32_t) * K));
    return c->lb_x0.ensure(sizeof(double) * (size_t)K * d);
}

// ---- closure optimisation (lbfgs_closure_kernel.hip): rounds of one step kernel + one closure call, scheduled by the pumping thread --------
#define PF_LBC_WINDOW 4                 // rounds in flight at most
// the round bookkeeping of a closure optimisation, packed (prog = null) or streamed (prog = the pipeline's progress words)
void lbc_begin(pfmi_ctx *c, int32_t K, int32_t J, int32_t maxiters, double g_tol, int32_t *prog) {
    LbcState &O = c->lbc;
    O.K = K; O.J = J; O.maxiters = maxiters; O.g_tol = g_tol;
    { const char *rj = pf_debug_get("PFMI_LBFGS_REJECT_EVERY"); O.reject_every = rj ? atoi(rj) : 0; }
    O.issued = 0; O.seen = 0; O.max_rounds = (int64_t)maxiters * (25 + 30) + 1; O.finished = false;
    O.rounds = 0; O.columns = 0; O.h_prog = prog;
    __atomic_store_n(c->lc_status, (int64_t)K, __ATOMIC_RELEASE);            // round 0: every path running
}

// Issues the rounds a closure optimisation may have in flight on stream `s` (the ctx stream: pfmi_optimize_batch_pump; s_opt: the streaming
// pipeline, pfmi_stream_pump): the gradient closure on all K trial points, with `s` as its stream, then the step kernel of the next round.
// At most PF_LBC_WINDOW rounds ahead of the last one whose progress word the host has read, never more than the hard cap.  Sets O.finished.
int32_t lbc_issue_rounds(pfmi_ctx *c, hipStream_t s) {
    LbcState &O = c->lbc;
    const int64_t w = __atomic_load_n(c->lc_status, __ATOMIC_ACQUIRE);
    const int64_t round = w >> 32, active = w & 0xffffffffll;
    if (round > O.seen) O.seen = round;
    if (round == O.seen && active == 0) O.finished = true;
    const TargetDev &T = c->target;
    const int d = T.d;
    while (!O.finished && O.issued < O.max_rounds && O.issued - O.seen < PF_LBC_WINDOW) {
        // the closure on all K trial points (written by the previous round), then the step kernel of the next round
        T.grad_fn(c->lc_X.as<double>(), d, O.K, c->lc_out.as<double>(), (void *)s, T.grad_user);
        O.columns += O.K;
        ++O.issued;
        PF_TRY(pf_launch_lbc_step(c, O.issued, s));
        O.rounds = O.issued;
    }
    if (!O.finished && O.issued >= O.max_rounds && O.seen >= O.issued) O.finished = true;      // the hard cap: a stuck flag cannot loop forever
    return PFMI_OK;
}

static int32_t lbc_enqueue(pfmi_ctx *c, int32_t K, const double *x0, int32_t J, int32_t maxiters, double g_tol) {
    const TargetDev &T = c->target;
    PF_CHECK(K > 0 && x0 && maxiters >= 0, PFMI_ERR_ARG, "optimize_batch: bad arguments");
    PF_CHECK(J >= 1 && J <= 32, PFMI_ERR_UNSUPPORTED, "optimize_batch: history_length %d outside 1..32 (closure target)", J);
    const int d = T.d;
    const size_t cap = (size_t)maxiters + 1;
    {   // everything the call allocates: staging trace, the closure's input / output, x, g, p, the ring, the Gram data
        size_t fr = 0, tot = 0;
        PF_HIP(hipMemGetInfo(&fr, &tot));
        const double need = 8.0 * K * ((double)cap * (2.0 * d + 1.0) + (6.0 + 2.0 * J) * d + 1.0) + (double)K * pf_lbc_path_state_bytes(J);
        PF_CHECK(need < 0.8 * (double)fr, PFMI_ERR_UNSUPPORTED, "optimize_batch: %.3g GB needed for K = %d, d = %d, J = %d, maxiters = %d; %.3g GB free",
                 need / 1e9, K, d, J, maxiters, (double)fr / 1e9);
    }
    PF_TRY(staging_reserve(c, K, cap, d));
    PF_TRY(pf_lbc_alloc(c, K, J, d));
    PF_TRY(pf_upload(c, c->lb_x0.p, x0, sizeof(double) * (size_t)K * d));
    // a streamed closure call may have left rounds behind its last one on s_opt (they find every path done, but still write the progress
    // word and the closure's buffers): they finish before this call reuses them
    if (c->s_opt) PF_HIP(hipStreamSynchronize(c->s_opt));
    lbc_begin(c, K, J, maxiters, g_tol, nullptr);
    c->lbc.active = true;                                                      // from here on, failure paths drain (lbc_abandon)
    c->opt_pending = true; c->opt_K = K; c->opt_cap = (int32_t)cap;
    results_reset(c); c->P = 0;
    pf_kernel_begin(c);
    const int32_t rc = pf_launch_lbc_init(c, c->stream);
    pf_kernel_end(c, "optimize");
    if (rc != PFMI_OK) lbc_abandon(c);
    return rc;
}

extern "C" {

// ---- inputs ------------------------------------------------------------------------------------------
int32_t pfmi_set_target(pfmi_ctx *c, const pfmi_target *t) {
    PF_CTX_MUT(c);
    PF_CHECK(t != nullptr, PFMI_ERR_ARG, "null target");
    PF_CHECK(t->d > 0, PFMI_ERR_ARG, "target dimension must be positive");
    lbc_abandon(c);
    hmc_forget(c);
    if (c->sr.active && c->sr.closure) stream_abandon(c);   // its pump would call the closures being replaced
    TargetDev &T = c->target;
    T.kind = t->kind; T.d = t->d; T.r = 0; T.rpad = 0; T.offset = 0.0; T.fn = nullptr; T.dev_fn = nullptr; T.user = nullptr;
    T.grad_fn = nullptr; T.grad_user = nullptr;
    if (t->kind == PFMI_TARGET_GAUSS) {
        PF_CHECK(t->mean && t->a, PFMI_ERR_ARG, "GAUSS target needs mean and a");
        PF_CHECK(t->r >= 0 && t->r <= 16, PFMI_ERR_UNSUPPORTED, "GAUSS target rank %d > 16 unsupported", t->r);
        PF_CHECK(t->r == 0 || (t->Wd && t->G), PFMI_ERR_ARG, "GAUSS target with r > 0 needs Wd and G");
        const int d = t->d, r = t->r, rpad = (r == 0) ? 0 : (r <= 8 ? 8 : 16);
        T.r = r; T.rpad = rpad; T.offset = t->offset;
        PF_TRY(T.mean.ensure(sizeof(double) * d));
        PF_TRY(T.a.ensure(sizeof(double) * d));
        PF_TRY(pf_upload(c, T.mean.p, t->mean, sizeof(double) * d));
        PF_TRY(pf_upload(c, T.a.p, t->a, sizeof(double) * d));
        if (r > 0) {
            std::vector<double> wd((size_t)d * rpad, 0.0), g((size_t)rpad * rpad, 0.0);
            for (int i = 0; i < d; ++i)
                for (int j = 0; j < r; ++j) wd[(size_t)i * rpad + j] = t->Wd[i + (size_t)d * j];
            for (int j = 0; j < r; ++j)
                for (int l = 0; l <= j; ++l) g[(size_t)j * rpad + l] = t->G[j + (size_t)r * l];
            PF_TRY(T.wd.ensure(sizeof(double) * wd.size()));
            PF_TRY(T.g.ensure(sizeof(double) * g.size()));
            PF_TRY(pf_upload(c, T.wd.p, wd.data(), sizeof(double) * wd.size()));
            PF_TRY(pf_upload(c, T.g.p, g.data(), sizeof(double) * g.size()));
            const size_t rows16 = ((size_t)d + 15) / 16 * 16;
            std::vector<double> w16(rows16 * 16, 0.0);
            for (int i = 0; i < d; ++i)
                for (int j = 0; j < r; ++j) w16[(size_t)i * 16 + j] = t->Wd[i + (size_t)d * j];
            PF_TRY(T.wd16.ensure(sizeof(double) * w16.size()));
            PF_TRY(pf_upload(c, T.wd16.p, w16.data(), sizeof(double) * w16.size()));
        }
    } else if (t->kind == PFMI_TARGET_FUNNEL) {
        /* no parameters */
    } else if (t->kind == PFMI_TARGET_HOST_CALLBACK) {
        PF_CHECK(t->fn != nullptr, PFMI_ERR_ARG, "HOST_CALLBACK target needs fn");
        T.fn = t->fn; T.user = t->user;
    } else if (t->kind == PFMI_TARGET_DEVICE_CALLBACK) {
        PF_CHECK(t->dev_fn != nullptr, PFMI_ERR_ARG, "DEVICE_CALLBACK target needs dev_fn");
        T.dev_fn = t->dev_fn; T.user = t->user;
    } else {
        T.kind = -1;
        PF_CHECK(false, PFMI_ERR_ARG, "unknown target kind %d", t->kind);
    }
    return PFMI_OK;
}

int32_t pfmi_set_traces(pfmi_ctx *c, int32_t K, const int64_t *npoints, int32_t d, const double *theta,
                        const double *grad) {
    PF_CTX_MUT(c);
    if (c->sr.active || c->stream_drain) stream_abandon(c);
    lbc_abandon(c);
    hmc_forget(c);
    PF_CHECK(K > 0 && d > 0 && npoints && theta && grad, PFMI_ERR_ARG, "set_traces: bad arguments");
    for (int k = 0; k < K; ++k) PF_CHECK(npoints[k] >= 1, PFMI_ERR_ARG, "path %d has no points", k);
    results_reset(c);
    PF_TRY(set_packed_layout(c, K, d, npoints));
    const size_t bytes = sizeof(double) * (size_t)c->P * d;
    PF_TRY(c->theta.ensure(bytes));
    PF_TRY(c->grad.ensure(bytes));
    PF_TRY(pf_upload(c, c->theta.p, theta, bytes));
    return pf_upload(c, c->grad.p, grad, bytes);
}

// ---- device trajectory generation ------------------------------------------------------------------------
int32_t pfmi_optimize_batch_enqueue(pfmi_ctx *c, int32_t K, const double *x0, int32_t J, int32_t maxiters, double g_tol) {
    PF_CTX_MUT(c);
    if (c->sr.active || c->stream_drain) stream_abandon(c);
    lbc_abandon(c);
    hmc_forget(c);
    const TargetDev &T = c->target;
    if (T.kind == PFMI_TARGET_DEVICE_CALLBACK && T.grad_fn) return lbc_enqueue(c, K, x0, J, maxiters, g_tol);
    c->lbc.rounds = 0; c->lbc.columns = 0;
    PF_CHECK(T.kind == PFMI_TARGET_GAUSS || T.kind == PFMI_TARGET_FUNNEL, PFMI_ERR_UNSUPPORTED,
             "optimize_batch: needs a built-in target or a DEVICE_CALLBACK target with a gradient closure (pfmi_set_target_gradient)");
    PF_CHECK(K > 0 && x0 && maxiters >= 0, PFMI_ERR_ARG, "optimize_batch: bad arguments");
    PF_CHECK(J >= 1 && J <= 16, PFMI_ERR_UNSUPPORTED, "optimize_batch: history_length %d outside 1..16", J);
    const int d = T.d;
    const size_t cap = (size_t)maxiters + 1;
    PF_TRY(staging_reserve(c, K, cap, d));
    PF_TRY(pf_upload(c, c->lb_x0.p, x0, sizeof(double) * (size_t)K * d));
    pf_kernel_begin(c);
    PF_TRY(pf_launch_lbfgs(c, K, J, maxiters, g_tol, c->lb_x0.as<double>()));
    pf_kernel_end(c, "optimize");
    c->opt_pending = true; c->opt_K = K; c->opt_cap = (int32_t)cap;
    results_reset(c); c->P = 0;
    return PFMI_OK;
}

int32_t pfmi_optimize_batch_wait(pfmi_ctx *c, int64_t *npoints) {
    PF_CTX_MUT(c);
    PF_CHECK(c->opt_pending, PFMI_ERR_STATE, "optimize_batch_wait: no pfmi_optimize_batch_enqueue outstanding");
    PF_CHECK(npoints != nullptr, PFMI_ERR_ARG, "optimize_batch_wait: null npoints");
    if (c->lbc.active) {
        int32_t fin = 0;
        while (true) {
            PF_TRY(pfmi_optimize_batch_pump(c, &fin));
            if (fin) break;
            for (int i = 0; i < 64; ++i) __builtin_ia32_pause();
        }
        c->lbc.active = false;                      // (the downloads below synchronise the stream behind the last round)
    }
    c->opt_pending = false;
    const int K = c->opt_K, d = c->target.d;
    const size_t cap = (size_t)c->opt_cap;
    std::vector<int32_t> np32((size_t)K);
    PF_TRY(d2h(c, np32.data(), c->st_npts.p, sizeof(int32_t) * K));
    for (int k = 0; k < K; ++k) {
        PF_CHECK(np32[(size_t)k] >= 1 && (size_t)np32[(size_t)k] <= cap, PFMI_ERR_NUMERIC, "optimize_batch: path %d produced %d points", k,
                 np32[(size_t)k]);
        npoints[k] = np32[(size_t)k];
    }
    PF_TRY(set_packed_layout(c, K, d, npoints));
    const size_t bytes = sizeof(double) * (size_t)c->P * d;
    PF_TRY(c->theta.ensure(bytes));
    PF_TRY(c->grad.ensure(bytes));
    PF_TRY(c->trace_lp.ensure(sizeof(double) * c->P));
    pf_kernel_begin(c);
    PF_TRY(pf_launch_trace_pack(c, (int64_t)cap));
    pf_kernel_end(c, "trace_pack");
    c->have_trace_lp = true;
    return PFMI_OK;
}

int32_t pfmi_optimize_batch(pfmi_ctx *c, int32_t K, const double *x0, int32_t J, int32_t maxiters, double g_tol,
                            int64_t *npoints) {
    PF_CHECK(npoints != nullptr, PFMI_ERR_ARG, "optimize_batch: bad arguments");
    PF_TRY(pfmi_optimize_batch_enqueue(c, K, x0, J, maxiters, g_tol));
    return pfmi_optimize_batch_wait(c, npoints);
}

int32_t pfmi_set_target_gradient(pfmi_ctx *c, pfmi_logp_dev_fn logp_grad_fn, void *user) {
    PF_CTX(c);
    PF_CHECK(c->target.kind == PFMI_TARGET_DEVICE_CALLBACK, PFMI_ERR_ARG, "set_target_gradient: the current target is not a DEVICE_CALLBACK target");
    PF_CHECK(logp_grad_fn != nullptr, PFMI_ERR_ARG, "set_target_gradient: null closure");
    lbc_abandon(c);
    hmc_forget(c);
    if (c->sr.active && c->sr.closure) stream_abandon(c);
    c->target.grad_fn = logp_grad_fn; c->target.grad_user = user;
    return PFMI_OK;
}

static int32_t lbc_pump_pass(pfmi_ctx *c, int32_t *finished) {
    LbcState &O = c->lbc;
    PF_TRY(lbc_issue_rounds(c, c->stream));
    if (!O.finished) {
        const hipError_t e = hipStreamQuery(c->stream);
        PF_CHECK(e == hipSuccess || e == hipErrorNotReady, PFMI_ERR_HIP, "optimize_batch_pump: %s", hipGetErrorString(e));
    }
    *finished = O.finished ? 1 : 0;
    return PFMI_OK;
}

int32_t pfmi_optimize_batch_pump(pfmi_ctx *c, int32_t *finished) {
    PF_CHECK(c != nullptr && finished != nullptr, PFMI_ERR_ARG, "optimize_batch_pump: null argument");
    PF_CHECK(c->lbc.active, PFMI_ERR_STATE, "optimize_batch_pump: no closure optimisation outstanding");
    PF_HIP(hipSetDevice(c->device));
    const int32_t rc = lbc_pump_pass(c, finished);
    if (rc != PFMI_OK) lbc_abandon(c);        // a failed pass ends the call: what is in flight is drained, the context is usable again
    return rc;
}

int32_t pfmi_optimize_batch_cancel(pfmi_ctx *c) {
    PF_CHECK(c != nullptr, PFMI_ERR_ARG, "null pfmi_ctx");
    PF_HIP(hipSetDevice(c->device));
    lbc_abandon(c);
    return PFMI_OK;
}

int32_t pfmi_optimize_stats(pfmi_ctx *c, int64_t *rounds, int64_t *closure_columns) {
    PF_CHECK(c != nullptr, PFMI_ERR_ARG, "null pfmi_ctx");
    if (rounds) *rounds = c->lbc.rounds;
    if (closure_columns) *closure_columns = c->lbc.columns;
    return PFMI_OK;
}

int32_t pfmi_get_trace(pfmi_ctx *c, int32_t k, double *theta, double *logp, double *grad) {
    PF_CTX(c);
    PF_CHECK(c->P > 0 && k >= 0 && k < c->K, PFMI_ERR_ARG, "get_trace: bad path index");
    const int64_t p0 = c->off[(size_t)k], n = c->path_npts(k);
    const size_t bytes = sizeof(double) * (size_t)n * c->d;
    if (theta) PF_TRY(d2h(c, theta, c->th() + (size_t)p0 * c->d, bytes));
    if (grad) PF_TRY(d2h(c, grad, c->gr() + (size_t)p0 * c->d, bytes));
    if (logp) {
        PF_CHECK(c->have_trace_lp, PFMI_ERR_STATE, "get_trace: log densities exist only for pfmi_optimize_batch traces");
        PF_TRY(d2h(c, logp, c->tlp() + p0, sizeof(double) * n));
    }
    return PFMI_OK;
}

}  // extern "C"
