// api_nuts.hip -- NUTS on a fitted metric for gradient closures: the entry points of include/pfmi.h over nuts_kernel.hip.  The chains, the
// closure buffers and the record buffers are static HMC's (api_hmc.hip: pfmi_hmc_get, pfmi_hmc_draws_dev and pfmi_chain_diagnostics serve a
// NUTS run unchanged); the rounds are scheduled as the closure L-BFGS's are (lbc_issue_rounds, api_inputs.hip).
#include "api_internal.h"

#include <math.h>
#include <vector>

#define PF_NUTS_WINDOW 4                // rounds in flight at most

// Issues the rounds a NUTS run may have in flight: the gradient closure on all K trial points, then the step kernel that consumes its answer.
// At most PF_NUTS_WINDOW rounds ahead of the last one whose progress word the host has read, never more than the hard cap.  Sets H.finished.
static int32_t nuts_issue_rounds(pfmi_ctx *c) {
    HmcState &H = c->hmc;
    const TargetDev &Tg = c->target;
    const int64_t w = __atomic_load_n(c->nt_status, __ATOMIC_ACQUIRE);
    const int64_t round = w >> 32, active = w & 0xffffffffll;
    if (round > H.seen) H.seen = round;
    if (round == H.seen && active == 0) H.finished = true;
    while (!H.finished && H.issued < H.max_rounds && H.issued - H.seen < PF_NUTS_WINDOW) {
        pf_kernel_begin(c);
        Tg.grad_fn(c->hm_X.as<double>(), c->d, H.K, c->hm_out.as<double>(), (void *)c->stream, Tg.grad_user);
        pf_kernel_end(c, H.adapting ? "nuts_adapt_closure" : "nuts_closure");
        H.columns += H.K;
        const int64_t prow = H.issued++;
        pf_kernel_begin(c);
        PF_TRY(pf_launch_nuts_step(c, H.issued, prow, false, c->stream));
        pf_kernel_end(c, H.adapting ? "nuts_adapt" : "nuts");
    }
    if (!H.finished && H.issued >= H.max_rounds && H.seen >= H.issued) H.finished = true;      // the hard cap: a stuck flag cannot loop forever
    return PFMI_OK;
}

static int32_t nuts_pump_pass(pfmi_ctx *c, int32_t *finished) {
    HmcState &H = c->hmc;
    PF_TRY(nuts_issue_rounds(c));
    if (!H.finished) {
        const hipError_t e = hipStreamQuery(c->stream);
        PF_CHECK(e == hipSuccess || e == hipErrorNotReady, PFMI_ERR_HIP, "nuts_pump: %s", hipGetErrorString(e));
    }
    *finished = H.finished ? 1 : 0;
    return PFMI_OK;
}

static int32_t nuts_drain(pfmi_ctx *c) {                  // pump to the end (every pass is bounded by the window, the run by the cap)
    int32_t fin = c->hmc.finished ? 1 : 0;
    while (!fin) {
        PF_TRY(nuts_pump_pass(c, &fin));
        if (!fin) for (int i = 0; i < 64; ++i) __builtin_ia32_pause();
    }
    return PFMI_OK;
}

int32_t nuts_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                     int32_t max_depth, int64_t T, int32_t flags, int64_t W, double delta) {
    HmcState &H = c->hmc;
    const TargetDev &Tg = c->target;
    const bool cont = (flags & PFMI_NUTS_CONTINUE) != 0, rec = (flags & PFMI_NUTS_RECORD_PATH) != 0;
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "nuts_enqueue: call pfmi_fit_batch first");
    PF_CHECK(Tg.kind == PFMI_TARGET_DEVICE_CALLBACK && Tg.grad_fn != nullptr, PFMI_ERR_UNSUPPORTED,
             "nuts_enqueue: needs a DEVICE_CALLBACK target with a gradient closure (pfmi_set_target_gradient)");
    PF_CHECK(Tg.d == c->d, PFMI_ERR_STATE, "nuts_enqueue: the target's dimension %d is not the fit's %d", Tg.d, c->d);
    PF_CHECK(K >= 1 && points && seeds && step_size && (cont || x0), PFMI_ERR_ARG, "nuts_enqueue: K < 1 or a null argument");
    PF_CHECK(max_depth >= 1 && max_depth <= 10 && T >= 1, PFMI_ERR_ARG, "nuts_enqueue: max_depth %d outside 1 .. 10 or ntransitions %lld < 1", max_depth,
             (long long)T);
    PF_CHECK((flags & ~(PFMI_NUTS_CONTINUE | PFMI_NUTS_RECORD_PATH)) == 0, PFMI_ERR_ARG, "nuts_enqueue: unknown flags %d", flags);
    for (int k = 0; k < K; ++k) {
        PF_CHECK(points[k] >= 0 && points[k] < c->P, PFMI_ERR_ARG, "nuts_enqueue: point %lld of chain %d outside [0, %lld)", (long long)points[k], k,
                 (long long)c->P);
        PF_CHECK(isfinite(step_size[k]) && step_size[k] > 0.0, PFMI_ERR_ARG, "nuts_enqueue: step size of chain %d is not positive and finite", k);
    }
    PF_CHECK(!cont || (H.have && H.K == K), PFMI_ERR_STATE, "nuts_enqueue: PFMI_NUTS_CONTINUE without %d resident chains", K);
    PF_CHECK(!cont || H.kind == 1, PFMI_ERR_STATE, "nuts_enqueue: PFMI_NUTS_CONTINUE on the chains of pfmi_hmc_enqueue");
    PF_CHECK(!cont || H.md_alloc >= max_depth, PFMI_ERR_ARG, "nuts_enqueue: PFMI_NUTS_CONTINUE with max_depth %d above the chains' %d", max_depth,
             H.md_alloc);
    PF_CHECK(((double)W + (double)T) * 1024.0 < 2147483648.0, PFMI_ERR_UNSUPPORTED, "nuts_enqueue: %lld transitions in one call", (long long)(W + T));
    const int d = c->d;
    const int64_t rounds = (cont ? 0 : 1) + (W + T) * (((int64_t)1 << max_depth) - 1);
    {   // the fits the chains ask for are successes
        std::vector<int32_t> st((size_t)c->P);
        PF_TRY(d2h(c, st.data(), c->status.p, sizeof(int32_t) * (size_t)c->P));
        for (int k = 0; k < K; ++k)
            PF_CHECK(st[(size_t)points[k]] == PFMI_FIT_OK, PFMI_ERR_NUMERIC, "nuts_enqueue: the fit of point %lld (chain %d) has status %d",
                     (long long)points[k], k, st[(size_t)points[k]]);
    }
    const size_t vec = sizeof(double) * (size_t)K * d, rows = (size_t)K * (size_t)T;
    const size_t out_bytes = sizeof(double) * (size_t)K * (d + 1);
    const size_t ev_bytes = sizeof(pfmi_nuts_event) * (size_t)K * (size_t)rounds;
    {   // what the call's `ensure`s below will grow, checkpoints and (RECORD_PATH) one path row per round of the cap included
        size_t fr = 0, tot = 0;
        PF_HIP(hipMemGetInfo(&fr, &tot));
        double need = 0.0;
        auto grow = [&](const DevBuf &b, size_t bytes) { if (bytes > b.cap) need += (double)bytes; };
        if (!cont) {
            for (const DevBuf *b : {&c->hm_X, &c->hm_x0}) grow(*b, vec);
            grow(c->hm_out, out_bytes);
            grow(c->nt_vec, vec * (size_t)pf_nuts_vec_slots(max_depth));
        }
        grow(c->hm_draws, sizeof(double) * rows * d);
        for (const DevBuf *b : {&c->hm_lp, &c->hm_acc, &c->hm_de}) grow(*b, sizeof(double) * rows);
        for (const DevBuf *b : {&c->hm_div, &c->nt_depth, &c->nt_nleap}) grow(*b, sizeof(int32_t) * rows);
        if (W) grow(c->hm_adapt, adapt_bytes(K, W));
        if (rec) {
            grow(c->hm_pX, vec * (size_t)rounds);
            grow(c->hm_pv, vec * (size_t)rounds);
            grow(c->hm_pout, out_bytes * (size_t)rounds);
            grow(c->nt_pev, ev_bytes);
        }
        PF_CHECK(need < 0.8 * (double)fr, PFMI_ERR_UNSUPPORTED,
                 "nuts_enqueue: %.3g GB more needed for K = %d, d = %d, %lld transitions, max_depth %d; %.3g GB free", need / 1e9, K, d, (long long)T,
                 max_depth, (double)fr / 1e9);
    }
    if (!cont) {
        hmc_forget(c);
        for (DevBuf *b : {&c->hm_X, &c->hm_x0}) PF_TRY(b->ensure(vec));
        PF_TRY(c->hm_out.ensure(out_bytes));
        PF_TRY(c->nt_vec.ensure(vec * (size_t)pf_nuts_vec_slots(max_depth)));
        PF_TRY(c->nt_st.ensure(pf_nuts_chain_bytes() * (size_t)K));
        PF_TRY(c->nt_ctr.ensure(sizeof(int32_t) * 2));
        PF_TRY(c->hm_pts.ensure(sizeof(int32_t) * (size_t)K));
        PF_TRY(c->hm_seeds.ensure(sizeof(uint64_t) * (size_t)K));
        PF_TRY(c->hm_eps.ensure(sizeof(double) * (size_t)K));
        if (!c->nt_status) PF_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->nt_status), sizeof(int64_t), hipHostMallocCoherent | hipHostMallocMapped));
    } else {
        PF_TRY(nuts_drain(c));                            // the rounds of the call before, whose records are rewritten (and may be reallocated)
        PF_HIP(hipStreamSynchronize(c->stream));
        H.active = false;
    }
    PF_TRY(c->hm_draws.ensure(sizeof(double) * rows * d));
    for (DevBuf *b : {&c->hm_lp, &c->hm_acc, &c->hm_de}) PF_TRY(b->ensure(sizeof(double) * rows));
    for (DevBuf *b : {&c->hm_div, &c->nt_depth, &c->nt_nleap}) PF_TRY(b->ensure(sizeof(int32_t) * rows));
    if (rec) {
        PF_TRY(c->hm_pX.ensure(vec * (size_t)rounds));
        PF_TRY(c->hm_pv.ensure(vec * (size_t)rounds));
        PF_TRY(c->hm_pout.ensure(out_bytes * (size_t)rounds));
        PF_TRY(c->nt_pev.ensure(ev_bytes));
        PF_HIP(hipMemsetAsync(c->nt_pev.p, 0xff, ev_bytes, c->stream));        // t = -1: a column no running chain wrote
    }
    std::vector<int32_t> p32((size_t)K);
    for (int k = 0; k < K; ++k) p32[(size_t)k] = (int32_t)points[k];
    PF_TRY(pf_upload(c, c->hm_pts.p, p32.data(), sizeof(int32_t) * (size_t)K));
    PF_TRY(pf_upload(c, c->hm_seeds.p, seeds, sizeof(uint64_t) * (size_t)K));
    if (cont) PF_TRY(adapt_keep_step_sizes(c));
    PF_TRY(pf_upload(c, c->hm_eps.p, step_size, sizeof(double) * (size_t)K));
    if (!cont) PF_TRY(pf_upload(c, c->hm_x0.p, x0, vec));
    if (W) PF_TRY(adapt_reserve(c, K, W, step_size, delta));
    H.adapting = W > 0;
    if (W) H.W = W;
    H.K = K; H.nleap = 0; H.record = rec; H.kind = 1;
    H.max_depth = max_depth;
    if (!cont) H.md_alloc = max_depth;                    // (a CONTINUE never asks for more checkpoints than the chains were given)
    H.t0 = cont ? H.t0 + H.T : W; H.T = T;
    H.rounds = 0; H.columns = 0; H.path_rounds = rec ? rounds : 0;
    H.issued = 0; H.seen = 0; H.max_rounds = rounds; H.finished = false;
    H.have = true; H.active = true;                       // from here on, failure paths drain (pfmi_nuts_enqueue)
    __atomic_store_n(c->nt_status, (int64_t)K, __ATOMIC_RELEASE);               // round 0: every chain running
    PF_HIP(hipMemsetAsync(c->nt_ctr.p, 0, sizeof(int32_t) * 2, c->stream));
    if (!cont) PF_TRY(pf_launch_nuts_init(c, c->stream));
    else {
        pf_kernel_begin(c);
        PF_TRY(pf_launch_nuts_step(c, 0, 0, true, c->stream));
        pf_kernel_end(c, "nuts");
    }
    return nuts_issue_rounds(c);
}

extern "C" {

int32_t pfmi_nuts_enqueue(pfmi_ctx *c, int32_t K, const int64_t *points, const double *x0, const uint64_t *seeds, const double *step_size,
                          int32_t max_depth, int64_t ntransitions, int32_t flags) {
    PF_CTX_MUT(c);
    const int32_t rc = nuts_enqueue(c, K, points, x0, seeds, step_size, max_depth, ntransitions, flags, 0, 0.0);
    if (rc != PFMI_OK) {                                  // an error exit drains this ctx's stream and leaves no chains behind
        (void)hipStreamSynchronize(c->stream);
        c->hmc.active = false; c->hmc.have = false; c->hmc.finished = true;
    }
    return rc;
}

int32_t pfmi_nuts_pump(pfmi_ctx *c, int32_t *finished) {
    PF_CHECK(c != nullptr && finished != nullptr, PFMI_ERR_ARG, "nuts_pump: null argument");
    PF_CHECK(c->hmc.have && c->hmc.kind == 1, PFMI_ERR_STATE, "nuts_pump: no pfmi_nuts_enqueue outstanding");
    PF_HIP(hipSetDevice(c->device));
    const int32_t rc = nuts_pump_pass(c, finished);
    if (rc != PFMI_OK) { c->hmc.finished = true; hmc_forget(c); }      // a failed pass ends the run: what is in flight is drained
    return rc;
}

int32_t pfmi_nuts_wait(pfmi_ctx *c) {
    PF_CTX(c);
    HmcState &H = c->hmc;
    PF_CHECK(H.have && H.kind == 1, PFMI_ERR_STATE, "nuts_wait: no pfmi_nuts_enqueue outstanding");
    const int32_t rc = nuts_drain(c);
    if (rc != PFMI_OK) { H.finished = true; hmc_forget(c); return rc; }
    PF_TRY(pf_stream_sync(c));
    H.active = false;
    std::vector<int32_t> dead;
    int64_t last = 0;
    PF_TRY(pf_nuts_chain_flags(c, dead, &last));
    H.rounds = last;
    for (int k = 0; k < H.K; ++k)
        if (dead[(size_t)k]) {
            H.have = false;
            PF_CHECK(false, PFMI_ERR_NUMERIC, "nuts: the start point of chain %d has a non-finite log density or gradient", k);
        }
    return PFMI_OK;
}

int32_t pfmi_nuts_get_stats(pfmi_ctx *c, int32_t *tree_depth, int32_t *n_leapfrog) {
    PF_CTX(c);
    const HmcState &H = c->hmc;
    PF_CHECK(H.have && H.kind == 1, PFMI_ERR_STATE, "nuts_get_stats: no NUTS run on this ctx");
    PF_CHECK(H.finished, PFMI_ERR_STATE, "nuts_get_stats: the run has rounds to go (pfmi_nuts_wait)");
    const size_t rows = (size_t)H.K * (size_t)H.T;
    if (tree_depth) PF_TRY(pf_download(c, tree_depth, c->nt_depth.p, sizeof(int32_t) * rows));
    if (n_leapfrog) PF_TRY(pf_download(c, n_leapfrog, c->nt_nleap.p, sizeof(int32_t) * rows));
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    return PFMI_OK;
}

int32_t pfmi_nuts_get_path(pfmi_ctx *c, int64_t round0, int64_t nrounds, double *X, double *closure_out, double *v, pfmi_nuts_event *events) {
    PF_CTX(c);
    const HmcState &H = c->hmc;
    PF_CHECK(H.have && H.record && H.kind == 1, PFMI_ERR_STATE, "nuts_get_path: the last pfmi_nuts_enqueue did not run with PFMI_NUTS_RECORD_PATH");
    PF_CHECK(H.finished, PFMI_ERR_STATE, "nuts_get_path: the run has rounds to go (pfmi_nuts_wait)");
    PF_CHECK(round0 >= 0 && nrounds >= 0 && round0 + nrounds <= H.issued, PFMI_ERR_ARG, "nuts_get_path: rounds [%lld, %lld) outside [0, %lld)",
             (long long)round0, (long long)(round0 + nrounds), (long long)H.issued);
    const size_t vec = (size_t)H.K * c->d, ovec = (size_t)H.K * (c->d + 1);
    if (X) PF_TRY(pf_download(c, X, c->hm_pX.as<double>() + (size_t)round0 * vec, sizeof(double) * vec * (size_t)nrounds));
    if (v) PF_TRY(pf_download(c, v, c->hm_pv.as<double>() + (size_t)round0 * vec, sizeof(double) * vec * (size_t)nrounds));
    if (closure_out) PF_TRY(pf_download(c, closure_out, c->hm_pout.as<double>() + (size_t)round0 * ovec, sizeof(double) * ovec * (size_t)nrounds));
    if (events)
        PF_TRY(pf_download(c, events, c->nt_pev.as<pfmi_nuts_event>() + (size_t)round0 * H.K, sizeof(pfmi_nuts_event) * (size_t)H.K * (size_t)nrounds));
    PF_TRY(pf_stream_sync(c));
    c->hmc.active = false;
    return PFMI_OK;
}

int32_t pfmi_nuts_stats(pfmi_ctx *c, int64_t *rounds, int64_t *closure_columns) {
    PF_CHECK(c != nullptr, PFMI_ERR_ARG, "null pfmi_ctx");
    PF_CHECK(c->hmc.kind == 1, PFMI_ERR_STATE, "nuts_stats: no NUTS run on this ctx");
    if (rounds) *rounds = c->hmc.rounds;
    if (closure_columns) *closure_columns = c->hmc.columns;
    return PFMI_OK;
}

}  // extern "C"
