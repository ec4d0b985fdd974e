// api_pool.hip -- the pooled stage: pool of draws, PSIS, resampling, gather.
#include "api_internal.h"

#include <math.h>
#include <vector>

// ---- pool / PSIS / resample ---------------------------------------------------------------------------
static int32_t pool_alloc(pfmi_ctx *c, int64_t N_r) {
    const int K = c->K, d = c->d;
    c->N_r = N_r;
    const size_t S = (size_t)K * N_r;
    PF_TRY(c->pool.ensure(sizeof(double) * S * d));
    PF_TRY(c->pool_lr.ensure(sizeof(double) * S));
    PF_TRY(c->pool_lp.ensure(sizeof(double) * S));
    PF_TRY(c->pool_lq.ensure(sizeof(double) * S));
    PF_TRY(c->pool_points.ensure(sizeof(int32_t) * K));
    PF_TRY(c->pool_seeds.ensure(sizeof(uint64_t) * K));
    c->pool_mix_done = false;              // the mixture-proposal ratios belong to the pool they were formed on
    c->pool_lmix_ok = false;
    c->tr_base = 0;                        // a new pool is a pool as built: no transform state survives
    c->tr_undo = 0;
    if (c->tr_bytes != 0 && c->tr_bytes != sizeof(double) * S * d) {   // spare sets made for a pool of another size are freed (a rebuild
        PF_HIP(hipStreamSynchronize(c->stream));                       // of the same size -- the summaries of a moment-matched result --
        for (pfmi_ctx::PoolSet *s : {&c->tr_a, &c->tr_b}) {            // keeps them and allocates nothing)
            s->x.release(); s->lp.release(); s->lq.release(); s->lr.release(); s->lr_mix.release();
        }
        c->tr_bytes = 0;
    }
    return PFMI_OK;
}

// draws of the K fits in pool_points / pool_seeds (device) -> pool, log ratios
static int32_t pool_fill(pfmi_ctx *c) {
    const int K = c->K, d = c->d;
    const int64_t N_r = c->N_r;
    const size_t S = (size_t)K * N_r;
    const bool cb = c->target.kind == PFMI_TARGET_HOST_CALLBACK, dcb = c->target.kind == PFMI_TARGET_DEVICE_CALLBACK;
    PF_TRY(pf_launch_elbo_draws(c, c->pool_points.as<int32_t>(), c->pool_seeds.as<uint64_t>(), K, 0, N_r, nullptr, 0,
                                c->pool.as<double>(), (int64_t)N_r * d, c->pool_lp.as<double>(),
                                c->pool_lq.as<double>(), N_r, !cb && !dcb, false));
    if (cb) PF_TRY(callback_logp(c, c->pool.as<double>(), (int64_t)S, c->pool_lp.as<double>()));
    if (dcb) PF_TRY(devcb_logp(c, c->pool.as<double>(), (int64_t)S, c->pool_lp.as<double>(), c->pool_points.as<int32_t>(), K, N_r));
    PF_TRY(pf_launch_logratio(c, (int64_t)S));
    c->pooled = true;
    return PFMI_OK;
}

// what the passes over the pool (pfmi_pool_moments / _cdf / _cross / _apply) check first: a pool, the entry point's own arguments (arg_error:
// its complaint, or NULL), a col_offset >= 0 and, with importance weighting, PSIS weights on this ctx that cover the pool's columns
// [col_offset, col_offset + K N_r) of the global pool.  arg_error exists to keep each entry point's message and the place of its
// check between the pool's and the weights'; pfmi_pool_cross words the offset and its NULL output as ONE complaint, so for it the
// col_offset check below never fires.
static int32_t pool_pass_check(pfmi_ctx *c, const char *name, int64_t col_offset, int32_t importance, const char *arg_error = nullptr) {
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "%s: call pfmi_pool_build first", name);
    PF_CHECK(!arg_error, PFMI_ERR_ARG, "%s: %s", name, arg_error);
    PF_CHECK(col_offset >= 0, PFMI_ERR_ARG, "%s: negative col_offset", name);
    const int64_t end = col_offset + (int64_t)c->K * c->N_r;
    PF_CHECK(!importance || (c->S_w > 0 && end <= c->S_w), PFMI_ERR_STATE,
             "%s: no PSIS weights for columns [%lld, %lld) on this ctx (run pfmi_psis / pfmi_comm_pool_psis first)", name,
             (long long)col_offset, (long long)end);
    return PFMI_OK;
}

// an optional host vector of n doubles on the device: *dev = buf, grown and filled on the ctx stream, or NULL when host is NULL
static int32_t upload_optional(pfmi_ctx *c, DevBuf &buf, const double *host, size_t n, const double **dev) {
    *dev = nullptr;
    if (!host) return PFMI_OK;
    PF_TRY(buf.ensure(sizeof(double) * n));
    PF_TRY(pf_upload(c, buf.p, host, sizeof(double) * n));
    *dev = buf.as<double>();
    return PFMI_OK;
}

// ---- pfmi_pool_transform: the current pool state against a spare set, whole buffers at a time
#define PF_TR_UNDO_TO_BUILT 1     // the call moved the pool as built: swap with tr_a, the current state is the pool as built again
#define PF_TR_UNDO_TO_MOVED 2     // the call moved a moved pool: swap with tr_b
#define PF_TR_UNDO_IDENTITY 3     // the call restored the pool as built over a moved pool: swap with tr_a, then with tr_b
#define PF_TR_UNDO_NOTHING 4      // the call restored the pool as built and it was current already

static void devbuf_swap(DevBuf &a, DevBuf &b) {
    void *p = a.p; a.p = b.p; b.p = p;
    const size_t cap = a.cap; a.cap = b.cap; b.cap = cap;
}
static void pool_set_swap(pfmi_ctx *c, pfmi_ctx::PoolSet &s) {
    devbuf_swap(c->pool, s.x); devbuf_swap(c->pool_lp, s.lp); devbuf_swap(c->pool_lq, s.lq); devbuf_swap(c->pool_lr, s.lr);
    devbuf_swap(c->pool_lr_mix, s.lr_mix);
}

// the moved pool into the current buffers (tr_a holds the pool as built): the pass, the closures as pool_fill runs them, the ratios
static int32_t pool_transform_fill(pfmi_ctx *c, const double *d_scale, const double *d_shift, double sla) {
    const int K = c->K;
    const int64_t N_r = c->N_r;
    const size_t S = (size_t)K * N_r;
    const bool cb = c->target.kind == PFMI_TARGET_HOST_CALLBACK, dcb = c->target.kind == PFMI_TARGET_DEVICE_CALLBACK;
    PF_TRY(pf_launch_pool_transform(c, c->tr_a.x.as<double>(), d_scale, d_shift, c->pool.as<double>(), c->pool_lp.as<double>()));
    if (cb) PF_TRY(callback_logp(c, c->pool.as<double>(), (int64_t)S, c->pool_lp.as<double>()));
    if (dcb) PF_TRY(devcb_logp(c, c->pool.as<double>(), (int64_t)S, c->pool_lp.as<double>(), c->pool_points.as<int32_t>(), K, N_r));
    return pf_launch_pool_transform_ratio(c, sla, c->tr_a.lq.as<double>(), c->pool_lmix_ok ? c->pool_lmix.as<double>() : nullptr,
                                          c->pool_lp.as<double>(), c->pool_lq.as<double>(), c->pool_lr.as<double>(),
                                          c->pool_lmix_ok ? c->pool_lr_mix.as<double>() : nullptr);
}

extern "C" {

int32_t pfmi_pool_transform(pfmi_ctx *c, const double *scale, const double *shift, double *logp_out, double *log_ratios_out) {
    PF_CTX_MUT(c);
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_transform: call pfmi_pool_build first");
    const int d = c->d;
    const size_t S = (size_t)c->K * c->N_r;
    double sla = 0.0;
    for (int i = 0; i < d; ++i) {
        PF_CHECK(!scale || (scale[i] > 0.0 && scale[i] <= 1.7976931348623157e308), PFMI_ERR_ARG,
                 "pool_transform: scale[%d] = %g is not positive and finite", i, scale[i]);
        PF_CHECK(!shift || (shift[i] >= -1.7976931348623157e308 && shift[i] <= 1.7976931348623157e308), PFMI_ERR_ARG,
                 "pool_transform: shift[%d] = %g is not finite", i, shift[i]);
        if (scale) sla += log(scale[i]);                                // index order: the ONE statement of sum log scale
    }
    const bool mix_before = c->pool_mix_done;
    if (!scale && !shift) {                                             // the pool as built, without a pass
        if (c->tr_base == 0) {
            c->tr_undo = PF_TR_UNDO_NOTHING;
        } else {
            pool_set_swap(c, c->tr_b);
            pool_set_swap(c, c->tr_a);
            c->tr_base = 0;
            c->tr_undo = PF_TR_UNDO_IDENTITY;
            c->pool_mix_done = c->pool_lmix_ok;
        }
        c->tr_undo_mix = mix_before;
    } else {
        std::vector<double> h((size_t)2 * d);
        for (int i = 0; i < d; ++i) { h[(size_t)i] = scale ? scale[i] : 1.0; h[(size_t)d + i] = shift ? shift[i] : 0.0; }
        PF_TRY(c->tr_scale.ensure(sizeof(double) * d));
        PF_TRY(c->tr_shift.ensure(sizeof(double) * d));
        pfmi_ctx::PoolSet &keep = c->tr_base == 0 ? c->tr_a : c->tr_b;  // where the state before the call goes
        PF_TRY(keep.x.ensure(sizeof(double) * S * d));                  // (every allocation before the first swap: a failure leaves the pool as it was)
        PF_TRY(keep.lp.ensure(sizeof(double) * S));
        PF_TRY(keep.lq.ensure(sizeof(double) * S));
        PF_TRY(keep.lr.ensure(sizeof(double) * S));
        if (c->pool_lmix_ok) PF_TRY(keep.lr_mix.ensure(sizeof(double) * S));
        PF_TRY(pf_upload(c, c->tr_scale.p, h.data(), sizeof(double) * d));
        PF_TRY(pf_upload(c, c->tr_shift.p, h.data() + d, sizeof(double) * d));
        c->tr_bytes = sizeof(double) * S * d;
        const int base_before = c->tr_base;
        pool_set_swap(c, keep);
        c->tr_base = 1;
        const int32_t rc = pool_transform_fill(c, c->tr_scale.as<double>(), c->tr_shift.as<double>(), sla);
        if (rc != PFMI_OK) {                                            // nothing happened
            pool_set_swap(c, keep);
            c->tr_base = base_before;
            return rc;
        }
        c->tr_undo = base_before == 0 ? PF_TR_UNDO_TO_BUILT : PF_TR_UNDO_TO_MOVED;
        c->tr_undo_mix = mix_before;
        c->pool_mix_done = c->pool_lmix_ok;
    }
    if (logp_out) PF_TRY(pf_download(c, logp_out, c->pool_lp.p, sizeof(double) * S));
    if (log_ratios_out) PF_TRY(pf_download(c, log_ratios_out, c->pool_lr.p, sizeof(double) * S));
    return pf_stream_sync(c);
}

int32_t pfmi_pool_transform_revert(pfmi_ctx *c) {
    PF_CTX_MUT(c);
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_transform_revert: call pfmi_pool_build first");
    PF_CHECK(c->tr_undo != 0, PFMI_ERR_STATE, "pool_transform_revert: no pfmi_pool_transform to undo");
    PF_HIP(hipStreamSynchronize(c->stream));
    switch (c->tr_undo) {
    case PF_TR_UNDO_TO_BUILT: pool_set_swap(c, c->tr_a); c->tr_base = 0; break;
    case PF_TR_UNDO_TO_MOVED: pool_set_swap(c, c->tr_b); break;
    case PF_TR_UNDO_IDENTITY: pool_set_swap(c, c->tr_a); pool_set_swap(c, c->tr_b); c->tr_base = 1; break;
    default: break;
    }
    c->pool_mix_done = c->tr_undo_mix;
    c->tr_undo = 0;
    return PFMI_OK;
}

int32_t pfmi_pool_build(pfmi_ctx *c, int64_t N_r, const int64_t *points, const uint64_t *seeds) {
    PF_CTX_MUT(c);
    PF_CHECK(c->fitted, PFMI_ERR_STATE, "pool_build: call pfmi_fit_batch first");
    PF_CHECK(c->target.kind >= 0, PFMI_ERR_STATE, "pool_build: call pfmi_set_target first");
    PF_CHECK(N_r >= 1 && points && seeds, PFMI_ERR_ARG, "pool_build: bad arguments");
    const int K = c->K;
    std::vector<int32_t> pts((size_t)K);
    for (int k = 0; k < K; ++k) {
        PF_CHECK(points[k] >= c->off[k] && points[k] < c->off[k] + c->path_npts(k), PFMI_ERR_ARG,
                 "pool_build: point %lld does not belong to path %d", (long long)points[k], k);
        pts[(size_t)k] = (int32_t)points[k];
    }
    PF_TRY(pool_alloc(c, N_r));
    PF_TRY(pf_upload(c, c->pool_points.p, pts.data(), sizeof(int32_t) * K));
    PF_TRY(pf_upload(c, c->pool_seeds.p, seeds, sizeof(uint64_t) * K));
    c->pool_from_best = false;
    return pool_fill(c);
}

int32_t pfmi_pool_build_best(pfmi_ctx *c, int64_t N_r, const uint64_t *fail_seeds) {
    PF_CTX_MUT(c);
    PF_CHECK(c->elbo_done, PFMI_ERR_STATE, "pool_build_best: call pfmi_elbo_batch[_enqueue] first");
    PF_CHECK(N_r >= 1, PFMI_ERR_ARG, "pool_build_best: bad arguments");
    PF_TRY(pool_alloc(c, N_r));
    PF_TRY(c->pool_ok.ensure(sizeof(int32_t) * c->K));
    if (fail_seeds) {
        PF_TRY(c->fail_seeds.ensure(sizeof(uint64_t) * c->K));
        PF_TRY(pf_upload(c, c->fail_seeds.p, fail_seeds, sizeof(uint64_t) * c->K));
    }
    PF_TRY(pf_launch_pool_pick(c, fail_seeds != nullptr));
    c->pool_from_best = true;
    return pool_fill(c);
}

int32_t pfmi_pool_winners(pfmi_ctx *c, int64_t *points, uint64_t *seeds, int32_t *success) {
    PF_CTX(c);
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_winners: call pfmi_pool_build[_best] first");
    std::vector<int32_t> pts((size_t)c->K);
    if (points) PF_TRY(pf_download(c, pts.data(), c->pool_points.p, sizeof(int32_t) * c->K));
    if (seeds) PF_TRY(pf_download(c, seeds, c->pool_seeds.p, sizeof(uint64_t) * c->K));
    if (success) {
        PF_CHECK(c->pool_from_best, PFMI_ERR_STATE, "pool_winners: success flags exist only after pfmi_pool_build_best");
        PF_TRY(pf_download(c, success, c->pool_ok.p, sizeof(int32_t) * c->K));
    }
    PF_TRY(pf_stream_sync(c));
    if (points)
        for (int k = 0; k < c->K; ++k) points[k] = pts[(size_t)k];
    return PFMI_OK;
}

int32_t pfmi_pool_get(pfmi_ctx *c, double *draws, double *log_ratios) {
    PF_CTX(c);
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_get: call pfmi_pool_build first");
    const size_t S = (size_t)c->K * c->N_r;
    if (draws) PF_TRY(d2h(c, draws, c->pool.p, sizeof(double) * S * c->d));
    if (log_ratios) PF_TRY(d2h(c, log_ratios, c->pool_lr.p, sizeof(double) * S));
    return PFMI_OK;
}

int32_t pfmi_pool_moments(pfmi_ctx *c, int64_t col_offset, int32_t importance, const double *center, double *wsum, double *s1,
                          double *s2, double *s2w) {
    PF_CTX_MUT(c);
    PF_TRY(pool_pass_check(c, "pool_moments", col_offset, importance));
    const size_t K = (size_t)c->K, d = (size_t)c->d;
    const double *d_center;
    PF_TRY(upload_optional(c, c->pool_center, center, d, &d_center));
    PF_TRY(pf_launch_pool_moments(c, col_offset, importance, d_center));
    const double *m = c->mom.as<double>();
    if (wsum) PF_TRY(pf_download(c, wsum, m, sizeof(double) * 2 * K));
    if (s1) PF_TRY(pf_download(c, s1, m + 2 * K, sizeof(double) * K * d));
    if (s2) PF_TRY(pf_download(c, s2, m + 2 * K + K * d, sizeof(double) * K * d));
    if (s2w) PF_TRY(pf_download(c, s2w, m + 2 * K + 2 * K * d, sizeof(double) * K * d));
    return pf_stream_sync(c);
}

int32_t pfmi_pool_cdf(pfmi_ctx *c, int64_t col_offset, int32_t importance, int32_t nthr, const double *thresholds, const double *wle_in,
                      double *wle, double *below, double *above, int32_t *nanflag) {
    PF_CTX_MUT(c);
    PF_TRY(pool_pass_check(c, "pool_cdf", col_offset, importance,
                           nthr >= 1 && nthr <= 32 && thresholds ? nullptr : "nthr must be in [1, 32] and thresholds non-NULL"));
    const size_t plane = (size_t)nthr * (size_t)c->d;
    const double *d_thr, *d_carry;
    PF_TRY(upload_optional(c, c->pcdf_thr, thresholds, plane, &d_thr));
    PF_TRY(upload_optional(c, c->pcdf_carry, wle_in, plane, &d_carry));
    PF_TRY(pf_launch_pool_cdf(c, col_offset, importance, nthr, d_thr, d_carry));
    const double *o = c->pcdf.as<double>();
    if (wle) PF_TRY(pf_download(c, wle, o, sizeof(double) * plane));
    if (below) PF_TRY(pf_download(c, below, o + plane, sizeof(double) * plane));
    if (above) PF_TRY(pf_download(c, above, o + 2 * plane, sizeof(double) * plane));
    if (nanflag) PF_TRY(pf_download(c, nanflag, o + 3 * plane, sizeof(int32_t) * (size_t)c->d));
    return pf_stream_sync(c);
}

int32_t pfmi_pool_cross(pfmi_ctx *c, int64_t col_offset, int32_t importance, const double *center, const double *c_in, double *c_out) {
    PF_CTX_MUT(c);
    PF_TRY(pool_pass_check(c, "pool_cross", col_offset, importance, col_offset >= 0 && c_out ? nullptr : "negative col_offset or NULL c_out"));
    const size_t d = (size_t)c->d;
    const double *d_center, *d_carry;
    PF_TRY(upload_optional(c, c->pool_center, center, d, &d_center));
    PF_TRY(upload_optional(c, c->cross, c_in, d * d, &d_carry));                   // accumulated in place
    PF_TRY(pf_launch_pool_cross(c, col_offset, importance, d_center, d_carry));
    PF_TRY(pf_download(c, c_out, c->cross.p, sizeof(double) * d * d));
    return pf_stream_sync(c);
}

int32_t pfmi_pool_apply(pfmi_ctx *c, int64_t col_offset, int32_t importance, const double *center, int32_t r, const double *v,
                        const double *y_in, double *y_out, double *scores) {
    PF_CTX_MUT(c);
    PF_TRY(pool_pass_check(c, "pool_apply", col_offset, importance,
                           r >= 1 && r <= PFMI_POOL_APPLY_MAX_R && v && y_out ? nullptr : "r must be in [1, 32] and v, y_out non-NULL"));
    const size_t plane = (size_t)r * (size_t)c->d;
    const double *d_center, *d_v, *d_carry;
    PF_TRY(upload_optional(c, c->pool_center, center, (size_t)c->d, &d_center));
    PF_TRY(upload_optional(c, c->apply_v, v, plane, &d_v));
    PF_TRY(upload_optional(c, c->apply_y, y_in, plane, &d_carry));                 // accumulated in place
    PF_TRY(pf_launch_pool_apply(c, col_offset, importance, d_center, r, d_v, d_carry));
    PF_TRY(pf_download(c, y_out, c->apply_y.p, sizeof(double) * plane));
    if (scores) PF_TRY(pf_download(c, scores, c->apply_z.p, sizeof(double) * (size_t)c->K * (size_t)c->N_r * (size_t)r));
    return pf_stream_sync(c);
}

int32_t pfmi_pool_draws_dev(pfmi_ctx *c, void **dev_ptr, int64_t *count) {
    PF_CTX(c);
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_draws_dev: call pfmi_pool_build first");
    PF_HIP(hipStreamSynchronize(c->stream));
    if (dev_ptr) *dev_ptr = c->pool.p;
    if (count) *count = (int64_t)c->d * c->K * c->N_r;
    return PFMI_OK;
}

int32_t pfmi_pool_log_ratios_dev(pfmi_ctx *c, void **dev_ptr, int64_t *count) {
    PF_CTX(c);
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_log_ratios_dev: call pfmi_pool_build first");
    PF_HIP(hipStreamSynchronize(c->stream));
    if (dev_ptr) *dev_ptr = c->pool_lr.p;
    if (count) *count = (int64_t)c->K * c->N_r;
    return PFMI_OK;
}

int32_t pfmi_pool_mixture_ratios(pfmi_ctx *c, double *log_mix, double *log_ratios) {
    PF_CTX_MUT(c);
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_mixture_ratios: call pfmi_pool_build first");
    PF_CHECK(c->tr_base == 0, PFMI_ERR_STATE,
             "pool_mixture_ratios: the pool is moved (pfmi_pool_transform): its mixture ratios follow from those of the pool as built");
    c->pool_mix_done = false;
    c->pool_lmix_ok = false;
    c->tr_undo = 0;                        // (a state to put back would not have these ratios)
    PF_TRY(pf_launch_pool_mixture_ratios(c));
    c->pool_mix_done = true;
    c->pool_lmix_ok = true;
    const size_t S = (size_t)c->K * c->N_r;
    if (log_mix) PF_TRY(pf_download(c, log_mix, c->pool_lmix.p, sizeof(double) * S));
    if (log_ratios) PF_TRY(pf_download(c, log_ratios, c->pool_lr_mix.p, sizeof(double) * S));
    return pf_stream_sync(c);
}

int32_t pfmi_pool_mixture_ratios_dev(pfmi_ctx *c, void **dev_ptr, int64_t *count) {
    PF_CTX(c);
    PF_CHECK(c->pooled && c->pool_mix_done, PFMI_ERR_STATE, "pool_mixture_ratios_dev: call pfmi_pool_mixture_ratios on the current pool first");
    PF_HIP(hipStreamSynchronize(c->stream));
    if (dev_ptr) *dev_ptr = c->pool_lr_mix.p;
    if (count) *count = (int64_t)c->K * c->N_r;
    return PFMI_OK;
}

int32_t pfmi_pool_psis_runs(pfmi_ctx *c, int32_t source, double *pareto_k, int64_t *tail_len, double *lse, double *sumsq, double *log_weights,
                            double *weights) {
    PF_CTX_MUT(c);
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_psis_runs: call pfmi_pool_build first");
    PF_CHECK(source == PFMI_RATIOS_COMPONENT || source == PFMI_RATIOS_MIXTURE, PFMI_ERR_ARG, "pool_psis_runs: unknown source %d", (int)source);
    PF_CHECK(source != PFMI_RATIOS_MIXTURE || c->pool_mix_done, PFMI_ERR_STATE,
             "pool_psis_runs: call pfmi_pool_mixture_ratios on the current pool first");
    const int K = c->K;
    const size_t S = (size_t)K * (size_t)c->N_r;
    PF_TRY(pf_launch_psis_runs(c, source == PFMI_RATIOS_MIXTURE ? c->pool_lr_mix.as<double>() : c->pool_lr.as<double>(), K, c->N_r));
    std::vector<double> out((size_t)K * PF_PSIS_RUN_OUT);
    PF_TRY(pf_download(c, out.data(), c->runs_out.p, sizeof(double) * out.size()));
    if (log_weights) PF_TRY(pf_download(c, log_weights, c->runs_lw.p, sizeof(double) * S));
    if (weights) PF_TRY(pf_download(c, weights, c->runs_w.p, sizeof(double) * S));
    PF_TRY(pf_stream_sync(c));
    for (int k = 0; k < K; ++k) {
        const double *o = out.data() + (size_t)k * PF_PSIS_RUN_OUT;
        if (pareto_k) pareto_k[k] = o[0];
        if (tail_len) tail_len[k] = (int64_t)o[1];
        if (lse) lse[k] = o[3];
        if (sumsq) sumsq[k] = o[4];
    }
    return PFMI_OK;
}

int32_t pfmi_psis_dev(pfmi_ctx *c, const void *lr_dev, int64_t S, double *weights, double *log_weights,
                      double *pareto_k, int64_t *tail_len) {
    PF_CTX_MUT(c);
    PF_CHECK(lr_dev != nullptr && S > 0, PFMI_ERR_ARG, "psis: bad arguments");
    PF_TRY(pf_launch_psis(c, reinterpret_cast<const double *>(lr_dev), S));
    double out[4];
    PF_TRY(d2h(c, out, c->psis_out.p, sizeof(out)));
    if (pareto_k) *pareto_k = out[0];
    if (tail_len) *tail_len = (int64_t)out[1];
    if (weights) PF_TRY(d2h(c, weights, c->w.p, sizeof(double) * S));
    if (log_weights) PF_TRY(d2h(c, log_weights, c->lw.p, sizeof(double) * S));
    return PFMI_OK;
}

int32_t pfmi_psis_weights(pfmi_ctx *c, int64_t S, double *weights, double *log_weights) {
    PF_CTX(c);
    PF_CHECK(S > 0 && c->S_w == S, PFMI_ERR_STATE, "psis_weights: no PSIS result for S=%lld on this ctx", (long long)S);
    if (weights) PF_TRY(pf_download(c, weights, c->w.p, sizeof(double) * S));
    if (log_weights) PF_TRY(pf_download(c, log_weights, c->lw.p, sizeof(double) * S));
    if (c->defer) return PFMI_OK;
    return pf_stream_sync(c);
}

int32_t pfmi_psis(pfmi_ctx *c, const double *lr, int64_t S, double *weights, double *log_weights, double *pareto_k,
                  int64_t *tail_len) {
    PF_CTX_MUT(c);
    PF_CHECK(lr != nullptr && S > 0, PFMI_ERR_ARG, "psis: bad arguments");
    PF_TRY(c->gbuf.ensure(sizeof(double) * S));
    PF_TRY(pf_upload(c, c->gbuf.p, lr, sizeof(double) * S));
    return pfmi_psis_dev(c, c->gbuf.p, S, weights, log_weights, pareto_k, tail_len);
}

int32_t pfmi_resample_indices(pfmi_ctx *c, int64_t S, int64_t ndraws, int32_t importance, int32_t replace,
                              uint64_t seed, const double *uniforms, int64_t *idx) {
    PF_CTX_MUT(c);
    PF_CHECK(S > 0 && ndraws >= 0, PFMI_ERR_ARG, "resample: bad arguments");
    PF_CHECK(!importance || c->S_w == S, PFMI_ERR_STATE,
             "resample: importance weights for S=%lld not available (run pfmi_psis first)", (long long)S);
    const double *d_uni = nullptr;
    if (uniforms && ndraws > 0) {
        PF_TRY(c->tailbuf.ensure(sizeof(double) * ndraws));
        PF_TRY(pf_upload(c, c->tailbuf.p, uniforms, sizeof(double) * ndraws));
        d_uni = c->tailbuf.as<double>();
    }
    PF_TRY(pf_launch_resample(c, S, ndraws, importance, replace, seed, d_uni));
    if (idx && ndraws > 0) PF_TRY(d2h(c, idx, c->idx.p, sizeof(int64_t) * ndraws));
    return PFMI_OK;
}

int32_t pfmi_resample_indices_direct(pfmi_ctx *c, int64_t S, int64_t ndraws, const double *uniforms, int64_t *idx) {
    PF_CTX_MUT(c);
    PF_CHECK(S > 0 && ndraws >= 0 && (uniforms != nullptr || ndraws == 0), PFMI_ERR_ARG, "resample_direct: bad arguments");
    PF_CHECK(c->S_w == S, PFMI_ERR_STATE, "resample_direct: importance weights for S=%lld not available (run pfmi_psis first)",
             (long long)S);
    if (ndraws == 0) return PFMI_OK;
    for (int64_t t = 0; t < ndraws; ++t)
        PF_CHECK(uniforms[t] >= 0.0 && uniforms[t] < 1.0, PFMI_ERR_ARG, "resample_direct: uniforms[%lld] = %g is not in [0, 1)", (long long)t,
                 uniforms[t]);
    PF_TRY(c->tailbuf.ensure(sizeof(double) * ndraws));
    PF_TRY(pf_upload(c, c->tailbuf.p, uniforms, sizeof(double) * ndraws));
    PF_TRY(pf_launch_resample_direct(c, S, ndraws, c->tailbuf.as<double>()));
    if (idx) PF_TRY(d2h(c, idx, c->idx.p, sizeof(int64_t) * ndraws));
    return PFMI_OK;
}

int32_t pfmi_pool_gather_dev(pfmi_ctx *c, int64_t ndraws, const int64_t *idx, int64_t col_offset, void *draws_dev) {
    PF_CTX(c);
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_gather: call pfmi_pool_build first");
    PF_CHECK(ndraws >= 0 && idx && draws_dev, PFMI_ERR_ARG, "pool_gather: bad arguments");
    PF_TRY(c->idx.ensure(sizeof(int64_t) * (ndraws > 0 ? ndraws : 1)));
    PF_TRY(pf_upload(c, c->idx.p, idx, sizeof(int64_t) * ndraws));
    PF_TRY(pf_launch_gather(c, ndraws, c->idx.as<int64_t>(), col_offset, reinterpret_cast<double *>(draws_dev)));
    PF_HIP(hipStreamSynchronize(c->stream));
    return PFMI_OK;
}

int32_t pfmi_pool_gather(pfmi_ctx *c, int64_t ndraws, const int64_t *idx, int64_t col_offset, double *draws) {
    PF_CTX(c);
    PF_CHECK(draws != nullptr, PFMI_ERR_ARG, "pool_gather: null output");
    PF_CHECK(c->pooled, PFMI_ERR_STATE, "pool_gather: call pfmi_pool_build first");
    PF_CHECK(ndraws >= 0 && (idx != nullptr || ndraws == 0), PFMI_ERR_ARG, "pool_gather: bad arguments");
    const int64_t owned = (int64_t)c->K * c->N_r;
    for (int64_t t = 0; t < ndraws; ++t)   // the host variant hands back real columns only: no silent zero fill
        PF_CHECK(idx[t] >= col_offset && idx[t] < col_offset + owned, PFMI_ERR_ARG,
                 "pool_gather: index %lld (position %lld) is outside this pool's columns [%lld, %lld)", (long long)idx[t],
                 (long long)t, (long long)col_offset, (long long)(col_offset + owned));
    PF_TRY(c->gbuf.ensure(sizeof(double) * (size_t)(ndraws > 0 ? ndraws : 1) * c->d));
    PF_TRY(pfmi_pool_gather_dev(c, ndraws, idx, col_offset, c->gbuf.p));
    PF_TRY(d2h(c, draws, c->gbuf.p, sizeof(double) * (size_t)ndraws * c->d));
    return PFMI_OK;
}

}  // extern "C"
