// lbfgs_closure_kernel.hip -- batched L-BFGS for DEVICE_CALLBACK targets that carry a value-and-gradient closure
// (pfmi_set_target_gradient).
//
// The same iteration as pf_lbfgs_kernel (lbfgs_kernels.hip), the CPU oracle's driver and pfmi/optimize.py -- gamma = s'y / y'y,
// restart on a non-descent direction, strong Wolfe (c1 = 1e-4, c2 = 0.9, doubling up to 1e10, 25 bracketing + 30 bisection-zoom
// evaluations, halving on a non-finite value), curvature test y's > 1e-10 y'y, ring of the last J pairs, the same stop rules -- but the
// function is the user's: it cannot be called from inside a kernel.  So the optimisation is cut into ROUNDS.  One round = one launch of
// pf_lbc_step_kernel (one workgroup per path) followed by one call of the user's closure on all K columns of X:
//   * the step kernel reads its path's column of the closure's output (logp, grad logp at the trial point it wrote in the previous round),
//     advances the line-search state machine of lb_search by exactly one evaluation, and -- when the search accepts -- records the trace
//     row, updates the (s, y) ring and the Gram data and forms the next direction;
//   * it then writes the path's next trial point x + a p into column k of X.  Finished paths write nothing.
// Everything a path carries between rounds lives in HBM: x, g, p [d]; the ring S, Y [J][d]; the Gram data of the compact form; the scalar
// state LcPath (the locals of lb_search plus the iteration counters).
//
// The direction is the compact form of Byrd, Nocedal & Schnabel (1994), as in pf_lbfgs_kernel: H g = gamma g + S a - gamma Y t with
// t = R^-1 S'g and a = R^-T ((D + gamma Y'Y) t - gamma Y'g).  The inner products it needs (the new column of R and Y'Y, S'g, Y'g) come
// out of the fused reduction of the acceptance, CH ring pairs per block reduction; the (h x h) triangular solves run on the lanes of
// wave 0 out of an LDS copy of the Gram data.  A search round costs one block reduction (g(x + a p)'p), an acceptance round
// 1 + ceil(h / CH).
//
// Every control-flow scalar comes out of a fixed-order block reduction (wave butterflies, then the waves' partials summed in wave order
// by every thread), so all threads of a path take the same branch and a path's trace depends on nothing but its own x0: not on K, not on
// the other paths, not on the run.
//
// Progress: every path that is still running after a round adds one to a device counter; the last workgroup of the round (a ticket)
// publishes (round << 32 | active paths) to page-locked host memory and resets the counters.  The host (pfmi_optimize_batch_pump) keeps
// at most a few rounds in flight and stops once it reads zero.
//
// Streaming (pfmi_stream_enqueue): h_prog != null.  A round that records a trace row, or ends the path, publishes the path's point count
// to h_prog[k] and -- behind the final count -- its done flag to h_prog[K + k], the page-locked words pfmi_stream_pump reads for the
// built-in optimiser too (same recipe as pf_lbfgs_kernel: every thread fences its row stores at agent scope, a barrier, then thread 0's
// system-scope release).  The staging trace [K][maxiters + 1][d] is already the fixed-stride layout of the stream: nothing is packed.
// h_prog == null (the packed route): nothing is published, the bits are today's.
#include "pfmi_common.h"

#define LC_NT 256                      // threads per path (4 waves)
#define LC_NW (LC_NT / 64)
#define LC_JMAX 32                     // history_length limit (the fit path's own)
#define LC_CH 4                        // ring pairs per block reduction of the acceptance
#define LC_NV (4 * LC_CH + 8)          // values of one such reduction

enum { LC_EVAL_X0 = 0, LC_SEARCH = 1, LC_DONE = 2 };

struct LcPath {                        // per-path scalar state (HBM); read by every thread, written back by thread 0
    double f, gg, nbig, nbad, gam;     // current point: -logp, g'g, #{|g_i| > g_tol}, #non-finite g_i; H0 scaling
    double a, a_prev, f_prev, lo, hi, f_lo, f0, g0;      // lb_search's locals
    int32_t phase, h, head, n, it, lsit, zit, zoom;
};

struct LcArgs {
    int d, J, K, maxiters, reject_every;
    double g_tol;
    int64_t cap;                       // maxiters + 1 trace rows per path
    int64_t round;
    const double *x0;                  // [K][d]
    double *X;                         // closure input: d x K column-major
    const double *out;                 // closure output: logp [K], then grad [K][d]
    double *x, *g, *p;                 // [K][d]; g = grad f = -grad logp at x
    double *hs, *hy;                   // ring [K][J][d]
    double *gram;                      // [K][2 J J + 3 J]: SY (slot-indexed, row = older pair), YY, U = S'g, W = Y'g, RI = 1 / s'y
    LcPath *st;                        // [K]
    double *tr_theta, *tr_grad, *tr_lp;      // staging trace [K][cap][d], [K][cap] (pf_trace_pack_kernel's input)
    int32_t *npts;                     // [K]
    int32_t *ctr;                      // [2]: paths still active after this round, workgroups finished
    int64_t *h_status;                 // page-locked host word: round << 32 | active
    int32_t *h_prog;                   // streaming: page-locked [2 K] (counts, then done flags); null: no publication
};

// Block-wide sums of NV values per thread; every thread returns the same totals.  Ping-pong buffers: a buffer is only rewritten two
// reductions later, after a barrier every thread reaches once it has read this one.
template <int NV>
__device__ __forceinline__ void lc_block_sum(double (&v)[NV], double *red, int &flip) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *buf = red + flip * (LC_NW * LC_NV);
    flip ^= 1;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        double s = v[j];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        v[j] = s;
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) buf[wave * NV + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        double s = buf[j];
#pragma unroll
        for (int w = 1; w < LC_NW; ++w) s += buf[w * NV + j];
        v[j] = s;
    }
}

__global__ __launch_bounds__(LC_NT) void pf_lbc_init_kernel(LcArgs A) {
    const int k = blockIdx.x, d = A.d;
    const double *x0 = A.x0 + (size_t)k * d;
    double *X = A.X + (size_t)k * d, *x = A.x + (size_t)k * d;
    for (int i = threadIdx.x; i < d; i += LC_NT) { const double v = x0[i]; X[i] = v; x[i] = v; }
    if (threadIdx.x == 0) {
        LcPath S = {};
        S.phase = LC_EVAL_X0; S.gam = 1.0;
        A.st[k] = S;
        A.npts[k] = 0;
        if (k == 0) { A.ctr[0] = 0; A.ctr[1] = 0; }
    }
}

__global__ __launch_bounds__(LC_NT) void pf_lbc_step_kernel(LcArgs A) {
    __shared__ double red[2 * LC_NW * LC_NV];
    __shared__ double sSY[LC_JMAX * LC_JMAX], sYY[LC_JMAX * LC_JMAX], sU[LC_JMAX], sW[LC_JMAX], sRI[LC_JMAX], cS[LC_JMAX], cY[LC_JMAX];
    __shared__ double sG0;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = A.d, J = A.J, K = A.K;
    int flip = 0;
    LcPath S = A.st[k];
    if (S.phase != LC_DONE) {
        const int n_in = S.n;
        const size_t kd = (size_t)k * d;
        double *X = A.X + kd, *x = A.x + kd, *g = A.g + kd, *p = A.p + kd;
        const double *gout = A.out + K + kd;
        const double fn = -A.out[k];
        double *tr_theta = A.tr_theta + (size_t)k * A.cap * d, *tr_grad = A.tr_grad + (size_t)k * A.cap * d, *tr_lp = A.tr_lp + (size_t)k * A.cap;
        const int gstride = 2 * J * J + 3 * J;
        double *gram = A.gram + (size_t)k * gstride;
        double *hs = A.hs + (size_t)k * J * d, *hy = A.hy + (size_t)k * J * d;
        auto slot = [&](int age) { return S.head + age - (S.head + age >= J ? J : 0); };
        // trace row n: the current point x (in `src`), grad logp = -g, logp = -f
        auto record = [&](const double *src, const double *gsrc, double f) {
            double *th = tr_theta + (size_t)S.n * d, *gr = tr_grad + (size_t)S.n * d;
            for (int i = tid; i < d; i += LC_NT) { th[i] = src[i]; gr[i] = -gsrc[i]; }
            if (tid == 0) { tr_lp[S.n] = -f; A.npts[k] = S.n + 1; }
            ++S.n;
        };
        bool start = false;             // begin the next iteration in this round
        if (S.phase == LC_EVAL_X0) {
            double v[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = tid; i < d; i += LC_NT) {
                const double gi = -gout[i];
                g[i] = gi;
                v[0] += gi * gi;
                v[1] += (fabs(gi) > A.g_tol) ? 1.0 : 0.0;
                v[2] += isfinite(gi) ? 0.0 : 1.0;
            }
            lc_block_sum<4>(v, red, flip);
            S.gg = v[0]; S.nbig = v[1]; S.nbad = v[2];
            S.f = fn;
            record(x, g, fn);
            start = true;
        } else {
            // ---- one step of lb_search (lbfgs_kernels.hip) on the value just evaluated at a = S.a
            double v[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = tid; i < d; i += LC_NT) v[0] += -gout[i] * p[i];
            lc_block_sum<4>(v, red, flip);
            const double f = fn, gd = v[0], c1 = 1e-4, c2 = 0.9, amax = 1e10, f0 = S.f0, g0 = S.g0;
            bool accept = false, bisect = true;
            if (!S.zoom) {
                const int it0 = S.lsit++;
                bisect = false;
                if (!isfinite(f)) { S.a = 0.5 * (S.a_prev + S.a); accept = S.lsit >= 25; }
                else if ((f > f0 + c1 * S.a * g0) || (it0 > 0 && f >= S.f_prev)) { S.zoom = 1; S.lo = S.a_prev; S.hi = S.a; S.f_lo = S.f_prev; bisect = true; }
                else if (fabs(gd) <= -c2 * g0) accept = true;
                else if (gd >= 0) { S.zoom = 1; S.lo = S.a; S.hi = S.a_prev; S.f_lo = f; bisect = true; }
                else { S.a_prev = S.a; S.f_prev = f; S.a = fmin(2 * S.a, amax); accept = S.lsit >= 25; }
            } else {
                if ((f > f0 + c1 * S.a * g0) || (f >= S.f_lo)) {
                    S.hi = S.a;
                } else if (fabs(gd) <= -c2 * g0) {
                    accept = true;
                } else {
                    if (gd * (S.hi - S.lo) >= 0) S.hi = S.lo;
                    S.lo = S.a; S.f_lo = f;
                }
                if (!accept && ++S.zit >= 30) accept = true;
            }
            if (!accept) {
                if (bisect) S.a = 0.5 * (S.lo + S.hi);
                for (int i = tid; i < d; i += LC_NT) X[i] = fma(S.a, p[i], x[i]);
            } else {
                // ---- accept the last evaluated point xn = X (what the closure saw), gn = -grad logp there.  The fused reduction of
                //      chunk 0 carries s'y, y'y, #moved, #non-finite gn, gn'gn, #{|gn_i| > g_tol}, s'gn, y'gn behind the ring values.
                for (int t = tid; t < 2 * J * J + 3 * J; t += LC_NT) {
                    const double v_ = gram[t];
                    if (t < J * J) sSY[t] = v_;
                    else if (t < 2 * J * J) sYY[t - J * J] = v_;
                    else if (t < 2 * J * J + J) sU[t - 2 * J * J] = v_;
                    else if (t < 2 * J * J + 2 * J) sW[t - 2 * J * J - J] = v_;
                    else sRI[t - 2 * J * J - 2 * J] = v_;
                }
                const int h = S.h;
                const int slot_new = (h == J) ? S.head : slot(h);              // h == J: the oldest pair is replaced
                const int nch = h > 0 ? (h + LC_CH - 1) / LC_CH : 1;
                double sy = 0.0, yy = 0.0, moved = 0.0, sgn = 0.0, ygn = 0.0;
                bool take = false, stop = false;
                for (int ch = 0; ch < nch; ++ch) {
                    double w[LC_NV];
#pragma unroll
                    for (int j = 0; j < LC_NV; ++j) w[j] = 0.0;
                    for (int i = tid; i < d; i += LC_NT) {
                        const double gni = -gout[i], yi = gni - g[i];
#pragma unroll
                        for (int cc = 0; cc < LC_CH; ++cc) {
                            const int age = ch * LC_CH + cc;
                            if (age < h) {
                                const int sl = slot(age);
                                const double sv = hs[(size_t)sl * d + i], yv = hy[(size_t)sl * d + i];
                                w[4 * cc + 0] += sv * yi;
                                w[4 * cc + 1] += yv * yi;
                                w[4 * cc + 2] += sv * gni;
                                w[4 * cc + 3] += yv * gni;
                            }
                        }
                        if (ch == 0) {
                            const double xi = x[i], xni = X[i], si = xni - xi;
                            w[4 * LC_CH + 0] += yi * si;
                            w[4 * LC_CH + 1] += yi * yi;
                            w[4 * LC_CH + 2] += (xni != xi) ? 1.0 : 0.0;
                            w[4 * LC_CH + 3] += isfinite(gni) ? 0.0 : 1.0;
                            w[4 * LC_CH + 4] += gni * gni;
                            w[4 * LC_CH + 5] += (fabs(gni) > A.g_tol) ? 1.0 : 0.0;
                            w[4 * LC_CH + 6] += si * gni;
                            w[4 * LC_CH + 7] += yi * gni;
                        }
                    }
                    lc_block_sum<LC_NV>(w, red, flip);
                    if (ch == 0) {
                        sy = w[4 * LC_CH + 0]; yy = w[4 * LC_CH + 1]; moved = w[4 * LC_CH + 2]; S.nbad = w[4 * LC_CH + 3];
                        S.gg = w[4 * LC_CH + 4]; S.nbig = w[4 * LC_CH + 5]; sgn = w[4 * LC_CH + 6]; ygn = w[4 * LC_CH + 7];
                        if (!isfinite(fn) || S.nbad > 0.0) { stop = true; break; }
                        take = sy > 1e-10 * yy && !(A.reject_every > 0 && (S.it + 1) % A.reject_every == 0);
                    }
                    if (tid == 0) {                                              // file the totals in the Gram data (LDS copy)
#pragma unroll
                        for (int cc = 0; cc < LC_CH; ++cc) {
                            const int age = ch * LC_CH + cc;
                            if (age >= h) continue;
                            const int sl = slot(age);
                            if (take && sl == slot_new) continue;                // the pair being replaced
                            sU[sl] = w[4 * cc + 2]; sW[sl] = w[4 * cc + 3];
                            if (take) { sSY[sl * J + slot_new] = w[4 * cc + 0]; sYY[sl * J + slot_new] = w[4 * cc + 1]; sYY[slot_new * J + sl] = w[4 * cc + 1]; }
                        }
                    }
                }
                if (stop) {                      // src/optimize.jl:96-105: the offending iterate is recorded, then the run stops
                    for (int i = tid; i < d; i += LC_NT) g[i] = -gout[i];
                    record(X, g, fn);
                    S.phase = LC_DONE;
                } else {
                    if (take) {
                        if (tid == 0) {
                            sSY[slot_new * J + slot_new] = sy; sRI[slot_new] = 1.0 / sy; sYY[slot_new * J + slot_new] = yy;
                            sU[slot_new] = sgn; sW[slot_new] = ygn;
                        }
                        for (int i = tid; i < d; i += LC_NT) {
                            const double gni = -gout[i];
                            hs[(size_t)slot_new * d + i] = X[i] - x[i];
                            hy[(size_t)slot_new * d + i] = gni - g[i];
                        }
                        if (h == J) S.head = S.head + 1 == J ? 0 : S.head + 1; else ++S.h;
                        S.gam = sy / yy;
                    }
                    for (int i = tid; i < d; i += LC_NT) { x[i] = X[i]; g[i] = -gout[i]; }
                    S.f = fn;
                    record(x, g, fn);
                    ++S.it;
                    if (!(moved > 0.0)) S.phase = LC_DONE;
                    else start = true;
                }
                __syncthreads();                                                 // the Gram data back to HBM
                for (int t = tid; t < 2 * J * J + 3 * J; t += LC_NT) {
                    double v_;
                    if (t < J * J) v_ = sSY[t];
                    else if (t < 2 * J * J) v_ = sYY[t - J * J];
                    else if (t < 2 * J * J + J) v_ = sU[t - 2 * J * J];
                    else if (t < 2 * J * J + 2 * J) v_ = sW[t - 2 * J * J - J];
                    else v_ = sRI[t - 2 * J * J - 2 * J];
                    gram[t] = v_;
                }
            }
        }
        if (start) {
            // ---- the next iteration: stop rules, direction, first trial point
            if (S.it >= A.maxiters || !isfinite(S.f) || S.nbad > 0.0 || S.nbig == 0.0) {
                S.phase = LC_DONE;
            } else {
                const int h = S.h;
                double g0 = 0.0;
                if (h > 0) {
                    // the two h x h triangular solves on the lanes of wave 0 (lane i = the pair of age i, 0 = oldest), as pf_lbfgs_kernel
                    if (wave == 0) {
                        const int li = lane < h ? lane : 0, sl = slot(li);
                        double u = sU[sl];
                        const double w = sW[sl], ri = sRI[sl], u0 = u, dd = sSY[sl * J + sl], gam = S.gam;
                        double t = 0.0, acc = 0.0;
                        for (int j = h - 1; j >= 0; --j) {
                            const int sj = slot(j);
                            const double tj = __shfl(u, j, 64) * __shfl(ri, j, 64);
                            if (lane == j) t = tj;
                            if (lane < j) u -= sSY[sl * J + sj] * tj;
                            acc += sYY[sl * J + sj] * tj;
                        }
                        double z = dd * t + gam * (acc - w), ca = 0.0;
                        for (int j = 0; j < h; ++j) {
                            const int sj = slot(j);
                            const double aj = __shfl(z, j, 64) * __shfl(ri, j, 64);
                            if (lane == j) ca = aj;
                            if (lane > j) z -= sSY[sj * J + sl] * aj;
                        }
                        const double s1 = (lane < h) ? u0 * ca - gam * (w * t) : 0.0;
                        double tot = 0.0;
                        for (int i = 0; i < h; ++i) tot += __shfl(s1, i, 64);
                        if (lane < h) { cS[lane] = ca; cY[lane] = -gam * t; }
                        if (lane == 0) sG0 = -(gam * S.gg + tot);              // g'p
                    }
                    __syncthreads();
                    g0 = sG0;
                }
                const bool restart = h == 0 || !(g0 < 0);
                if (restart) { S.h = 0; S.head = 0; g0 = -S.gg; }
                const double a0 = restart ? fmin(1.0, 1.0 / fmax(sqrt(S.gg), 1e-300)) : 1.0;
                for (int i = tid; i < d; i += LC_NT) {
                    double pi;
                    if (restart) {
                        pi = -g[i];
                    } else {
                        double q = S.gam * g[i];
                        for (int c = 0; c < h; ++c) {
                            const int sl = slot(c);
                            q += cS[c] * hs[(size_t)sl * d + i] + cY[c] * hy[(size_t)sl * d + i];
                        }
                        pi = -q;
                    }
                    p[i] = pi;
                    X[i] = fma(a0, pi, x[i]);
                }
                S.a = a0; S.a_prev = 0.0; S.f_prev = S.f; S.f0 = S.f; S.g0 = g0; S.lo = 0.0; S.hi = 0.0; S.f_lo = 0.0;
                S.lsit = 0; S.zit = 0; S.zoom = 0;
                S.phase = LC_SEARCH;
            }
        }
        // streaming: rows 0 .. S.n - 1 reach memory (every thread's stores, agent scope) before thread 0 publishes the count; the flag
        // goes behind the final count.  (S is the same in every thread: the condition is uniform.)
        const bool pub = A.h_prog && (S.n != n_in || S.phase == LC_DONE);
        if (pub) __threadfence();
        __syncthreads();                    // every thread has read S and the LDS state before thread 0 writes
        if (tid == 0) {
            A.st[k] = S;
            if (pub) {
                __hip_atomic_store(A.h_prog + k, S.n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                if (S.phase == LC_DONE) __hip_atomic_store(A.h_prog + K + k, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    // ---- progress of the round: the last workgroup publishes the number of paths still running
    if (tid == 0) {
        if (S.phase != LC_DONE) __hip_atomic_fetch_add(A.ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const int ticket = __hip_atomic_fetch_add(A.ctr + 1, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == K - 1) {
            const int active = __hip_atomic_load(A.ctr, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            A.ctr[0] = 0; A.ctr[1] = 0;
            __hip_atomic_store(A.h_status, (int64_t)((A.round << 32) | (int64_t)active), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
static LcArgs lc_args(pfmi_ctx *c, int64_t round) {
    const LbcState &O = c->lbc;
    LcArgs A;
    A.d = c->target.d; A.J = O.J; A.K = O.K; A.maxiters = O.maxiters; A.reject_every = O.reject_every; A.g_tol = O.g_tol;
    A.cap = (int64_t)O.maxiters + 1; A.round = round;
    A.x0 = c->lb_x0.as<double>(); A.X = c->lc_X.as<double>(); A.out = c->lc_out.as<double>();
    A.x = c->lc_x.as<double>(); A.g = c->lc_g.as<double>(); A.p = c->lc_p.as<double>();
    A.hs = c->lb_hs.as<double>(); A.hy = c->lb_hy.as<double>(); A.gram = c->lc_gram.as<double>();
    A.st = c->lc_st.as<LcPath>();
    A.tr_theta = c->st_theta.as<double>(); A.tr_grad = c->st_grad.as<double>(); A.tr_lp = c->st_lp.as<double>();
    A.npts = c->st_npts.as<int32_t>(); A.ctr = c->lc_ctr.as<int32_t>(); A.h_status = c->lc_status; A.h_prog = O.h_prog;
    return A;
}

size_t pf_lbc_path_state_bytes(int J) { return sizeof(LcPath) + sizeof(double) * (size_t)(2 * J * J + 3 * J); }

int32_t pf_lbc_alloc(pfmi_ctx *c, int K, int J, int d) {
    const size_t vec = sizeof(double) * (size_t)K * d;
    PF_TRY(c->lc_X.ensure(vec));
    PF_TRY(c->lc_out.ensure(sizeof(double) * (size_t)K * (d + 1)));
    PF_TRY(c->lc_x.ensure(vec));
    PF_TRY(c->lc_g.ensure(vec));
    PF_TRY(c->lc_p.ensure(vec));
    PF_TRY(c->lb_hs.ensure(vec * J));
    PF_TRY(c->lb_hy.ensure(vec * J));
    PF_TRY(c->lc_gram.ensure(sizeof(double) * (size_t)K * (2 * J * J + 3 * J)));
    PF_TRY(c->lc_st.ensure(sizeof(LcPath) * (size_t)K));
    PF_TRY(c->lc_ctr.ensure(sizeof(int32_t) * 2));
    if (!c->lc_status) PF_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->lc_status), sizeof(int64_t), hipHostMallocCoherent | hipHostMallocMapped));
    return PFMI_OK;
}

int32_t pf_launch_lbc_init(pfmi_ctx *c, hipStream_t s) {
    hipLaunchKernelGGL(pf_lbc_init_kernel, dim3(c->lbc.K), dim3(LC_NT), 0, s, lc_args(c, 0));
    PF_HIP(hipGetLastError());
    return PFMI_OK;
}

int32_t pf_launch_lbc_step(pfmi_ctx *c, int64_t round, hipStream_t s) {
    hipLaunchKernelGGL(pf_lbc_step_kernel, dim3(c->lbc.K), dim3(LC_NT), 0, s, lc_args(c, round));
    PF_HIP(hipGetLastError());
    return PFMI_OK;
}
