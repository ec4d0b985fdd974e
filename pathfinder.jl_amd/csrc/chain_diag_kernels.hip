// chain_diag_kernels.hip -- rank-normalised split R-hat, bulk / tail ESS, mean, sd and MCSE of MCMC chains (pfmi_chain_diagnostics).
//
// Definitions: include/pfmi.h (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021).  Input: records [K][T][d], d innermost (the layout of
// pfmi_hmc_get's draws), optionally one more series [K][T] (logp) as coordinate d.  V = d (+ 1) coordinates, R = K T rows, n = T / 2,
// M = 2 K split chains, S' = M n values survive the split.
//
// Layout.  One transpose into xs [V][R]: from there on a coordinate's series, and inside it every split chain (chain k's first and last n
// draws), is contiguous and every load is coalesced.  z(x) and z(fold(x)) are materialised as [V][S']; the two indicator series are
// formed from xs and their threshold on the fly.
//
// Ranks.  Fractional ranks with average ties by COUNTING, for any S': rank_i = (#{x_j < x_i} + #{x_j <= x_i} + 1) / 2.  The S' values are
// cut into tiles of CD_TILE; pf_cd_tilesort_kernel sorts every tile once in LDS (bitonic) and pf_cd_rank_kernel stages the sorted tiles
// through LDS one after the other, each thread finding the two counts of its CD_IPT values in a tile by two binary searches:
// O(S' (S' / CD_TILE) log CD_TILE) per coordinate and transform, one route for every size.  The counts also name the order statistics the
// type-7 median and quantiles need (value i is order statistic j iff #less <= j < #less-or-equal).  Cost: profiles/chain_diagnostics.md.
//
// Autocovariances.  One workgroup per (coordinate, series); lags in ascending batches of CD_LAGS, the workgroup stops at the batch
// that holds Geyer's truncation point J, so a chain that mixes in a few lags costs O(n J).  Every sum is a per-lane strided sum, a
// fixed-order wave sum and the waves in wave order (pf_block_sum): no atomics, the same bits on every call.
#include "pfmi_common.h"

#include <math.h>

#define CD_THREADS 256
#define CD_TILE 2048          // doubles of one counting tile in LDS (16 KB)
#define CD_IPT 4              // values of its own per thread of the counting kernel
#define CD_LAGS 8             // lags per batch of the autocovariance kernel (four Geyer pairs)
#define CD_NSERIES 5          // x, z(x), z(fold(x)), [x <= q05], [x <= q95]
#define CD_NOUT 7             // mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, rhat

struct CdShape {
    int d, V, K, M;
    int64_t T, n, R, Sp;
    int64_t os[6];            // order statistics wanted: the two of the median, the two of q05, the two of q95 (0-based)
    double t05, t95;          // numpy's interpolation weights of the two quantiles
};

// ---- [R][d] (+ lp [R]) -> xs [V][R] --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pf_cd_transpose_kernel(int d, int64_t R, const double *__restrict__ src, double *__restrict__ xs) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    for (int j = ty; j < 32; j += 8) {
        const int64_t r = r0 + j;
        const int cc = c0 + tx;
        if (r < R && cc < d) tile[j][tx] = src[(size_t)r * d + cc];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int cc = c0 + j;
        const int64_t r = r0 + tx;
        if (cc < d && r < R) xs[(size_t)cc * R + r] = tile[tx][j];
    }
}

// ---- mean and sd (ddof = 1) over all R draws; flag[v] = 1 when a draw is not finite ---------------------------------------------------
__global__ __launch_bounds__(CD_THREADS) void pf_cd_moments_kernel(int64_t R, const double *__restrict__ xs, double *__restrict__ mom,
                                                                  int32_t *__restrict__ flag) {
    __shared__ double red[3 * (CD_THREADS / 64)];
    const int v = blockIdx.x, tid = threadIdx.x;
    const double *x = xs + (size_t)v * R;
    const double x0 = x[0];
    double a[3] = {0.0, 0.0, 0.0};
    for (int64_t i = tid; i < R; i += CD_THREADS) {
        const double t = x[i];
        a[0] += t;
        a[1] += isfinite(t) ? 0.0 : 1.0;
        a[2] += t != x0 ? 1.0 : 0.0;
    }
    pf_block_sum<3>(a, red);
    const bool bad = a[1] != 0.0;
    const double mean = a[2] == 0.0 ? x0 : a[0] / (double)R;      // all draws equal: that value, exactly (sd = 0)
    double s[1] = {0.0};
    if (!bad)
        for (int64_t i = tid; i < R; i += CD_THREADS) {
            const double t = x[i] - mean;
            s[0] += t * t;
        }
    pf_block_sum<1>(s, red);
    if (tid == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        mom[2 * (size_t)v] = bad ? nan : mean;
        mom[2 * (size_t)v + 1] = bad ? nan : sqrt(s[0] / (double)(R - 1));
        flag[v] = bad ? 1 : 0;
    }
}

// ---- Wichura (1988), Algorithm AS 241, PPND16: the normal quantile to about 1 part in 10^16 --------------------------------------------
__device__ __forceinline__ double cd_ppnd16(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                              1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = ((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                               2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                            4.2313330701600911252e+1) * r + 1.0;
        return num / den;
    }
    double r = q < 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    double val;
    if (r <= 5.0) {
        r -= 1.6;
        const double num = ((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                               1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                            4.63033784615654529590e+0) * r + 1.42343711074968357734e+0;
        const double den = ((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                               1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                            2.05319162663775882187e+0) * r + 1.0;
        val = num / den;
    } else {
        r -= 5.0;
        const double num = ((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                               2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                            5.46378491116411436990e+0) * r + 6.65790464350110377720e+0;
        const double den = ((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                               7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                            5.99832206555887937690e-1) * r + 1.0;
        val = num / den;
    }
    return q < 0.0 ? -val : val;
}

// numpy's linear (type-7) interpolation between the order statistics a <= b with weight t, in its operation order and without contraction
__device__ __forceinline__ double cd_lerp(double a, double b, double t) {
    const double diff = __dsub_rn(b, a);
    if (t >= 0.5) return __dsub_rn(b, __dmul_rn(diff, __dsub_rn(1.0, t)));
    return __dadd_rn(a, __dmul_rn(diff, t));
}

// value s (0 <= s < S') of a coordinate's split-surviving series: split chain m = s / n holds draws [0, n) (m even) or [T - n, T) (m odd)
__device__ __forceinline__ double cd_split_value(const CdShape &sh, const double *__restrict__ xv, int64_t s) {
    const int64_t m = s / sh.n, i = s - m * sh.n;
    return xv[(size_t)(m >> 1) * sh.T + ((m & 1) ? sh.T - sh.n : 0) + i];
}

// ---- sorted tiles: tile t of a coordinate holds its values s in [t CD_TILE, (t + 1) CD_TILE), ascending, padded with +inf -----------------
// FOLD: of |x - median| (the median's two order statistics were published by the !FOLD rank kernel)
template <bool FOLD>
__global__ __launch_bounds__(CD_THREADS) void pf_cd_tilesort_kernel(CdShape sh, int64_t ntiles, const double *__restrict__ xs,
                                                                   const int32_t *__restrict__ flag, const double *__restrict__ ostat,
                                                                   double *__restrict__ sorted) {
    __shared__ double tile[CD_TILE];
    const int v = blockIdx.y, tid = threadIdx.x;
    if (flag[v]) return;                                           // workgroup-uniform
    const double *xv = xs + (size_t)v * sh.R;
    const double med = FOLD ? (ostat[6 * (size_t)v] + ostat[6 * (size_t)v + 1]) * 0.5 : 0.0;
    const int64_t j0 = (int64_t)blockIdx.x * CD_TILE;
    for (int e = tid; e < CD_TILE; e += CD_THREADS) {
        const int64_t s = j0 + e;
        double x = INFINITY;                                       // +inf counts for no finite value
        if (s < sh.Sp) {
            x = cd_split_value(sh, xv, s);
            if (FOLD) x = fabs(x - med);
        }
        tile[e] = x;
    }
    __syncthreads();
    for (int k = 2; k <= CD_TILE; k <<= 1)                         // bitonic sort, ascending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = tid; e < CD_TILE; e += CD_THREADS) {
                const int l = e ^ j;
                if (l > e) {
                    const double a = tile[e], b = tile[l];
                    if ((a > b) == ((e & k) == 0)) { tile[e] = b; tile[l] = a; }
                }
            }
            __syncthreads();
        }
    double *o = sorted + ((size_t)v * ntiles + blockIdx.x) * CD_TILE;
    for (int e = tid; e < CD_TILE; e += CD_THREADS) o[e] = tile[e];
}

// number of the CD_TILE ascending values of `tile` that are < x (LE: <= x): a branch-free binary search over the first CD_TILE - 1
// values (the steps CD_TILE / 2 ... 1 add up to CD_TILE - 1), then the last one
template <bool LE>
__device__ __forceinline__ unsigned cd_tile_count(const double *tile, double x) {
    unsigned lo = 0;
#pragma unroll
    for (unsigned step = CD_TILE / 2; step > 0; step >>= 1) {
        const double t = tile[lo + step - 1];
        lo += (LE ? t <= x : t < x) ? step : 0u;
    }
    const double t = tile[lo];
    return lo + ((LE ? t <= x : t < x) ? 1u : 0u);
}

// ---- ranks by counting against the sorted tiles -> z = PPND16((rank - 3/8) / (S' + 1/4)); !FOLD also publishes the order statistics ----------
template <bool FOLD>
__global__ __launch_bounds__(CD_THREADS) void pf_cd_rank_kernel(CdShape sh, int64_t ntiles, const double *__restrict__ xs,
                                                               const int32_t *__restrict__ flag, const double *__restrict__ sorted,
                                                               double *__restrict__ ostat, double *__restrict__ zout) {
    __shared__ double tile[CD_TILE];
    const int v = blockIdx.y, tid = threadIdx.x;
    if (flag[v]) return;                                           // workgroup-uniform
    const double *xv = xs + (size_t)v * sh.R;
    const double med = FOLD ? (ostat[6 * (size_t)v] + ostat[6 * (size_t)v + 1]) * 0.5 : 0.0;
    const int64_t s0 = (int64_t)blockIdx.x * (CD_THREADS * CD_IPT) + tid;
    double xi[CD_IPT];
    unsigned lt[CD_IPT], le[CD_IPT];
#pragma unroll
    for (int q = 0; q < CD_IPT; ++q) {
        const int64_t s = s0 + q * CD_THREADS;
        double x = 0.0;
        if (s < sh.Sp) {
            x = cd_split_value(sh, xv, s);
            if (FOLD) x = fabs(x - med);
        }
        xi[q] = x;
        lt[q] = le[q] = 0u;
    }
    for (int64_t t = 0; t < ntiles; ++t) {
        const double *src = sorted + ((size_t)v * ntiles + t) * CD_TILE;
        __syncthreads();
        for (int e = tid; e < CD_TILE; e += CD_THREADS) tile[e] = src[e];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < CD_IPT; ++q) {
            lt[q] += cd_tile_count<false>(tile, xi[q]);
            le[q] += cd_tile_count<true>(tile, xi[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < CD_IPT; ++q) {
        const int64_t s = s0 + q * CD_THREADS;
        if (s >= sh.Sp) continue;
        const double rank = 0.5 * ((double)lt[q] + (double)le[q] + 1.0);
        zout[(size_t)v * sh.Sp + s] = cd_ppnd16((rank - 0.375) / ((double)sh.Sp + 0.25));
        if (!FOLD) {
#pragma unroll
            for (int o = 0; o < 6; ++o)                            // equal values write equal numbers
                if ((int64_t)lt[q] <= sh.os[o] && sh.os[o] < (int64_t)le[q]) ostat[6 * (size_t)v + o] = xi[q];
        }
    }
}

// ---- split R-hat and Geyer ESS of one series ---------------------------------------------------------------------------------------
// KIND 0: x itself (xs), 1: a materialised series [S'], 2: the indicator [x <= q] of xs
template <int KIND>
__device__ __forceinline__ void cd_series(const CdShape &sh, const double *__restrict__ src, double q, bool want_ess,
                                          double *__restrict__ chmean, double *red, double *out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = CD_THREADS / 64;
    const int64_t n = sh.n;
    const int M = sh.M;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    auto chain = [&](int m) { return KIND == 1 ? src + (size_t)m * n : src + (size_t)(m >> 1) * sh.T + ((m & 1) ? sh.T - n : 0); };
    auto val = [&](const double *p, int64_t i) {
        const double x = p[i];
        return KIND == 2 ? (x <= q ? 1.0 : 0.0) : x;
    };
    for (int m = wave; m < M; m += nw) {                           // chain means: one wave per chain
        const double *p = chain(m);
        const double v0 = val(p, 0);
        double s = 0.0, ne = 0.0;
        for (int64_t i = lane; i < n; i += 64) {
            const double t = val(p, i);
            s += t;
            ne += t != v0 ? 1.0 : 0.0;
        }
        s = pf_wave_sum(s);
        ne = pf_wave_sum(ne);
        if (lane == 0) chmean[m] = ne == 0.0 ? v0 : s / (double)n;   // a constant chain: its value, exactly, so that W = 0 is exact
    }
    __syncthreads();
    double W = 0.0, varp = 0.0, sumP = 0.0, prevP = 0.0, tail = 0.0;
    const int64_t NP = (n - 1) / 2;                                // pairs with 2 j + 1 <= n - 2
    for (int64_t t0 = 0;; t0 += CD_LAGS) {
        double acc[CD_LAGS];
#pragma unroll
        for (int b = 0; b < CD_LAGS; ++b) acc[b] = 0.0;
        for (int m = wave; m < M; m += nw) {
            const double *p = chain(m);
            const double mu = chmean[m];
            for (int64_t i = lane; i < n - t0; i += 64) {
                const double a = val(p, i) - mu;
#pragma unroll
                for (int b = 0; b < CD_LAGS; ++b) {
                    const int64_t j = i + t0 + b;
                    const double c = j < n ? val(p, j) - mu : 0.0;
                    acc[b] += a * c;
                }
            }
        }
        pf_block_sum<CD_LAGS>(acc, red);                           // every thread holds the sums over all M chains
        double rho[CD_LAGS];
        if (t0 == 0) {
            const double g0 = acc[0] / (double)n / (double)M;      // mean_m gamma_m(0)
            W = (double)n / (double)(n - 1) * g0;
            double mm = 0.0, ss = 0.0;                             // var_m(chain means, ddof = 1), chains in order
            for (int m = 0; m < M; ++m) mm += chmean[m];
            mm /= (double)M;
            for (int m = 0; m < M; ++m) ss += (chmean[m] - mm) * (chmean[m] - mm);
            varp = (double)(n - 1) / (double)n * W + ss / (double)(M - 1);
            if (!(W > 0.0)) {                                      // a constant series (or indicator): NaN, not an error
                if (tid == 0) { out[0] = nan; out[1] = nan; }
                return;
            }
            if (tid == 0) out[1] = sqrt(varp / W);
            if (!want_ess) return;
        }
#pragma unroll
        for (int b = 0; b < CD_LAGS; ++b) rho[b] = 1.0 - (W - acc[b] / (double)n / (double)M) / varp;
        if (t0 == 0) rho[0] = 1.0;
        bool done = false, ran_out = false;
#pragma unroll
        for (int b = 0; b < CD_LAGS; b += 2) {
            if (done) continue;
            const int64_t j = t0 / 2 + b / 2;
            if (j >= NP) { done = true; ran_out = true; continue; }
            const double P = rho[b] + rho[b + 1];
            if (!(P > 0.0)) { done = true; tail = fmax(rho[b], 0.0); continue; }
            const double Pm = j == 0 ? P : fmin(prevP, P);
            sumP += Pm;
            prevP = Pm;
        }
        if (done) {
            double tau = -1.0 + 2.0 * sumP + (ran_out ? 0.0 : tail);
            tau = fmax(tau, 1.0 / log10((double)sh.Sp));
            if (tid == 0) out[0] = (double)sh.Sp / tau;
            return;
        }
    }
}

// grid (CD_NSERIES, V); st [V][CD_NSERIES][2] = (ess, rhat); chmean [V][CD_NSERIES][M]
__global__ __launch_bounds__(CD_THREADS) void pf_cd_ess_kernel(CdShape sh, const double *__restrict__ xs, const double *__restrict__ zs,
                                                              const double *__restrict__ zf, const double *__restrict__ ostat,
                                                              const int32_t *__restrict__ flag, double *__restrict__ chmean,
                                                              double *__restrict__ st) {
    __shared__ double red[CD_LAGS * (CD_THREADS / 64)];
    const int tr = blockIdx.x, v = blockIdx.y;
    if (flag[v]) return;
    double *cm = chmean + ((size_t)v * CD_NSERIES + tr) * sh.M;
    double *out = st + ((size_t)v * CD_NSERIES + tr) * 2;
    const double *xv = xs + (size_t)v * sh.R, *os = ostat + 6 * (size_t)v;
    switch (tr) {
    case 0: cd_series<0>(sh, xv, 0.0, true, cm, red, out); break;
    case 1: cd_series<1>(sh, zs + (size_t)v * sh.Sp, 0.0, true, cm, red, out); break;
    case 2: cd_series<1>(sh, zf + (size_t)v * sh.Sp, 0.0, false, cm, red, out); break;
    case 3: cd_series<2>(sh, xv, cd_lerp(os[2], os[3], sh.t05), true, cm, red, out); break;
    default: cd_series<2>(sh, xv, cd_lerp(os[4], os[5], sh.t95), true, cm, red, out); break;
    }
}

// out [CD_NOUT][V]: mean, sd, mcse_mean, ess_mean, ess_bulk, ess_tail, rhat; a NaN among the inputs of a min / max stays a NaN
__global__ void pf_cd_final_kernel(int V, const double *__restrict__ mom, const int32_t *__restrict__ flag, const double *__restrict__ st,
                                   double *__restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double r[CD_NOUT];
    if (flag[v]) {
#pragma unroll
        for (int q = 0; q < CD_NOUT; ++q) r[q] = nan;
    } else {
        const double *s = st + (size_t)v * CD_NSERIES * 2;
        const double e05 = s[6], e95 = s[8], r1 = s[3], r2 = s[5];
        r[0] = mom[2 * (size_t)v];
        r[1] = mom[2 * (size_t)v + 1];
        r[3] = s[0];
        r[2] = r[1] / sqrt(r[3]);
        r[4] = s[2];
        r[5] = (e05 != e05 || e95 != e95) ? nan : fmin(e05, e95);
        r[6] = (r1 != r1 || r2 != r2) ? nan : fmax(r1, r2);
    }
#pragma unroll
    for (int q = 0; q < CD_NOUT; ++q) out[(size_t)q * V + v] = r[q];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
struct CdLayout { size_t xs, zs, zf, sorted, ostat, chmean, st, mom, out, flag, bytes; };   // offsets in bytes

static int64_t cd_ntiles(const CdShape &sh) { return (sh.Sp + CD_TILE - 1) / CD_TILE; }

static CdLayout cd_layout(const CdShape &sh) {
    CdLayout L;
    size_t o = 0;
    auto take = [&](size_t doubles) { const size_t at = o; o += sizeof(double) * doubles; return at; };
    L.xs = take((size_t)sh.V * sh.R);
    L.zs = take((size_t)sh.V * sh.Sp);
    L.zf = take((size_t)sh.V * sh.Sp);
    L.sorted = take((size_t)sh.V * cd_ntiles(sh) * CD_TILE);
    L.ostat = take((size_t)sh.V * 6);
    L.chmean = take((size_t)sh.V * CD_NSERIES * sh.M);
    L.st = take((size_t)sh.V * CD_NSERIES * 2);
    L.mom = take((size_t)sh.V * 2);
    L.out = take((size_t)sh.V * CD_NOUT);
    L.flag = take(((size_t)sh.V + 1) / 2);
    L.bytes = o;
    return L;
}

static CdShape cd_shape(int d, int64_t T, int K, bool with_lp) {
    CdShape sh;
    sh.d = d; sh.V = d + (with_lp ? 1 : 0); sh.K = K; sh.M = 2 * K;
    sh.T = T; sh.n = T / 2; sh.R = (int64_t)K * T; sh.Sp = (int64_t)sh.M * sh.n;
    const double ps[2] = {0.05, 0.95};
    double ts[2];
    sh.os[0] = sh.Sp / 2 - 1; sh.os[1] = sh.Sp / 2;               // S' is even: the median is the mean of the two middle values
    for (int q = 0; q < 2; ++q) {                                  // numpy: virtual index (S' - 1) p, its floor and the rest
        const double vi = (double)(sh.Sp - 1) * ps[q], lo = floor(vi);
        sh.os[2 + 2 * q] = (int64_t)lo;
        sh.os[3 + 2 * q] = (int64_t)lo + 1 < sh.Sp ? (int64_t)lo + 1 : sh.Sp - 1;
        ts[q] = vi - lo;
    }
    sh.t05 = ts[0]; sh.t95 = ts[1];
    return sh;
}

size_t pf_chain_diag_bytes(int d, int64_t T, int K, bool with_lp) { return cd_layout(cd_shape(d, T, K, with_lp)).bytes; }

// the seven outputs of the records d_rec [K][T][d] (and d_lp [K][T] as coordinate d when it is not NULL) into *d_out [CD_NOUT][V], a
// device pointer into c->cd_ws (sized by the caller: pf_chain_diag_bytes).  Enqueues on the ctx stream; no wait.
int32_t pf_launch_chain_diag(pfmi_ctx *c, const double *d_rec, const double *d_lp, int d, int64_t T, int K, const double **d_out) {
    const CdShape sh = cd_shape(d, T, K, d_lp != nullptr);
    const CdLayout L = cd_layout(sh);
    PF_CHECK(c->cd_ws.cap >= L.bytes, PFMI_ERR_STATE, "chain_diagnostics: workspace not reserved");
    char *ws = c->cd_ws.as<char>();
    double *xs = (double *)(ws + L.xs), *zs = (double *)(ws + L.zs), *zf = (double *)(ws + L.zf), *ostat = (double *)(ws + L.ostat);
    double *sorted = (double *)(ws + L.sorted);
    double *chmean = (double *)(ws + L.chmean), *st = (double *)(ws + L.st), *mom = (double *)(ws + L.mom), *out = (double *)(ws + L.out);
    int32_t *flag = (int32_t *)(ws + L.flag);
    hipStream_t s = c->stream;
    const int V = sh.V;
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_cd_transpose_kernel, dim3((unsigned)((sh.R + 31) / 32), (unsigned)((d + 31) / 32)), dim3(256), 0, s, d, sh.R, d_rec, xs);
    PF_HIP(hipGetLastError());
    if (d_lp) PF_HIP(hipMemcpyAsync(xs + (size_t)d * sh.R, d_lp, sizeof(double) * (size_t)sh.R, hipMemcpyDeviceToDevice, s));
    pf_kernel_end(c, "chain_diag_transpose");
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_cd_moments_kernel, dim3(V), dim3(CD_THREADS), 0, s, sh.R, xs, mom, flag);
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "chain_diag_moments");
    const int64_t ntiles = cd_ntiles(sh);
    const dim3 sgrid((unsigned)ntiles, (unsigned)V);
    const dim3 rgrid((unsigned)((sh.Sp + CD_THREADS * CD_IPT - 1) / (CD_THREADS * CD_IPT)), (unsigned)V);
    ++c->cd_plans[ntiles == 1 ? "chain_diag:count:one" : "chain_diag:count:tiled"];
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_cd_tilesort_kernel<false>, sgrid, dim3(CD_THREADS), 0, s, sh, ntiles, xs, flag, ostat, sorted);
    PF_HIP(hipGetLastError());
    hipLaunchKernelGGL(pf_cd_rank_kernel<false>, rgrid, dim3(CD_THREADS), 0, s, sh, ntiles, xs, flag, sorted, ostat, zs);
    PF_HIP(hipGetLastError());
    hipLaunchKernelGGL(pf_cd_tilesort_kernel<true>, sgrid, dim3(CD_THREADS), 0, s, sh, ntiles, xs, flag, ostat, sorted);
    PF_HIP(hipGetLastError());
    hipLaunchKernelGGL(pf_cd_rank_kernel<true>, rgrid, dim3(CD_THREADS), 0, s, sh, ntiles, xs, flag, sorted, ostat, zf);
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "chain_diag_rank");
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_cd_ess_kernel, dim3(CD_NSERIES, (unsigned)V), dim3(CD_THREADS), 0, s, sh, xs, zs, zf, ostat, flag, chmean, st);
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "chain_diag_ess");
    pf_kernel_begin(c);
    hipLaunchKernelGGL(pf_cd_final_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, V, mom, flag, st, out);
    PF_HIP(hipGetLastError());
    pf_kernel_end(c, "chain_diag_final");
    *d_out = out;
    return PFMI_OK;
}
