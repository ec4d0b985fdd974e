// elbo_qf_kernel.hip -- single-pass ELBO scan: rand_and_logpdf + target of every draw of a fit (reference
// src/mvnormal.jl:24-39, src/elbo.jl:12-16) WITHOUT ever forming the draw x.
//
// For the built-in targets logp(x) is a quadratic form in x (Gaussian family) or needs only x_1 and sum x_i^2 (funnel),
// and x = mu + U'(z - Vh tv), tv = T Vh'z is affine in the transformed normals z (z = u except z_head = V'u_head,
// src/woodbury.jl:136-143).  Expanding, with s = sqrt(alpha), c = mu - m, a = target diagonal precision:
//   sum_i a_i e_i^2 = C0 + sum a s^2 z^2 + 2 sum a c s z  +  tv'M tv - 2 tv'(v + A3),      A3 = Vh'(a s^2 . z)
//   Wd'e            = t0 + A4 - Nn tv,                                                        A4 = Wd'(s . z)
// with per-fit constants C0 = sum a c^2, M = Vh' diag(a s^2) Vh, v = Vh'(a c s), t0 = Wd'c, Nn = Wd' diag(s) Vh
// (computed by the scan itself from "pseudo draws", see the kernel).  The draws fold the linear term into the A3 operand: they
// accumulate A3' = Vh'(a s^2 z + 2 a c s) = A3 + 2v, whose row operand is the same fma that feeds the scalar sum a s^2 z^2 + 2 a c s z,
// and the draw's finish uses -2 tv'(A3' - v).  One pass over the rows therefore accumulates, per draw, |u|^2, two scalars and the three skinny
// contractions w = Vh'z, A3, A4 -- all with the SAME A operand tiles -- and the draw is finished with O(KC^2) flops.
// (Verified against the direct evaluation in extended precision: same 1e-14 relative error, no cancellation, because
// every term is a sum of squares or a projection of one.)
//
// Consequences for the hardware mapping:
//   * no second pass => the normals never have to be kept: a wave owns 16 draws end to end (lane (q, c): rows
//     16 blk + 4q + {0..3} of draw c = one Philox4x32 call per block), the 8 waves of a workgroup own 8 different
//     16-draw groups, and there is NO cross-wave reduction and no barrier in the steady state;
//   * the factor is only read: Vh is staged through LDS in 256-row chunks (double buffered) for any d, or kept fully
//     resident when it fits (d <= ~1100 at J = 6), in the exact lane order of the v_mfma_f64_4x4x4 A operand so that every
//     fetch is a conflict-free broadcast read;
//   * per 16-row block a wave issues 4 k-steps x (2 KC/4 + RPAD/4) quarter-size MFMAs (16 cycles each) -- the same
//     matrix work as the two-pass kernel -- plus the RNG.
#include <type_traits>
#include <stdio.h>
#include <stdlib.h>
#include "pfmi_common.h"
#include "elbo_args.h"
#ifndef QF_PROF
#define QF_PROF 0                       // 1: waves 0 and 5 of one workgroup in 1024 print the 10 ns ticks of their phases (experiments only)
#endif

#ifndef QF_WAVES
#define QF_WAVES 8                     // waves per workgroup = 16-draw groups in flight per fit
#endif
#define QF_THREADS (QF_WAVES * 64)
#ifndef QF_NG
#define QF_NG 2                        // 16-draw groups per wave (share the operand fetches of a block)
#endif
#ifndef QF_ABLATE
#define QF_ABLATE 0
#endif
#ifndef QF_PHILOX_HOIST
#define QF_PHILOX_HOIST 1              // 0: every generator call of the block loop runs all of its rounds (A/B builds)
#endif
#ifndef QF_PSEUDO_FLIGHT
#define QF_PSEUDO_FLIGHT 1             // 0: the c/s column of the pseudo group loads its inputs row by row, behind guards (A/B builds)
#endif
#ifndef QF_CS_LDS
#define QF_CS_LDS 1                    // 0: the c/s column is never staged in LDS, every block of the pseudo group loads and divides (A/B builds)
#endif
#ifndef QF_EPI_PAIR
#define QF_EPI_PAIR 1                  // 0: every group of a wave is finished on its own, its A operands read inside its chains (A/B builds)
#endif
#ifndef QF_EPI_MFMA4
#define QF_EPI_MFMA4 1                 // 0: the paired finish keeps the 16x16x4 MFMA at every KC (A/B builds; needs QF_EPI_PAIR)
#endif
#ifndef QF_NG2_MAXKC
#define QF_NG2_MAXKC 20                // two groups per wave up to this KC (round 2: 12; KC = 16, 20 take the register-lean block body)
#endif
// Wave balance (round 4).  The two waves of a SIMD (w and w + 4) do the same work, but the instruction arbiter prefers the OLDER wave and
// the kernel is issue bound (one wave alone keeps the SIMD ~96 % busy): in-kernel timers showed waves 0 - 3 done after 355 us and waves
// 4 - 7 after 540 us, i.e. the younger waves ran the last third of the workgroup's time alone, without a partner to fill their stalls.
// The waves therefore take turns at s_setprio 1, QF_PRIO_FAIR blocks at a time, and finish together: scan 22.04 -> 21.69 ms (periods of
// 8 / 16 / 32 blocks alike, 4: 21.77, 1: 21.87).  (Raising the priority of one wave's MFMA burst -- round 3's QF_SETPRIO -- was slower.)
#ifndef QF_PRIO_FAIR
#define QF_PRIO_FAIR 8                 // 0: off; power of two
#endif
#ifndef QF_PRIO_YOUNG
#define QF_PRIO_YOUNG 0                // 1: waves 4 .. 7 (the younger wave of every SIMD) run at s_setprio 1 for the whole kernel (experiment)
#endif
#ifndef QF_SETPRIO
#define QF_SETPRIO 0                   // s_setprio level during a group's MFMA burst (0 = off; A/B in profiles/r03_scan_experiments.md)
#endif
#define QF_MIN_FRONT 1024             // doubles in front of the inverse-CDF table (>= 2 * PF_ICDF_BFE_FRONT = 704)
static_assert(QF_MIN_FRONT >= 2 * PF_ICDF_BFE_FRONT, "the look-up's front guard");
// blocks (of 16 rows) per streamed chunk; KC = 32 halves it: two staging buffers of 16 blocks x 32 columns would not fit 160 KB of LDS
// (round 3: history_length 11..16 with d > ~1000 used to fail with "LDS too large")
template <int KC> struct qf_chb { static constexpr int v = (KC > 20) ? 8 : 16; };

// Results must not depend on the launch geometry (which fits fall into the tail launch, how a fit's groups are cut into pieces,
// which of a wave's groups a draw lands in): the block body exists in several inlined instances (first batch / steady state,
// group 0 / group 1), and with the default -ffp-contract=fast LLVM decides PER INSTANCE whether `a * b + c` becomes an fma -- round 3
// found ELBOs differing in the last bit between a 64-path and a 16-path launch of the same fits.  Every fused operation in this file is
// an explicit fma(); nothing else may be contracted.
#pragma clang fp contract(off)

typedef double qf_d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ qf_d4 qf_mfma16(double a, double b, qf_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ double qf_mfma4(double a, double b, double c) { return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0); }

// per-fit constant block in LDS (doubles): [0] C0  [1] mu_0  [2] s_0  [3] -   then v[KC], M[KC][KC], t0[RPAD], Nn[RPAD][KC], vh0[KC]
__host__ __device__ constexpr int qf_nconst(int KC, int RPAD) { return 4 + KC + KC * KC + RPAD + RPAD * KC + KC; }

// Doubles of LDS for the head transform's A operands.  Two groups per wave at KC <= 12 have no registers to spare in the block loop
// (256 VGPRs, two waves per SIMD) and use the four operands of a lane only in block 0 of each batch: the prologue parks them in LDS, one
// 16 x 16 tile in lane order, and the peeled first block reads them back (conflict-free ds_read_b64).  Every other instantiation keeps
// them in registers (KC <= 12, one group) or fetches them from L2 when a special block comes up (KC >= 16, two groups).
__host__ __device__ constexpr int qf_head_lds(int KC, int NG) { return (NG == 2 && KC < 16) ? 256 : 0; }

// a_i (target diagonal weight), c_i = mu_i - m_i for row i
template <int TGT>
__device__ __forceinline__ void qf_row_ac(const ElboArgs &A, const double *mu, int i, double &a, double &c) {
    if (TGT == 1) { a = A.t_a[i]; c = mu[i] - A.t_mean[i]; }
    else if (TGT == 2) { a = (i >= 1) ? 1.0 : 0.0; c = mu[i]; }
    else { a = 0.0; c = 0.0; }
}

// ---------------------------------------------------------------------------------------------------
// LDS layout of one staged chunk (nb blocks of 16 rows):
//   vh:  [(bl*4 + r)*NT + T][q*4 + i]  = Vh[row 16 bl + 4 q + r][4 T + i]      (16 contiguous doubles = one A operand)
//   rs:  [bl][arr][4 q + r], arr = 0: a s^2, 1: 2 a c s, 2: s
template <int KC>
__device__ __forceinline__ int qf_vh_pos(int lrow, int col) {
    const int bl = lrow >> 4, rr = lrow & 15, q = rr >> 2, r = rr & 3, T = col >> 2, i = col & 3;
    return (((bl * 4 + r) * (KC / 4) + T) << 4) + q * 4 + i;
}

// the kernel's argument block (same members, same order: the kernarg segment is laid out like this struct).  The hand-over pointers are
// read from the segment where they are needed -- as named parameters they would sit in SGPRs across the whole block loop, and the scan
// has none to spare (measured: +0.1 ms per config-3 scan from the extra spills).  cs_off: offset (in doubles from `lds`) of the staged c/s
// column, 16 * ch_blocks doubles behind the rest of the allocation; 0 = the launch has no room for it (launch_qf_ng)
struct QfKernArgs { ElboArgs A; int ch_blocks, nchunks, groups_per_wg, ngroups, n_whole, n_tail, ndep; double *cshare; unsigned *cflag; unsigned epoch; int cs_off; };
// which instantiations stage the c/s column: those with a pseudo group, except the register-lean body (two groups at KC >= 16), where it
// costs 8 B of scratch (<20, 2, 0, 2>: 64 -> 72 B, over the pin of tests/test_kernel_resources.py)
__host__ __device__ constexpr bool qf_cs_lds(int KC, int TGT, int NG) { return QF_CS_LDS != 0 && TGT != 0 && !(NG == 2 && KC >= 16); }
__device__ __forceinline__ int qf_arg_cs_off() {
    const char *ka = (const char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));                                   // read here, not carried from the kernel's entry
    return *reinterpret_cast<const int *>(ka + offsetof(QfKernArgs, cs_off));
}
#ifndef QF_SHARE_SPINS
#define QF_SHARE_SPINS 2000000          // x ~1 us: how long a dependent piece waits for its fit's constants before it gives up
#endif
template <int KC, int TGT, int RPAD, int NG>
__global__ __launch_bounds__(QF_THREADS) void pf_elbo_qf_kernel(ElboArgs A, int ch_blocks, int nchunks, int groups_per_wg, int ngroups, int n_whole,
                                                                  int n_tail, int ndep, double *, unsigned *, unsigned, int) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
#if QF_PROF
    const long long qf_t0 = wall_clock64();
    long long qf_tb = 0, qf_te = 0, qf_tp = 0, qf_last = 0;
#endif
    constexpr int NT = KC / 4, TR = RPAD / 4, NC = qf_nconst(KC, RPAD);
    constexpr int QF_CHB = qf_chb<KC>::v;
    // real draws accumulate A3' = A3 + 2v (the linear term folded into the A3 operand, see the top of the file) -- except in the
    // register-lean body (two groups, KC >= 16): there the fused operand needs both row scalars at once, and the extra LDS waits and
    // wait states cost more than the saved f64 adds (tools/qf_issue_count.py at <20, 2, 0, 2>)
    constexpr bool FOLD = !(NG == 2 && KC >= 16);
    // the block loop's generator calls start from the per-draw share of Philox rounds 1 - 3 (pf_philox4x32_hoisted: the same words)
    constexpr bool PHX = QF_PHILOX_HOIST != 0;
    constexpr int PRE = (QF_CHB * 16 * KC + QF_THREADS - 1) / QF_THREADS;      // prefetch registers per thread (streaming)
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15, l3 = lane & 3;
    const int d = A.d, nblk = (d + 15) >> 4;
    // cshare == nullptr: workgroup (x, y) = piece x of fit y.  Otherwise (grid.x == 1) the first n_whole workgroups take one fit each;
    // behind them every one of the n_tail remaining fits is cut into one-batch pieces that fill the CUs the last round of whole fits
    // leaves idle: first the n_tail PUBLISHERS (role 1: the pseudo groups + the first groups of the fit; they hand the per-fit
    // constants over through `cshare` / `cflag`), then the ndep DEPENDENTS of each fit (role 2: a full batch of real groups, the
    // constants fetched before the first draw is finished).  A workgroup that waits was dispatched after every publisher.
    int slot = blockIdx.y, role = 0;
    int g_begin = blockIdx.x * groups_per_wg, g_cap = groups_per_wg;
    if (n_tail > 0 && slot >= n_whole) {
        constexpr int SL = QF_WAVES * NG, NPG_ = (TGT != 0) ? (KC + 1 + 15) / 16 : 0;
        int tail_f;
        if (slot < n_whole + n_tail) { role = 1; tail_f = slot - n_whole; g_begin = 0; g_cap = SL - NPG_; }
        else {
            const int t = slot - n_whole - n_tail;
            role = 2; tail_f = t / ndep;
            g_begin = (SL - NPG_) + (t - tail_f * ndep) * SL; g_cap = SL;
        }
        slot = n_whole + tail_f;
    }
    const int p = A.points[slot];
    const size_t blkidx = A.by_point ? (size_t)p : (size_t)slot;
    double *out_lp = A.logp + blkidx * A.log_stride, *out_lq = A.logq + blkidx * A.log_stride;
    // this workgroup's 16-draw groups [g_begin, g_end), preceded by NPG "pseudo groups" whose columns are the KC columns of
    // Vh and c/s: pushing them through the SAME contraction code yields the per-fit constants
    //   A3(Vh[:, j]) = M[:, j], A4(Vh[:, j]) = Nn[:, j], A3(c/s) = v, A4(c/s) = t0, q12(c/s) = 3 C0
    // in the first batch, for one wave-slot (the 63 real groups of N = 1000 leave exactly one of 64 slots free)
    constexpr int NPG = (TGT != 0) ? (KC + 1 + 15) / 16 : 0;
    const int npg = (role == 2) ? 0 : NPG;                         // a dependent gets the constants from its fit's publisher
    const int g_end = (g_begin + g_cap < ngroups) ? g_begin + g_cap : ngroups;
    const int nlb = (npg + (g_end - g_begin) + QF_WAVES * NG - 1) / (QF_WAVES * NG);   // batches of this workgroup
    if (A.status[p] != PFMI_FIT_OK) {
        for (int64_t n = (int64_t)g_begin * 16 + tid; n < (int64_t)g_end * 16 && n < A.N; n += QF_THREADS) {
            out_lp[n] = NAN; out_lq[n] = NAN;
        }
        return;
    }
    // ---- LDS carve-up (offsets in doubles from `lds`; plain offsets keep every access a ds_ instruction)
    const int vh_sz = ch_blocks * 16 * KC, rs_sz = ch_blocks * 48;
    const int buf_stride = (nchunks > 1) ? vh_sz + rs_sz : 0;       // second staging buffer only when streaming
    // the clamp-free interval look-up (pf_icdf_issue_bfe) may read up to PF_ICDF_BFE_FRONT x 16 B = 5.5 KB in FRONT of the table: keep at
    // least that much staged data before it (only matters for d < 64); the PF_ICDF_BFE_BEHIND entries behind it are the end of the
    // allocation (qf_lds_bytes)
    const int stage_sz = (nchunks > 1 ? 2 : 1) * (vh_sz + rs_sz);
    const int fix_off = stage_sz > QF_MIN_FRONT ? stage_sz : QF_MIN_FRONT;
    double *t_s = lds + fix_off;                   // [KC][KC]
    double *cn_s = t_s + KC * KC;                  // [NC]
    double *g_s = cn_s + NC;                       // [RPAD][RPAD]
    double *h_s = g_s + RPAD * RPAD;               // [4][64] head-transform operands, lane order (two groups per wave at KC <= 12 only)
    double2 *icdf = reinterpret_cast<double2 *>(h_s + qf_head_lds(KC, NG) + ((KC * KC + NC + RPAD * RPAD) & 1));   // [2 * 608] inverse-CDF table + guard

    const double *Vh = A.vh + (size_t)p * d * KC, *mu = A.mu + (size_t)p * d, *sqa = A.sqrt_alpha + (size_t)p * d;
    auto stage_direct = [&](int ck, int buf) {
        // (round 4: the loads of a trip are issued together.  As plain loops with a guarded load per element these were one global round
        //  trip per element -- `global_load; s_waitcnt vmcnt(0); ds_write` 24 times per thread for the factor block of config 3, ~7 % of
        //  a workgroup's time, with nothing to overlap it: one workgroup per CU.)
        const int row0 = ck * ch_blocks * 16;
        double *vs = lds + buf * buf_stride, *rs = vs + vh_sz;
        // the chunk is contiguous in the row-major factor block: 16-byte loads of column pairs (KC is even: a pair never straddles rows)
        const int npair = ch_blocks * 8 * KC;
        const int lim = (d - row0) * KC;                                       // doubles of this chunk that exist (rows < d)
        const double2 *src = reinterpret_cast<const double2 *>(Vh + (size_t)row0 * KC);
        constexpr int U = 6;
        for (int j0 = tid; j0 < npair; j0 += QF_THREADS * U) {
            double2 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u * QF_THREADS, jc = (2 * j + 1 < lim) ? j : (lim >> 1) - 1;
                v[u] = src[jc];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u * QF_THREADS, idx = 2 * j;
                if (j < npair) {
                    const int lrow = idx / KC, col = idx - lrow * KC;
                    const double2 val = (idx < lim) ? v[u] : make_double2(0.0, 0.0);
                    *reinterpret_cast<double2 *>(vs + qf_vh_pos<KC>(lrow, col)) = val;
                }
            }
        }
        // the c/s column of the pseudo group (column KC, see pseudo_cols), when the launch has room for it: formed here once per fit from the
        // row inputs that are in registers anyway, instead of twelve loads and four divisions per block in the wave that publishes
        int cs_o = 0;
        if constexpr (qf_cs_lds(KC, TGT, NG)) { if (npg > 0) cs_o = qf_arg_cs_off(); }
        for (int l0 = tid; l0 < ch_blocks * 16; l0 += QF_THREADS * 2) {
            double a[2], cc[2], s[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int lrow = l0 + u * QF_THREADS, row = row0 + lrow, rc = row < d ? row : d - 1;
                qf_row_ac<TGT>(A, mu, rc, a[u], cc[u]);
                s[u] = sqa[rc];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int lrow = l0 + u * QF_THREADS, row = row0 + lrow;
                if (lrow < ch_blocks * 16) {
                    const bool in = row < d;
                    double *o = rs + (lrow >> 4) * 48 + (lrow & 15);
                    o[0] = in ? a[u] * s[u] * s[u] : 0.0; o[16] = in ? 2.0 * a[u] * cc[u] * s[u] : 0.0; o[32] = in ? s[u] : 0.0;
                    if constexpr (qf_cs_lds(KC, TGT, NG)) { if (cs_o) lds[cs_o + lrow] = in ? cc[u] / s[u] : 0.0; }
                }
            }
        }
    };
    {
        const double *T = A.tmat + (size_t)p * KC * KC;
        for (int i = tid; i < KC * KC; i += QF_THREADS) t_s[i] = T[i];
        for (int i = tid; i < NC; i += QF_THREADS) cn_s[i] = 0.0;
        if (RPAD > 0) for (int i = tid; i < RPAD * RPAD; i += QF_THREADS) g_s[i] = A.t_g[i];
        pf_icdf_load(icdf);
        stage_direct(0, 0);
    }
    // head transform z_head = V'u_head as 16x16x4 MFMAs (same operand trick as the two-pass kernel): lane (q, c) supplies
    // A_r[i' = c][k = q] = H[rho(c)][4 q + r], H = V' identity padded; block 1 needs H10, H11 when KC > 16
    const int rho = 4 * (c & 3) + (c >> 2);
    // (two groups per wave at KC >= 16 need the registers: there the operands are fetched when a special block comes up -- L2, twice per
    // 16-draw group -- instead of living in 48 VGPRs for the whole kernel)
    constexpr bool HLDS = qf_head_lds(KC, NG) > 0;
    constexpr bool HREG = !(NG == 2 && KC >= 16) && !HLDS;
    const double *Vc = A.vchol + (size_t)p * KC * KC;
    auto head_op = [&](const int which, const int r) -> double {          // which: 0 = H00, 1 = H10, 2 = H11
        const int b = 4 * q + r;
        if (which == 0) { double v = (rho == b) ? 1.0 : 0.0; if (rho < KC && b < KC) v = Vc[b * KC + rho]; return v; }
        const int i1 = 16 + rho, b1 = 16 + b;
        if (which == 1) return (i1 < KC) ? Vc[b * KC + i1] : 0.0;
        double v1 = (i1 == b1) ? 1.0 : 0.0;
        if (i1 < KC && b1 < KC) v1 = Vc[b1 * KC + i1];
        return v1;
    };
    double a_h00[HREG ? 4 : 1], a_h10[HREG ? 4 : 1], a_h11[HREG ? 4 : 1];
    if (HREG) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            a_h00[HREG ? r : 0] = head_op(0, r);
            a_h10[HREG ? r : 0] = (KC > 16) ? head_op(1, r) : 0.0;
            a_h11[HREG ? r : 0] = (KC > 16) ? head_op(2, r) : 0.0;
        }
    }
    if (HLDS && wv == 0) {                                              // (KC < 16: H00 only; the same values in every wave)
#pragma unroll
        for (int r = 0; r < 4; ++r) h_s[r * 64 + lane] = head_op(0, r);
    }
    auto hop = [&](const int which, const int r) -> double {
        if (HLDS) return h_s[r * 64 + lane];
        if (HREG) return which == 0 ? a_h00[HREG ? r : 0] : (which == 1 ? a_h10[HREG ? r : 0] : a_h11[HREG ? r : 0]);
        return head_op(which, r);
    };
    const uint64_t seed = A.seeds[slot];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const double logdet = A.logdet[p];
    __syncthreads();
#if QF_PROF
    qf_tp = wall_clock64() - qf_t0; qf_last = wall_clock64();
#endif
#if QF_PRIO_YOUNG
    if (wv >= 4) __builtin_amdgcn_s_setprio(1);
#endif
    if (TGT == 2) {                                                 // funnel: tau = x_1 needs row 0 of the factor
        if (tid == 0) { cn_s[1] = mu[0]; cn_s[2] = sqa[0]; }
        if (tid < KC) cn_s[4 + KC + KC * KC + RPAD + RPAD * KC + tid] = Vh[tid];
    }

    // A wave owns NG 16-draw groups at a time ("slots" NG*wv + g of the batch): they share every operand fetch of a block
    // and give the scheduler NG independent RNG / MFMA streams to interleave.
    int cur = 0;
    for (int lb = 0; lb < nlb; ++lb) {
        bool pseudo[NG], active[NG];
        int sl[NG];
        int grp[NG];                                                // wave-uniform; the draw of lane column c is 16 grp + c
        pf_philox_inv pinv[NG];                                     // the draw's share of Philox rounds 1 - 3 (pfmi_common.h)
        // Philox counter word 0 of lane column c of group g.  Formed where it is used: the block loop needs it only on the refinement
        // path (probability 2^-19 per normal), its generator calls start from pinv[g]
        auto draw_of = [&](const int g) -> uint32_t { return (uint32_t)(A.n0 + ((int64_t)grp[g] * 16 + c)); };
        double accw[NG][NT], acc3[NG][NT], acc4[NG][TR > 0 ? TR : 1];
        double usq[NG], q12[NG], z00[NG], u0[NG][4];
        bool any_active = false, any_pseudo = false, any_real = false;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            sl[g] = (lb * QF_WAVES + wv) * NG + g;                  // wave-uniform slot
            pseudo[g] = sl[g] < npg;
            grp[g] = g_begin + sl[g] - npg;
            active[g] = pseudo[g] || grp[g] < g_end;
            if (PHX) {
                pinv[g] = pf_philox_draw_invariants(draw_of(g), k0, k1);
                // (register-lean body: the words pinned in registers, or part of them is formed again in every block -- one more VALU per
                //  block and 8 B more scratch at <20, 2, 0, 2>; the other bodies keep them live without it and measure 0.2 % faster so)
                if constexpr (NG == 2 && KC >= 16) asm volatile("" : "+v"(pinv[g].C), "+v"(pinv[g].D), "+v"(pinv[g].E), "+v"(pinv[g].F));
            }
            any_active |= active[g]; any_pseudo |= pseudo[g]; any_real |= active[g] && !pseudo[g];
#pragma unroll
            for (int T = 0; T < NT; ++T) { accw[g][T] = 0.0; acc3[g][T] = 0.0; }
#pragma unroll
            for (int T = 0; T < (TR > 0 ? TR : 1); ++T) acc4[g][T] = 0.0;
            usq[g] = 0.0; q12[g] = 0.0; z00[g] = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) u0[g][r] = 0.0;
        }
        // generator in two halves: `gen_issue` = Philox call, interval index, start of the two table reads per normal; `finish` =
        // the cubics + everything `normals` does.  Issuing every group's look-ups before finishing any keeps 8 (two groups) random
        // LDS reads in flight per lane.  (A deeper software pipeline -- look-ups issued one MFMA burst ahead, landing registers
        // shared by the alternating groups -- was built and measured in round 2: 25.3 vs 24.7 ms for two groups, 121 vs 95 ms for
        // one group at d = 10^4; with no MFMA / VALU co-issue on gfx950 there is nothing to hide the look-ups behind.)
        struct Pend { uint32_t x[4]; double dp[4]; double2 c01[4], c23[4]; };
        const uint32_t icdf_adj = pf_icdf_adj_bfe<PF_ICDF_NB_LDS>(icdf);
        auto gen_issue = [&](const int g, const int blk, const uint64_t t, Pend &P) {
            auto words = [&](uint32_t (&x)[4]) {
                if (PHX) pf_philox4x32_hoisted<PF_NORMAL_ROUNDS>(pinv[g], t, k0, k1, x);
                else pf_philox_normals(draw_of(g), (uint32_t)(blk * 4 + q), 0u, 0u, k0, k1, x);
            };
#if QF_ABLATE == 1                     // ablation (timing experiments only): no generator at all
#pragma unroll
            for (int r = 0; r < 4; ++r) { P.x[r] = 0x40000000u | (draw_of(g) + blk); P.dp[r] = 1e-3 * (blk + r); P.c01[r] = make_double2(0.1, 0.2); P.c23[r] = make_double2(0.3, 0.4); }
#elif QF_ABLATE == 2                   // ablation: Philox only, no table look-up
            words(P.x);
#pragma unroll
            for (int r = 0; r < 4; ++r) { P.dp[r] = (double)P.x[r] * 0x1p-32; P.c01[r] = make_double2(0.1, 0.2); P.c23[r] = make_double2(0.3, 0.4); }
#else
            words(P.x);
#pragma unroll
            for (int r = 0; r < 4; ++r) pf_icdf_issue_bfe<PF_ICDF_NB_LDS>(P.x[r], icdf_adj, P.dp[r], P.c01[r], P.c23[r]);
#endif
        };
        for (int ck = 0; ck < nchunks; ++ck) {
            // ---- streaming: fetch the next chunk (or chunk 0 for the next batch) into registers while this one is consumed
            double pre[PRE], pr_s = 0.0, pr_a = 0.0, pr_c = 0.0;
            const int nck = (ck + 1 < nchunks) ? ck + 1 : 0;
            const bool do_pre = (nchunks > 1) && (ck + 1 < nchunks || lb + 1 < nlb);
            if (do_pre) {
                const int row0 = nck * QF_CHB * 16;
                int tid_p = tid;                                   // opaque: see the refill below
                asm volatile("" : "+v"(tid_p));
#pragma unroll
                for (int e = 0; e < PRE; ++e) {
                    const int idx = tid_p + e * QF_THREADS;
                    const int lrow = idx / KC, row = row0 + lrow;
                    pre[e] = (idx < QF_CHB * 16 * KC && row < d) ? Vh[(size_t)row0 * KC + idx] : 0.0;
                }
                if (tid_p < QF_CHB * 16) {
                    const int row = row0 + tid_p;
                    if (row < d) { qf_row_ac<TGT>(A, mu, row, pr_a, pr_c); pr_s = sqa[row]; }
                }
            }
            if (any_active) {
                const double *vs = lds + cur * buf_stride, *rs = vs + vh_sz;
                const int blk0 = ck * ch_blocks;
                const int nb = (nblk - blk0 < ch_blocks) ? nblk - blk0 : ch_blocks;
                // operands of one block: A tiles of Vh (LDS), A tiles of Wd (L2), row scalars (LDS), fetched before the RNG
                struct Ops { double av[4][NT]; double wd[4][TR > 0 ? TR : 1]; double rs[12]; };
                auto load_ops = [&](const int bl, Ops &o) {
                    const double *rp = rs + bl * 48 + 4 * q;
                    const double *ap = vs + ((bl * 4) * NT << 4) + q * 4 + l3;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
#pragma unroll
                        for (int T = 0; T < NT; ++T) o.av[r][T] = ap[(r * NT + T) << 4];
                        o.rs[r] = rp[r]; o.rs[4 + r] = rp[16 + r]; o.rs[8 + r] = rp[32 + r];
                    }
                    if (TGT == 1 && RPAD > 0) {
                        const double *wp = A.t_wd16 + ((size_t)(blk0 + bl) * 16 + 4 * q) * 16 + l3;
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int T = 0; T < TR; ++T) o.wd[r][T] = wp[r * 16 + 4 * T];
                    }
                };
                // the contractions of one group: w = Vh'z, A3' = Vh'(a s^2 z + 2 a c s) (real draws, FOLD; a pseudo group, with_w = false,
                // accumulates A3 = Vh'(a s^2 z) so that M and v come out directly, without the cancellation M = A3' - 2v), A4 = Wd'(s z),
                // and the two scalars
                auto contract = [&](const int g, const double (&z)[4], const Ops &o, const bool with_w) {
#if QF_SETPRIO                         // experiment (round 3): raise the wave's priority for its MFMA burst
                    __builtin_amdgcn_s_setprio(QF_SETPRIO);
#endif
                    // the B operands of the whole group first: each lands well before the MFMAs that read it (no s_nop in between)
                    double bp[4], bs[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        bp[r] = 0.0; bs[r] = 0.0;
                        if (TGT != 0) bp[r] = (with_w && FOLD) ? fma(o.rs[r], z[r], o.rs[4 + r]) : o.rs[r] * z[r];
                        if (TGT == 1 && RPAD > 0) bs[r] = o.rs[8 + r] * z[r];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (TGT != 0) q12[g] = fma((with_w && FOLD) ? bp[r] : bp[r] + o.rs[4 + r], z[r], q12[g]);
#pragma unroll
                        for (int T = 0; T < NT; ++T) {
                            if (with_w) accw[g][T] = qf_mfma4(o.av[r][T], z[r], accw[g][T]);
                            if (TGT != 0) acc3[g][T] = qf_mfma4(o.av[r][T], bp[r], acc3[g][T]);
                        }
                        if (TGT == 1 && RPAD > 0) {
#pragma unroll
                            for (int T = 0; T < TR; ++T) acc4[g][T] = qf_mfma4(o.wd[r][T], bs[r], acc4[g][T]);
                        }
                    }
#if QF_SETPRIO
                    __builtin_amdgcn_s_setprio(0);
#endif
                };
                // normals of rows 16 blk + 4q + {0..3} of draw n[g], head transform included
                auto normals = [&](const int g, const int blk, double (&z)[4]) {
                    uint32_t x[4];
                    pf_philox_normals(draw_of(g), (uint32_t)(blk * 4 + q), 0u, 0u, k0, k1, x);
                    pf_icdf4(x, draw_of(g), (uint32_t)(blk * 4 + q), 0u, k0, k1, icdf, z);
                    if (blk == nblk - 1) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) z[r] = (blk * 16 + 4 * q + r < d) ? z[r] : 0.0;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) usq[g] = fma(z[r], z[r], usq[g]);      // |u|^2 before the transform (src/mvnormal.jl:31)
                    if (blk == 0) {                                                    // z[1:k] = V'u[1:k] (src/woodbury.jl:139)
                        qf_d4 h = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int r = 0; r < 4; ++r) { u0[g][r] = z[r]; h = qf_mfma16(hop(0, r), z[r], h); }
#pragma unroll
                        for (int r = 0; r < 4; ++r) z[r] = h[r];
                        z00[g] = z[0];
                    } else if (KC > 16 && blk == 1) {
                        qf_d4 h = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int r = 0; r < 4; ++r) h = qf_mfma16(hop(1, r), u0[g][r], h);
#pragma unroll
                        for (int r = 0; r < 4; ++r) h = qf_mfma16(hop(2, r), z[r], h);
#pragma unroll
                        for (int r = 0; r < 4; ++r) z[r] = h[r];
                    }
                };
                // second half of the pipelined generator: normals of block blk from the pending coefficients (+ what `normals` does)
                auto finish = [&](const int g, const int blk, const Pend &P, double (&z)[4], auto special_tag) {
                    constexpr bool SPECIAL = decltype(special_tag)::value;       // first / second / last block of the scan
#pragma unroll
                    for (int r = 0; r < 4; ++r) z[r] = pf_icdf_finish(P.x[r], P.dp[r], P.c01[r], P.c23[r]);
                    if (__builtin_expect(__any(pf_icdf_miss4(P.x)), 0))          // probability 2^-19 per normal
                        pf_icdf4_fix(P.x, draw_of(g), (uint32_t)(blk * 4 + q), 0u, k0, k1, z);
                    if (SPECIAL) {
                        if (blk == nblk - 1) {                                   // rows >= d do not exist
#pragma unroll
                            for (int r = 0; r < 4; ++r) z[r] = (blk * 16 + 4 * q + r < d) ? z[r] : 0.0;
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) usq[g] = fma(z[r], z[r], usq[g]);
                        if (blk == 0) {                                          // z[1:k] = V'u[1:k] (src/woodbury.jl:139)
                            qf_d4 h = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                            for (int r = 0; r < 4; ++r) { u0[g][r] = z[r]; h = qf_mfma16(hop(0, r), z[r], h); }
#pragma unroll
                            for (int r = 0; r < 4; ++r) z[r] = h[r];
                            z00[g] = z[0];
                        } else if (KC > 16 && blk == 1) {
                            qf_d4 h = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                            for (int r = 0; r < 4; ++r) h = qf_mfma16(hop(1, r), u0[g][r], h);
#pragma unroll
                            for (int r = 0; r < 4; ++r) h = qf_mfma16(hop(2, r), z[r], h);
#pragma unroll
                            for (int r = 0; r < 4; ++r) z[r] = h[r];
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) usq[g] = fma(z[r], z[r], usq[g]);      // |u|^2 before the transform (src/mvnormal.jl:31)
                    }
                };
                // pseudo group: column j of this lane is Vh[:, j] (j < KC) or c/s (j == KC); no RNG, no head transform
                // (cs_o != 0: the c/s column was staged by stage_direct -- the same operands, the same division -- and is read back: no global
                //  load and no division here, for every target)
                auto pseudo_cols = [&](const int g, const int blk, const int bl, const int cs_o, double (&z)[4]) {
                    const int j = 16 * sl[g] + c;
                    if (qf_cs_lds(KC, TGT, NG) && cs_o != 0) {
                        const double *cs = lds + cs_o + bl * 16 + 4 * q;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            double v = 0.0;
                            if (j < KC) v = vs[qf_vh_pos<KC>(bl * 16 + 4 * q + r, j)];
                            else if (j == KC) v = cs[r];                                     // (rows >= d were staged as 0)
                            z[r] = v;
                        }
                    } else if constexpr (QF_PSEUDO_FLIGHT != 0 && TGT == 1) {
                        // Gaussian targets: the inputs of the c/s column's four rows in one flight, from clamped addresses, then the
                        // subtractions and divisions.  As guarded loads they were one round trip per row (the loads, s_waitcnt vmcnt(0), the
                        // division), each of them waiting for the block's Wd loads as well, in the wave every other wave of the workgroup
                        // waits for before the constants are published.  (The funnel's column is two loads per row; in one flight it costs
                        // the register-lean body 16 B of scratch.)
                        double pm[4], ptm[4], ps[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = blk * 16 + 4 * q + r, rc = row < d ? row : d - 1;
                            pm[r] = mu[rc]; ptm[r] = A.t_mean[rc]; ps[r] = sqa[rc];
                        }
                        asm volatile("" ::: "memory");               // the loads stay above: none sinks into the guarded block of its row
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = blk * 16 + 4 * q + r;
                            double v = 0.0;
                            if (j < KC) v = vs[qf_vh_pos<KC>(bl * 16 + 4 * q + r, j)];
                            else if (j == KC && row < d) v = (pm[r] - ptm[r]) / ps[r];       // c = mu - m as in qf_row_ac
                            z[r] = v;
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = blk * 16 + 4 * q + r;
                            double v = 0.0;
                            if (j < KC) v = vs[qf_vh_pos<KC>(bl * 16 + 4 * q + r, j)];
                            else if (j == KC && row < d) {
                                double aa, cc;
                                qf_row_ac<TGT>(A, mu, row, aa, cc);
                                v = cc / sqa[row];
                            }
                            z[r] = v;
                        }
                    }
                };
                if (any_pseudo) {
                    // first batch only: the mixed pseudo / real wave.  Every other wave of the workgroup waits for it at the publish barrier
                    // (and a tail fit's dependents for their publisher), so its latencies are nobody's to hide but its own.
                    int cs_o = 0;
                    if constexpr (qf_cs_lds(KC, TGT, NG)) cs_o = qf_arg_cs_off();
                    for (int bl = 0; bl < nb; ++bl) {
                        Ops oa;
                        load_ops(bl, oa);
#pragma unroll
                        for (int g = 0; g < NG; ++g) {
                            if (!active[g]) continue;
                            double z[4];
                            if (pseudo[g]) { pseudo_cols(g, blk0 + bl, bl, cs_o, z); contract(g, z, oa, false); }
                            else { normals(g, blk0 + bl, z); contract(g, z, oa, true); }
                        }
                    }
                } else {
                    // one block of both groups; the body exists twice: interior blocks (no row masking, no head transform) and the
                    // first / second / last block (see the block loop below)
                    // KC >= 16 with two groups (round 3): the block is MFMA dominated (2 x 4 x 2 NT quarter-size MFMAs), registers are the
                    // scarce resource -- one set of pending look-ups at a time, and the A tiles of ONE k-step (4 rows) live at a time,
                    // shared by both groups' MFMAs (the r loop is outermost)
                    auto block_body_seq = [&](const int bl, auto special_tag) {
                        const int blk = blk0 + bl;
                        double z[NG][4];
                        const uint64_t t = pf_philox_block_product((uint32_t)(blk * 4 + q), k0);   // shared by the groups
#pragma unroll
                        for (int g = 0; g < NG; ++g) {
                            Pend pp;
                            gen_issue(g, blk, t, pp);
                            finish(g, blk, pp, z[g], special_tag);
                        }
                        const double *rp = rs + bl * 48 + 4 * q;
                        const double *ap = vs + ((bl * 4) * NT << 4) + q * 4 + l3;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            double av[NT];
#pragma unroll
                            for (int T = 0; T < NT; ++T) av[T] = ap[(r * NT + T) << 4];
                            const double r0 = rp[r], r1 = rp[16 + r];
#pragma unroll
                            for (int g = 0; g < NG; ++g) {
                                const double zr = z[g][r];
                                double bp = 0.0;
                                if (TGT != 0) {
                                    bp = r0 * zr;
                                    q12[g] = fma(bp + r1, zr, q12[g]);
                                }
#pragma unroll
                                for (int T = 0; T < NT; ++T) {
                                    accw[g][T] = qf_mfma4(av[T], zr, accw[g][T]);
                                    if (TGT != 0) acc3[g][T] = qf_mfma4(av[T], bp, acc3[g][T]);
                                }
                            }
                            if (TGT == 1 && RPAD > 0) {
                                const double *wp = A.t_wd16 + ((size_t)(blk0 + bl) * 16 + 4 * q + r) * 16 + l3;
                                double wd[TR > 0 ? TR : 1];
#pragma unroll
                                for (int T = 0; T < TR; ++T) wd[T] = wp[4 * T];
                                const double r2 = rp[32 + r];
#pragma unroll
                                for (int g = 0; g < NG; ++g) {
                                    const double bs = r2 * z[g][r];
#pragma unroll
                                    for (int T = 0; T < TR; ++T) acc4[g][T] = qf_mfma4(wd[T], bs, acc4[g][T]);
                                }
                            }
                        }
                    };
                    auto block_body = [&](const int bl, auto special_tag) {
                        if constexpr (NG == 2 && KC >= 16) { block_body_seq(bl, special_tag); return; }
                        const int blk = blk0 + bl;
                        Ops oa;
                        load_ops(bl, oa);                        // operands first: the generator below hides their latency
                        __builtin_amdgcn_sched_barrier(0);
                        Pend pp[NG];
                        double z[NG][4];
                        const uint64_t t = pf_philox_block_product((uint32_t)(blk * 4 + q), k0);   // shared by the groups
#pragma unroll
                        for (int g = 0; g < NG; ++g) gen_issue(g, blk, t, pp[g]);
#pragma unroll
                        for (int g = 0; g < NG; ++g) {           // the MFMA burst of group g hides the look-up latency of group g + 1
                            finish(g, blk, pp[g], z[g], special_tag);
#if QF_ABLATE == 3                     // ablation: generator only, no contraction
                            q12[g] += z[g][0] + z[g][1] + z[g][2] + z[g][3] + oa.av[0][0] + oa.rs[0];
#else
                            contract(g, z[g], oa, true);
#endif
                        }
                    };
                    // nothing of the LDS / scalar-memory queue may be pending when the block loop is entered: otherwise the compiler's wait
                    // counts at the loop head have to cover the unknown entry state and become a full `s_waitcnt lgkmcnt(0)` in EVERY
                    // block (the previous block's table reads drained before the next block's operand reads issue: +0.7 % per scan)
                    __builtin_amdgcn_s_waitcnt(0xC07F);
                    auto prio_turn = [&](const int blk) {
#if QF_PRIO_FAIR
                        // the two waves of a SIMD (w and w + 4) take turns at the higher issue priority, QF_PRIO_FAIR blocks at a time (see the
                        // note on wave balance at the launch code)
                        if ((blk & (QF_PRIO_FAIR - 1)) == 0) {
                            if (((blk / QF_PRIO_FAIR) ^ (wv >> 2) ^ lb) & 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
                        }
#endif
                    };
                    if constexpr (NG == 2 && KC >= 16) {
                        // register-lean body: ONE loop, the body selected per block (it has no accumulator copies to lose; peeled like
                        // below, its three inlined special bodies put 880 B per thread on the stack)
                        for (int bl = 0; bl < nb; ++bl) {
                            const int blk = blk0 + bl;
                            prio_turn(blk);
                            if (__builtin_expect((blk == 0) | (blk == nblk - 1) | (KC > 16 && blk == 1), 0)) block_body(bl, std::true_type{});
                            else block_body(bl, std::false_type{});
                        }
                    } else {
                        // The special blocks (the first, the second when KC > 16, the last) are peeled off the interior loop: blocks [0, s_lo)
                        // and [s_hi, nb) of this chunk run the special body as straight-line code, [s_lo, s_hi) the interior loop, in block
                        // order.  (Round 6 selected the body per block inside the one loop: the accumulators then merged from two bodies at
                        // the latch, 20 v_mov_b64 per block at <12, 1, 8, 2>, ~4 % of the block's issue -- tools/qf_issue_count.py,
                        // profiles/r07_scan_issue.md.  The special blocks as a loop of their own kept both loops' invariants alive across
                        // both: 56 -> 260 B of scratch.)
                        constexpr int LEAD = (KC > 16) ? 2 : 1;
                        const int s_lo = (LEAD - blk0 <= 0) ? 0 : (LEAD - blk0 < nb ? LEAD - blk0 : nb);
                        const int s_hi = (blk0 + nb == nblk) ? (nb - 1 > s_lo ? nb - 1 : s_lo) : nb;   // [s_hi, nb): at most the last block
#pragma unroll
                        for (int bl = 0; bl < LEAD; ++bl)
                            if (bl < s_lo) { prio_turn(blk0 + bl); block_body(bl, std::true_type{}); }
                        for (int bl = s_lo; bl < s_hi; ++bl) { prio_turn(blk0 + bl); block_body(bl, std::false_type{}); }
                        if (s_hi < nb) { prio_turn(blk0 + s_hi); block_body(s_hi, std::true_type{}); }
                    }
                }
            }
            if (nchunks > 1) {
                if (do_pre) {
                    double *vs = lds + (cur ^ 1) * buf_stride, *rs = vs + vh_sz;
                    // (opaque thread index: the per-thread LDS offsets of this refill are otherwise hoisted to the top of the kernel and
                    //  spilled there -- also by launches with a resident block, which never come here)
                    int tid_e = tid;
                    asm volatile("" : "+v"(tid_e));
#pragma unroll
                    for (int e = 0; e < PRE; ++e) {
                        const int idx = tid_e + e * QF_THREADS;
                        if (idx < QF_CHB * 16 * KC) { const int lrow = idx / KC; vs[qf_vh_pos<KC>(lrow, idx - lrow * KC)] = pre[e]; }
                    }
                    if (tid_e < QF_CHB * 16) {
                        double *o = rs + (tid_e >> 4) * 48 + (tid_e & 15);
                        o[0] = pr_a * pr_s * pr_s; o[16] = 2.0 * pr_a * pr_c * pr_s; o[32] = pr_s;
                    }
                }
                __syncthreads();
                cur ^= 1;
            }
        }
#if QF_PROF
        { const long long t_ = wall_clock64(); qf_tb += t_ - qf_last; qf_last = t_; }
#endif
        if (NPG > 0 && lb == 0) {                                  // publish the per-fit constants before any draw is finished
            int lane_p = lane;                                     // opaque lane coordinates (see the finishing section below)
            asm volatile("" : "+v"(lane_p));
            const int qp = lane_p >> 4, cp = lane_p & 15;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (!pseudo[g]) continue;
                const int j = 16 * sl[g] + cp;
                double *vv = cn_s + 4, *Mm = cn_s + 4 + KC, *t0 = Mm + KC * KC, *Nn = t0 + RPAD;
                const double q4 = pf_sum_q(q12[g]);
#pragma unroll
                for (int T = 0; T < NT; ++T) {
                    const int a = 4 * T + qp;
                    if (j < KC) Mm[a * KC + j] = acc3[g][T];
                    else if (j == KC) vv[a] = acc3[g][T];
                }
#pragma unroll
                for (int T = 0; T < TR; ++T) {
                    const int jr = 4 * T + qp;
                    if (j < KC) Nn[jr * KC + j] = acc4[g][T];
                    else if (j == KC) t0[jr] = acc4[g][T];
                }
                if (j == KC && qp == 0) cn_s[0] = q4 / 3.0;         // q12(c/s) = sum a c^2 + 2 sum a c^2
            }
            // (hand-over state re-read from the argument block, see QfKernArgs)
            double *cshare = nullptr; unsigned *cflag = nullptr; unsigned epoch = 0u; int tail_f = 0, n_tail_l = 0;
            if (role != 0) {
                const char *ka = (const char *)__builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(ka));
                cshare = *reinterpret_cast<double *const *>(ka + offsetof(QfKernArgs, cshare));
                cflag = *reinterpret_cast<unsigned *const *>(ka + offsetof(QfKernArgs, cflag));
                epoch = *reinterpret_cast<const unsigned *>(ka + offsetof(QfKernArgs, epoch));
                n_tail_l = *reinterpret_cast<const int *>(ka + offsetof(QfKernArgs, n_tail));
                const int n_whole_l = *reinterpret_cast<const int *>(ka + offsetof(QfKernArgs, n_whole));
                tail_f = slot - n_whole_l;
            }
            if (role == 2) {
                // the constants come from the fit's publisher (the same code on the same inputs: the same bits as computed here)
                if (tid == 0) {
                    int spins = 0;
                    while (__hip_atomic_load(cflag + tail_f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != epoch && spins < QF_SHARE_SPINS) {
                        __builtin_amdgcn_s_sleep(32); ++spins;
                    }
                    // (never seen.  Why a dependent cannot starve its publisher: publishers precede dependents in the grid, and a publisher never
                    //  blocks -- it needs nothing from anybody -- so once dispatched it always finishes; dispatch order is per XCD queue, not
                    //  device-wide, so a dependent may START first, but it only spins, it holds nothing a publisher waits for.  What the
                    //  time-out guards against is the publisher not being dispatched AT ALL for seconds: another process holding the CUs, CU
                    //  masking, a debugger / profiler serialising dispatch.  Draws finished without the constants would be silently wrong, so
                    //  they are poisoned and counted; pfmi_elbo_batch_wait turns the count into the retryable PFMI_ERR_RETRY and switches this
                    //  ctx to the two-launch cut, which has no in-kernel wait.)
                    if (spins >= QF_SHARE_SPINS) { cn_s[3] = NAN; atomicAdd(cflag + n_tail_l, 1u); }
                }
                __syncthreads();
                const bool lost = cn_s[3] != 0.0;
                int tid_s = tid;                                   // opaque: the per-thread offsets of this copy are formed here, not in the prologue
                asm volatile("" : "+v"(tid_s));
                const double *src = cshare + (size_t)tail_f * NC;
                double cv[(NC + QF_THREADS - 1) / QF_THREADS];
#pragma unroll
                for (int u = 0; u < (NC + QF_THREADS - 1) / QF_THREADS; ++u) {
                    const int i = tid_s + u * QF_THREADS;
                    cv[u] = __hip_atomic_load(src + (i < NC ? i : NC - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __syncthreads();                                   // everybody has read cn_s[3]
#pragma unroll
                for (int u = 0; u < (NC + QF_THREADS - 1) / QF_THREADS; ++u) {
                    const int i = tid_s + u * QF_THREADS;
                    if (i < NC) cn_s[i] = lost ? NAN : cv[u];
                }
            }
            __syncthreads();
            if (role == 1) {
                double *dst = cshare + (size_t)tail_f * NC;
                for (int i = tid; i < NC; i += QF_THREADS) __hip_atomic_store(dst + i, cn_s[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __threadfence();
                __syncthreads();
                if (tid == 0) __hip_atomic_store(cflag + tail_f, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (!any_real) continue;
        // The lane coordinates of this section come from an OPAQUE copy of the lane index: otherwise the compiler hoists the ~30 per-lane
        // LDS offsets and predicates of the matrix-vector products below out of the batch loop, keeps them alive across the whole block
        // loop and spills them in the prologue -- 140 bytes per thread, ~0.8 GB of scratch writes per scan launch (round 4; VERDICT r3
        // weak #8: WRITE_SIZE was 1.0 GB per launch where the log-density tables need 0.18 GB)
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int qe = lane_e >> 4, ce = lane_e & 15;
        // (the same for the draw index: formed here from an opaque wave index, it is not carried -- and spilled -- across the block loop)
        int wv_e = tid;
        asm volatile("" : "+v"(wv_e));
        wv_e >>= 6;
        int d_e = d;                                                // (and for the two constants (double) d feeds: one v_cvt here, not 8 B of scratch each)
        asm volatile("" : "+s"(d_e));
        // ---- finish the 16 draws of each group in registers: lane (q, c) holds entries 4T + q of w, A3, A4 of draw c
#if QF_EPI_PAIR
        // One finish for all groups of the wave (round 12).  The A operands of T, M, Nn and G are the same for every group and batch:
        // they are read once here, in one flight in front of the first cross-q sum, and the groups' chains run in lockstep -- T w of
        // every group, then M tv and Nn tv (independent of each other) step by step, then G tt -- so that no MFMA has the one issued
        // just before it as an operand.  Every dot product and sum keeps its operations and their order: the same bits.  A group that
        // is idle or a pseudo group goes through the same arithmetic on its zeroed / constant-bearing accumulators and stores nothing.
        {
            // M4 (QF_EPI_MFMA4, KC <= 12, where a 16-row tile is mostly padding): the products run on v_mfma_f64_4x4x4 -- lane (q, c)
            // holding entry 4T + q of draw c is its B operand (k = q, block = c >> 2, n = c & 3) and its result, the A operand is
            // Mat[4 rt + (lane & 3)][4 st + q] for all four blocks: one MFMA per 4 x 4 tile of Mat, the tiles of a row in a chain
            constexpr bool M4 = QF_EPI_MFMA4 != 0 && KC <= 12;
            constexpr int TRr = TR > 0 ? TR : 1;
            constexpr int NRT = M4 ? NT : (NT + 3) / 4, NRR = M4 ? TRr : (TRr + 3) / 4;   // row tiles of a KC-row / RPAD-row matrix
            constexpr bool LOWR = TGT == 1 && RPAD > 0;
            using acc_t = std::conditional_t<M4, double, qf_d4>;
            const int l3e = lane_e & 3;
            auto load_a = [&](const double *Mat, const int ld, const int nrows, auto lower_tag, auto &a) {
                constexpr bool LOWER = decltype(lower_tag)::value;
                constexpr int NR = sizeof(a) / sizeof(a[0]), NX = sizeof(a[0]) / sizeof(double);
#pragma unroll
                for (int rt = 0; rt < NR; ++rt) {
                    const int row = M4 ? 4 * rt + l3e : 16 * rt + ce;
#pragma unroll
                    for (int st = 0; st < NX; ++st) {
                        const int col = 4 * st + qe;
                        const bool ok = row < nrows && (!LOWER || col <= row);
                        a[rt][st] = ok ? Mat[row * ld + col] : 0.0;
                    }
                }
            };
            // step st of y = Mat x for every row tile and group: one MFMA each, all on different accumulators
            auto mv_step = [&](const int st, const auto &a, const auto &x, auto &acc) {
                constexpr int NR = sizeof(a) / sizeof(a[0]);
#pragma unroll
                for (int rt = 0; rt < NR; ++rt)
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        if constexpr (M4) acc[g][rt] = qf_mfma4(a[rt][st], x[g][st], acc[g][rt]);
                        else acc[g][rt] = qf_mfma16(a[rt][st], x[g][st], acc[g][rt]);
                    }
            };
            auto mv_zero = [&](auto &acc) {
                constexpr int NR = sizeof(acc[0]) / sizeof(acc_t);
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int rt = 0; rt < NR; ++rt) acc[g][rt] = acc_t{};
            };
            auto mv_out = [&](const auto &acc, auto &y) {
                constexpr int NR = sizeof(acc[0]) / sizeof(acc_t), NY = sizeof(y[0]) / sizeof(double);
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int rt = 0; rt < NR; ++rt) {
                        if constexpr (M4) { if (rt < NY) y[g][rt] = acc[g][rt]; }
                        else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) if (4 * rt + r < NY) y[g][4 * rt + r] = acc[g][rt][r];
                        }
                    }
            };
            const double *vv = cn_s + 4, *Mm = cn_s + 4 + KC, *t0 = Mm + KC * KC, *Nn = t0 + RPAD, *vh0 = Nn + RPAD * KC;
            double aT[NRT][NT], aM[NRT][NT], aN[NRR][NT], aG[NRR][TRr];
            if (TGT != 0) {
                load_a(t_s, KC, KC, std::false_type{}, aT);
                load_a(Mm, KC, KC, std::false_type{}, aM);
                if (LOWR) {
                    load_a(Nn, KC, RPAD, std::false_type{}, aN);
                    load_a(g_s, RPAD, RPAD, std::true_type{}, aG);
                }
                __builtin_amdgcn_sched_barrier(0);                  // the reads are in flight before the sums below start
            }
            double us[NG], lp[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) { us[g] = pf_sum_q(usq[g]); lp[g] = NAN; }
            if (TGT != 0) {
                double qs[NG], tvd[NG][NT], mt[NG][NT], nt[NG][TRr], q1[NG];
                acc_t cT[NG][NRT], cM[NG][NRT], cN[NG][NRR];
#pragma unroll
                for (int g = 0; g < NG; ++g) qs[g] = pf_sum_q(q12[g]);
                mv_zero(cT);
#pragma unroll
                for (int st = 0; st < NT; ++st) mv_step(st, aT, accw, cT);
                mv_out(cT, tvd);
                mv_zero(cM);
                if (LOWR) mv_zero(cN);
#pragma unroll
                for (int st = 0; st < NT; ++st) {
                    mv_step(st, aM, tvd, cM);
                    if (LOWR) mv_step(st, aN, tvd, cN);
                }
                mv_out(cM, mt);
                if (LOWR) mv_out(cN, nt);
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    double qa = 0.0;
#pragma unroll
                    for (int T = 0; T < NT; ++T)
                        qa = fma(tvd[g][T], mt[g][T] - 2.0 * (FOLD ? acc3[g][T] - vv[4 * T + qe] : vv[4 * T + qe] + acc3[g][T]), qa);   // A3' - v = A3 + v
                    qa = pf_sum_q(qa);
                    q1[g] = cn_s[0] + qs[g] + qa;
                }
                if (TGT == 1) {
                    double corr[NG];
#pragma unroll
                    for (int g = 0; g < NG; ++g) corr[g] = 0.0;
                    if (RPAD > 0) {
                        double tt[NG][TRr], gg[NG][TRr];
                        acc_t cG[NG][NRR];
#pragma unroll
                        for (int g = 0; g < NG; ++g)
#pragma unroll
                            for (int T = 0; T < TR; ++T) tt[g][T] = t0[4 * T + qe] + acc4[g][T] - nt[g][T];
                        mv_zero(cG);
#pragma unroll
                        for (int st = 0; st < TRr; ++st) mv_step(st, aG, tt, cG);
                        mv_out(cG, gg);
#pragma unroll
                        for (int g = 0; g < NG; ++g) {
#pragma unroll
                            for (int T = 0; T < TR; ++T) corr[g] = fma(gg[g][T], gg[g][T], corr[g]);
                            corr[g] = pf_sum_q(corr[g]);
                        }
                    }
#pragma unroll
                    for (int g = 0; g < NG; ++g) lp[g] = A.t_offset - 0.5 * (q1[g] - corr[g]);
                } else {                                                   // funnel: tau = x_1, ss = sum_{i>=2} x_i^2
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const double zh = __shfl(z00[g], ce, 64);
                        double pr = 0.0;
#pragma unroll
                        for (int T = 0; T < NT; ++T) pr = fma(vh0[4 * T + qe], tvd[g][T], pr);
                        pr = pf_sum_q(pr);
                        const double ta = cn_s[1] + cn_s[2] * (zh - pr), t3 = ta / 3.0;
                        lp[g] = (t3 * t3 + (double)(d_e - 1) * ta + q1[g] * exp(-ta)) / -2.0;
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (!active[g] || pseudo[g]) continue;
                const int64_t nl = (int64_t)(g_begin + (lb * QF_WAVES + wv_e) * NG + g - npg) * 16 + ce;
                if (qe == 0 && nl < A.N) {
                    out_lq[nl] = ((double)d_e * PF_LOG2PI + logdet + us[g]) / -2.0;     // src/mvnormal.jl:36
                    out_lp[nl] = lp[g];
                }
            }
        }
#else
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (!active[g] || pseudo[g]) continue;
            double us = usq[g];
            us = pf_sum_q(us);
            double lp = NAN;
            if (TGT != 0) {
                double qs = q12[g];
                qs = pf_sum_q(qs);
                // The small matrix-vector products of the 16 draws run on v_mfma_f64_16x16x4: lane (q, c) holds entries 4T + q of
                // draw c, which is both the B-operand layout (k = q, column = draw) and -- rows q + 4 reg -- the result layout, so
                // y = Mat x needs no cross-lane step at all; the A operand is Mat[row 16 rt + c][4 s + q] straight from LDS.  (Until
                // round 2 every entry of T w was a 4-lane shuffle sum and M tv, Nn tv ran on the VALU with tv replicated: 375 VALU +
                // 86 LDS instructions per group.)
                auto matvec = [&](const double *Mat, const int ld, const int nrows, auto nx_tag, auto ny_tag, auto lower_tag,
                                  const double (&x)[decltype(nx_tag)::value], double (&y)[decltype(ny_tag)::value]) {
                    constexpr int NX = decltype(nx_tag)::value, NY = decltype(ny_tag)::value;
                    constexpr bool LOWER = decltype(lower_tag)::value;
#pragma unroll
                    for (int rt = 0; rt < (NY + 3) / 4; ++rt) {
                        qf_d4 acc = {0.0, 0.0, 0.0, 0.0};
                        const int row = 16 * rt + ce;
#pragma unroll
                        for (int st = 0; st < NX; ++st) {
                            const int col = 4 * st + qe;
                            const bool ok = row < nrows && (!LOWER || col <= row);
                            const double av = ok ? Mat[row * ld + col] : 0.0;
                            acc = qf_mfma16(av, x[st], acc);
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) if (4 * rt + r < NY) y[4 * rt + r] = acc[r];
                    }
                };
                const double *vv = cn_s + 4, *Mm = cn_s + 4 + KC, *t0 = Mm + KC * KC, *Nn = t0 + RPAD, *vh0 = Nn + RPAD * KC;
                double tvd[NT], mt[NT];                                   // entries 4T + q of tv = T w and of M tv
                matvec(t_s, KC, KC, std::integral_constant<int, NT>{}, std::integral_constant<int, NT>{}, std::false_type{}, accw[g], tvd);
                matvec(Mm, KC, KC, std::integral_constant<int, NT>{}, std::integral_constant<int, NT>{}, std::false_type{}, tvd, mt);
                double qa = 0.0;
#pragma unroll
                for (int T = 0; T < NT; ++T)
                    qa = fma(tvd[T], mt[T] - 2.0 * (FOLD ? acc3[g][T] - vv[4 * T + qe] : vv[4 * T + qe] + acc3[g][T]), qa);   // A3' - v = A3 + v
                qa = pf_sum_q(qa);
                const double q1 = cn_s[0] + qs + qa;
                if (TGT == 1) {
                    double corr = 0.0;
                    if (RPAD > 0) {
                        constexpr int TRr = TR > 0 ? TR : 1;
                        double nt[TRr], tt[TRr], gg[TRr];
                        matvec(Nn, KC, RPAD, std::integral_constant<int, NT>{}, std::integral_constant<int, TRr>{}, std::false_type{}, tvd, nt);
#pragma unroll
                        for (int T = 0; T < TR; ++T) tt[T] = t0[4 * T + qe] + acc4[g][T] - nt[T];
                        matvec(g_s, RPAD, RPAD, std::integral_constant<int, TRr>{}, std::integral_constant<int, TRr>{}, std::true_type{}, tt, gg);
#pragma unroll
                        for (int T = 0; T < TR; ++T) corr = fma(gg[T], gg[T], corr);
                        corr = pf_sum_q(corr);
                    }
                    lp = A.t_offset - 0.5 * (q1 - corr);
                } else {                                                   // funnel: tau = x_1, ss = sum_{i>=2} x_i^2
                    const double zh = __shfl(z00[g], ce, 64);
                    double pr = 0.0;
#pragma unroll
                    for (int T = 0; T < NT; ++T) pr = fma(vh0[4 * T + qe], tvd[T], pr);
                    pr = pf_sum_q(pr);
                    const double ta = cn_s[1] + cn_s[2] * (zh - pr), t3 = ta / 3.0;
                    lp = (t3 * t3 + (double)(d_e - 1) * ta + q1 * exp(-ta)) / -2.0;
                }
            }
            const int64_t nl = (int64_t)(g_begin + (lb * QF_WAVES + wv_e) * NG + g - npg) * 16 + ce;
            if (qe == 0 && nl < A.N) {
                out_lq[nl] = ((double)d_e * PF_LOG2PI + logdet + us) / -2.0;        // src/mvnormal.jl:36
                out_lp[nl] = lp;
            }
        }
#endif
#if QF_PROF
        { const long long t_ = wall_clock64(); qf_te += t_ - qf_last; qf_last = t_; }
#endif
    }
#if QF_PROF
    if (g_begin == 0 && (slot & 1023) == 3 && lane == 0)
        printf("QF_PROF fit %d wave %d (10 ns ticks): prologue %lld blocks %lld epilogue+publish %lld total %lld batches %d\n", slot, wv, qf_tp, qf_tb,
               qf_te, (long long)(wall_clock64() - qf_t0), nlb);
#endif
}

// ---------------------------------------------------------------------------------------------------
static size_t qf_lds_bytes(int ch_blocks, int nchunks, int kc, int rpad, int ng) {
    const size_t per = (size_t)ch_blocks * 16 * kc + (size_t)ch_blocks * 48;
    size_t stage = per * (nchunks > 1 ? 2 : 1);
    if (stage < QF_MIN_FRONT) stage = QF_MIN_FRONT;
    return sizeof(double) * (stage + (size_t)kc * kc + qf_nconst(kc, rpad) + (size_t)rpad * rpad + qf_head_lds(kc, ng) + 1 + 4 * PF_ICDF_LDS_ENTRIES + 2 * PF_ICDF_BFE_BEHIND);
}

// the plan of one scan call, counted per ctx for pfmi_kernel_time (include/pfmi.h): instantiation, resident / streamed factor block, and the
// cut -- whole (a workgroup per fit, or per fit and piece), split (few fits: each cut into pieces), tail-share (the one-launch tail with
// its publishers and dependents), tail-two (the tail as a second launch)
static void qf_note_plan(pfmi_ctx *c, int kc, int tgt, int rpad, int ng, bool streamed, const char *cut) {
    char nm[64];
    snprintf(nm, sizeof nm, "qf:%d,%d,%d,%d:%s:%s", kc, tgt, rpad, ng, streamed ? "stream" : "res", cut);
    ++c->qf_plans[nm];
}

template <int KC, int TGT, int RPAD, int NG>
static int32_t launch_qf_ng(pfmi_ctx *c, const ElboArgs &a, int64_t nfits) {
    const int nblk = (a.d + 15) / 16;
    int ch_blocks = nblk, nchunks = 1;
    constexpr int QF_CHB = qf_chb<KC>::v;
    if (qf_lds_bytes(nblk, 1, KC, RPAD, NG) > 156 * 1024) { ch_blocks = QF_CHB; nchunks = (nblk + QF_CHB - 1) / QF_CHB; }
    size_t lds_bytes = qf_lds_bytes(ch_blocks, nchunks, KC, RPAD, NG);
    // the staged c/s column of the pseudo group (QF_CS_LDS): 16 doubles per block behind everything else, for a resident block, when the
    // request with it stays within the limit checked below.  The resident / streamed decision above does not look at it.
    int cs_off = 0;
    const char *no_cs = pf_debug_get("PFMI_QF_NO_CS_LDS");           // test hook: the column's loads and divisions in every block, as without room
    if (qf_cs_lds(KC, TGT, NG) && nchunks == 1 && !(no_cs && no_cs[0] == '1') &&
        lds_bytes + sizeof(double) * 16 * (size_t)ch_blocks <= 160 * 1024) {
        cs_off = (int)(lds_bytes / sizeof(double));
        lds_bytes += sizeof(double) * 16 * (size_t)ch_blocks;
    }
    PF_CHECK(lds_bytes <= 160 * 1024, PFMI_ERR_UNSUPPORTED, "qf kernel LDS %zu too large", lds_bytes);
    auto kern = pf_elbo_qf_kernel<KC, TGT, RPAD, NG>;
    PF_TRY(pf_raise_lds_limit(c, reinterpret_cast<const void *>(kern), 160 * 1024));
    const int ngroups = (int)((a.N + 15) / 16);
    constexpr int NPG = (TGT != 0) ? (KC + 1 + 15) / 16 : 0;
    // one workgroup per fit; a fit's groups are split over several workgroups only when there are few fits (every
    // workgroup recomputes the per-fit constants, so the pieces are kept to whole batches)
    // (a segment of the streaming pipeline that is not the last: whole fits only -- the next segment's workgroups fill the CUs this one leaves)
    int split = 1;
    while (!c->qf_seg_mode && (int64_t)split * nfits < 1024 && (ngroups + NPG) / (split * 2) >= QF_WAVES * NG) split *= 2;
    int gpw = (ngroups + split - 1) / split;
    if (split > 1) gpw = ((gpw + NPG + QF_WAVES * NG - 1) / (QF_WAVES * NG)) * (QF_WAVES * NG) - NPG;   // fill the last batch
    if (gpw < 1) gpw = 1;
    const int gx = (ngroups + gpw - 1) / gpw;
    auto launch = [&](int64_t f0, int64_t nf, int gpw_, int gx_) {
        for (int64_t s0 = f0; s0 < f0 + nf; s0 += 32768) {
            const int64_t ns = (f0 + nf - s0 < 32768) ? (f0 + nf - s0) : 32768;
            ElboArgs b = a;
            b.points = a.points + s0; b.seeds = a.seeds + s0;
            if (!a.by_point) { b.logp += s0 * a.log_stride; b.logq += s0 * a.log_stride; }
            hipLaunchKernelGGL(kern, dim3((unsigned)gx_, (unsigned)ns), dim3(QF_THREADS), lds_bytes, c->stream, b, ch_blocks, nchunks, gpw_,
                               ngroups, 0, 0, 0, (double *)nullptr, (unsigned *)nullptr, 0u, cs_off);
        }
    };
    // Workgroups of one launch all take the same time, so the fits beyond the last full round of CUs (nfits mod #CU) would keep a
    // few CUs busy for a whole workgroup time while the rest idle.  Those fits are cut into one-batch pieces whenever that finishes
    // sooner.  Regular route (round 4): ONE launch -- a workgroup per whole fit, then the pieces; only a fit's first piece (the
    // "publisher") spends a slot on the pseudo groups and hands the per-fit constants to the others through global memory, so that
    // N = 1000 (63 groups + 1 pseudo group = 4 batches) is 4 pieces of one full batch, no work added.  (Round 3: a second launch
    // in which every piece recomputed the constants -- 5 pieces per fit; kept behind PFMI_QF_TWO_LAUNCHES for the invariance tests
    // and for scans of more than 65 535 workgroups.)
    int64_t tail = 0;
    int gpw_t = gpw, gx_t = gx, ndep = 0;
    const char *no_tail = pf_debug_get("PFMI_QF_NO_TAIL");            // test hook: one workgroup per fit (geometry-invariance tests)
    const char *two = pf_debug_get("PFMI_QF_TWO_LAUNCHES");          // test hook: the round-3 cut
    const bool two_launches = (two && two[0] == '1') || c->qf_no_share;   // (qf_no_share: a hand-over timed out on this ctx before, pfmi_elbo_batch_wait)
    if (split == 1 && TGT != 0 && !(no_tail && no_tail[0] == '1') && !c->qf_seg_mode) {
        int ncu = 0;
        PF_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
        if (c->ncu_eff > 0 && c->ncu_eff < ncu) ncu = c->ncu_eff;           // streaming segments: the optimiser's workgroups hold some CUs
        const int slots = QF_WAVES * NG, nb_full = (ngroups + NPG + slots - 1) / slots;
        const int64_t rem = ncu > 0 ? nfits % ncu : 0;
        gpw_t = slots - NPG;
        gx_t = gpw_t > 0 ? (ngroups + gpw_t - 1) / gpw_t : 0;
        ndep = (ngroups > gpw_t) ? (ngroups - gpw_t + slots - 1) / slots : 0;
        const bool share_ok = !two_launches && gpw_t > 0 && (nfits - rem) + rem * (1 + ndep) <= 65535;
        const int pieces = share_ok ? 1 + ndep : gx_t;
        if (rem > 0 && nfits > ncu && gpw_t > 0 && nb_full > 1 && (rem * pieces + ncu - 1) / ncu < nb_full) tail = rem;
        if (tail > 0 && share_ok) {
            constexpr int NC = qf_nconst(KC, RPAD);
            const size_t cbytes = (size_t)tail * NC * sizeof(double), fbytes = ((size_t)tail + 1) * sizeof(unsigned);
            DevBuf &share = c->qf_share_s[c->qf_slot];
            uint32_t &epoch = c->qf_epoch_s[c->qf_slot];
            if (share.cap < cbytes + fbytes || epoch == 0xFFFFFFFFu) {          // (new flags start at 0 = "never published")
                PF_CHECK(!c->stream_pending, PFMI_ERR_STATE, "scan: the hand-over buffer of a streaming call must be allocated before its first launch");
                PF_TRY(share.ensure(cbytes + fbytes + (64 << 10)));
                PF_HIP(hipMemsetAsync(share.p, 0, share.cap, c->stream));
                epoch = 0;
            }
            // flags live at the END of the buffer so that a larger tail of a later launch never reads constants as flags
            unsigned *cflag = reinterpret_cast<unsigned *>(share.as<char>() + share.cap) - (tail + 1);
            hipLaunchKernelGGL(kern, dim3(1, (unsigned)((nfits - tail) + tail * (1 + ndep))), dim3(QF_THREADS), lds_bytes, c->stream, a, ch_blocks,
                               nchunks, gpw, ngroups, (int)(nfits - tail), (int)tail, ndep, share.as<double>(), cflag, ++epoch, cs_off);
            qf_note_plan(c, KC, TGT, RPAD, NG, nchunks > 1, "tail-share");
            return PFMI_OK;
        }
    }
    if (nfits - tail > 0) launch(0, nfits - tail, gpw, gx);
    if (tail > 0) launch(nfits - tail, tail, gpw_t, gx_t);
    qf_note_plan(c, KC, TGT, RPAD, NG, nchunks > 1, tail > 0 ? "tail-two" : (split > 1 ? "split" : "whole"));
    return PFMI_OK;
}

// two 16-draw groups per wave when the scan is long enough to fill whole batches of 2 x 8 slots (measured +1 % at N = 1000;
// short scans keep one group per wave so that more waves are busy); KC >= 16 would spill with two groups
template <int KC, int TGT, int RPAD>
static int32_t launch_qf(pfmi_ctx *c, const ElboArgs &a, int64_t nfits) {
    if constexpr (KC <= QF_NG2_MAXKC && QF_NG == 2) {
        // (KC >= 16: only when there are fits enough to fill the CUs -- a pool of a few fits wants more, smaller pieces)
        if (a.N >= 768 && (KC <= 12 || nfits >= 128)) return launch_qf_ng<KC, TGT, RPAD, 2>(c, a, nfits);
    }
    return launch_qf_ng<KC, TGT, RPAD, 1>(c, a, nfits);
}

template <int KC>
static int32_t launch_qf_t(pfmi_ctx *c, const ElboArgs &a, int64_t nfits, int tgt, int rpad) {
    if (tgt == 0) return launch_qf<KC, 0, 0>(c, a, nfits);
    if (tgt == 2) return launch_qf<KC, 2, 0>(c, a, nfits);
    if (rpad == 0) return launch_qf<KC, 1, 0>(c, a, nfits);
    if (rpad == 8) return launch_qf<KC, 1, 8>(c, a, nfits);
    return launch_qf<KC, 1, 16>(c, a, nfits);
}

// single-pass scan: in-kernel RNG, no draws written, any d; kpad in {4, 8, 12, 16, 20, 32}
int32_t pf_launch_elbo_qf(pfmi_ctx *c, const ElboArgs &a, int64_t nfits, int tgt, int rpad, bool *handled) {
    *handled = false;
    if (a.u != nullptr || a.x != nullptr) return PFMI_OK;
    int32_t rc = PFMI_OK;
    *handled = pf_dispatch_kpad<4, 8, 12, 16, 20, 32>(c->kpad, [&](auto KP) { rc = launch_qf_t<KP()>(c, a, nfits, tgt, rpad); });
    return rc;
}
