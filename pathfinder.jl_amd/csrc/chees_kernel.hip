// chees_kernel.hip -- ChEES-HMC on the fitted Woodbury factor (adapt.h: the rule; include/pfmi.h: pfmi_chees_enqueue): static HMC whose step
// size and trajectory length are shared by all chains and learned across them during the warm-up.  pf_chees_step_kernel is the step body
// of hmc_kernel.hip in its fourth mode, one kernel for warm-up and sampling, in a translation unit of its own as the metric kernels are.
//
// The chains run in lockstep (the leapfrog count of a transition is the same in every chain), so every chain ends warm-up transition t in
// the same launch.  The cross-chain update follows as launches of its own in stream order -- the kernel boundary is the only
// synchronisation between workgroups:
//     pf_chees_mean_kernel     one thread per coordinate, the chains in order: xbar, xbar'            (coalesced over i)
//     pf_chees_sums_kernel     one workgroup per chain: p_k, q_k, r_k, fixed-order block sums
//     pf_chees_scalar_kernel   one wave: the scalars (pf_chees_scalars), the shared state, the traces, every chain's hm_eps entry
// and then a step launch that opens transition t + 1 with the new step size and length.  The three launches do nothing unless the step
// launch before them left an update pending (PfChees::pending, set by workgroup 0 of the step launch, cleared by the scalar kernel).
#define PF_CHAIN_METRIC_TU
#include "hmc_kernel.hip"

struct HmCheesArgs : HmArgs {
    PfChees *C;
    double *ua, *ux, *uxp, *uv;        // the update's inputs: a [K]; x, x', u' [K][d] (slot 0)
    int32_t *nl;                       // L_t of the call's transitions
    int64_t *h_status;                 // page-locked progress word
    int64_t pround, tcall;             // the number this launch publishes; the call's first transition
    int64_t nrec;                      // > 1: update t's vectors go to slot t (PFMI_CHEES_RECORD_UPDATE)
    size_t vec;                        // K d
    int reopen;
};

template <int KPAD, bool RES>
__global__ __launch_bounds__(HM_NT) void pf_chees_step_kernel(HmCheesArgs A) { hm_step_body<KPAD, RES, HM_CHEES>(A); }

struct HmCheesFamily {
    static constexpr bool has_warm = false;
    template <int KPAD, bool RES, bool ADAPT>
    static auto kernel() { return &pf_chees_step_kernel<KPAD, RES>; }
};

struct CheesUpd {
    PfChees *C;
    int K, d;
    int64_t W, nrec;
    double *trace, *ua, *pqr, *xbar, *upd, *eps_out;
    size_t vec;
};

// the slot of update t's vectors
__device__ __forceinline__ const double *chees_slot(const CheesUpd &U, int which) {
    const size_t slot = U.nrec > 1 ? (size_t)U.C->t_upd : 0;
    return U.upd + ((size_t)which * (size_t)U.nrec + slot) * U.vec;
}

__global__ __launch_bounds__(256) void pf_chees_mean_kernel(CheesUpd U) {
    if (U.C->pending != 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= U.d) return;
    double xb, xbp;
    pf_chees_means(U.K, U.d, i, chees_slot(U, 0), chees_slot(U, 1), U.ua, &xb, &xbp);
    U.xbar[i] = xb; U.xbar[U.d + i] = xbp;
}

__global__ __launch_bounds__(256) void pf_chees_sums_kernel(CheesUpd U) {
    __shared__ double red[2 * 4 * 4];
    if (U.C->pending != 1) return;
    const int k = blockIdx.x, d = U.d;
    const size_t kd = (size_t)k * d;
    const double *x = chees_slot(U, 0) + kd, *xp = chees_slot(U, 1) + kd, *u = chees_slot(U, 2) + kd;
    const bool left_out = U.ua[k] == 0.0;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < d; i += 256) pf_chees_terms(x[i], xp[i], u[i], U.xbar[i], U.xbar[d + i], left_out, s[0], s[1], s[2]);
    int flip = 0;
    pf_block_sum_mv<4, 4>(s, red, flip);
    if (threadIdx.x == 0) { U.pqr[k] = s[0]; U.pqr[U.K + k] = s[1]; U.pqr[2 * U.K + k] = s[2]; }
}

__global__ __launch_bounds__(64) void pf_chees_scalar_kernel(CheesUpd U) {
    if (U.C->pending != 1) return;
    __shared__ double sEps;
    if (threadIdx.x == 0) {
        PfChees C = *U.C;
        const int64_t t = C.t_upd;
        const double tau = C.tau;
        double g, hm;
        pf_chees_scalars(C, U.K, U.ua, U.pqr, pf_chees_halton(t), t + 1 >= U.W, &g, &hm);
        U.trace[t] = tau; U.trace[U.W + t] = g; U.trace[2 * U.W + t] = hm;
        C.pending = 0;
        *U.C = C;
        sEps = C.eps;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < U.K; k += 64) U.eps_out[k] = sEps;      // what pfmi_adapt_get reports as the chains' step size
}

static CheesUpd chees_upd(pfmi_ctx *c) {
    const HmcState &H = c->hmc;
    const CheesLayout Y(H.K, c->d, H.ch_W, H.ch_T, H.ch_nrec);
    double *b = c->hm_chees.as<double>();
    CheesUpd U;
    U.C = reinterpret_cast<PfChees *>(b);
    U.K = H.K; U.d = c->d; U.W = H.ch_W; U.nrec = H.ch_nrec;
    U.trace = b + Y.trace; U.ua = b + Y.ua; U.pqr = b + Y.pqr; U.xbar = b + Y.xbar; U.upd = b + Y.upd; U.eps_out = c->hm_eps.as<double>();
    U.vec = Y.vec;
    return U;
}

int32_t pf_launch_chees_step(pfmi_ctx *c, int64_t round, int64_t prow, bool reopen, hipStream_t s) {
    const HmcState &H = c->hmc;
    const CheesLayout Y(H.K, c->d, H.ch_W, H.ch_T, H.ch_nrec);
    double *b = c->hm_chees.as<double>();
    HmCheesArgs A;
    static_cast<HmArgs &>(A) = hm_args(c, prow);
    A.C = reinterpret_cast<PfChees *>(b);
    A.ua = b + Y.ua; A.ux = b + Y.upd; A.uxp = A.ux + Y.vec * (size_t)H.ch_nrec; A.uv = A.uxp + Y.vec * (size_t)H.ch_nrec;
    A.nl = reinterpret_cast<int32_t *>(b + Y.nl);
    A.h_status = c->nt_status;
    A.pround = round; A.tcall = H.t0 - H.ch_W; A.nrec = H.ch_nrec; A.vec = Y.vec;
    A.reopen = reopen ? 1 : 0;
    return hm_launch_step<HmCheesFamily>(c, "chees", A, s);
}

int32_t pf_launch_chees_update(pfmi_ctx *c, hipStream_t s) {
    const CheesUpd U = chees_upd(c);
    hipLaunchKernelGGL(pf_chees_mean_kernel, dim3((U.d + 255) / 256), dim3(256), 0, s, U);
    hipLaunchKernelGGL(pf_chees_sums_kernel, dim3(U.K), dim3(256), 0, s, U);
    hipLaunchKernelGGL(pf_chees_scalar_kernel, dim3(1), dim3(64), 0, s, U);
    PF_HIP(hipGetLastError());
    return PFMI_OK;
}
