// hmc_rows.h -- what the chain kernels (hmc_kernel.hip: static HMC, nuts_kernel.hip: NUTS) share: the momentum normals and the two
// per-row products of the Woodbury passes.
#pragma once
#include "pfmi_common.h"

#ifdef __HIPCC__
// the standard normal of row i of draw n under `seed`: the value pf_randn4(seed, i / 4, n, stream 0) gives row i (full table in global
// memory: the same values as the LDS copy's)
__device__ __forceinline__ double hm_normal(uint64_t seed, uint32_t n, int i) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), g = (uint32_t)i >> 2, q = (uint32_t)i & 3u;
    uint32_t x[4];
    pf_philox_normals(n, g, 0u, 0u, k0, k1, x);
    const uint32_t xw = q == 0 ? x[0] : q == 1 ? x[1] : q == 2 ? x[2] : x[3];
    uint32_t x2w = 0u;
    if ((xw & 0x7FFFFFFFu) < (1u << PF_ICDF_TAILBITS)) {
        uint32_t x2[4];
        pf_philox_normals(n, g, 0u, 1u, k0, k1, x2);
        x2w = q == 0 ? x2[0] : q == 1 ? x2[1] : q == 2 ? x2[2] : x2[3];
    }
    return pf_icdf_any(xw, x2w);
}

// w[j] += row[j] z and y - row . tv, KPAD columns in groups of 4 (one 32-byte load each)
template <int KPAD, int NV, bool KEEP>
__device__ __forceinline__ void hm_row_axpy(const double *row, double *keep, double z, double (&w)[NV]) {
#pragma unroll
    for (int c = 0; c < KPAD; c += 4) {
        const double4 r = *reinterpret_cast<const double4 *>(row + c);
        if (KEEP) *reinterpret_cast<double4 *>(keep + c) = r;           // the thread's own LDS copy of the row, for the later passes
        w[c] = fma(r.x, z, w[c]); w[c + 1] = fma(r.y, z, w[c + 1]); w[c + 2] = fma(r.z, z, w[c + 2]); w[c + 3] = fma(r.w, z, w[c + 3]);
    }
}
template <int KPAD>
__device__ __forceinline__ double hm_row_sub(const double *row, const double *tv, double y) {
#pragma unroll
    for (int c = 0; c < KPAD; c += 4) {
        const double4 r = *reinterpret_cast<const double4 *>(row + c);
        y = fma(-r.x, tv[c], y); y = fma(-r.y, tv[c + 1], y); y = fma(-r.z, tv[c + 2], y); y = fma(-r.w, tv[c + 3], y);
    }
    return y;
}
#endif
