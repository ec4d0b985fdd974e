// pool_geometry.h -- what the passes over the pool share.  pool_moments_kernels.hip and pool_cdf_kernels.hip take the cut of a run
// into workgroups (mom_geometry), the place of a thread in its workgroup (pool_lane) and the walk over a slot's columns (pool_walk)
// from here; pool_cross_kernels.hip, which stages tiles for the matrix cores instead, takes the weight rule (pool_weight, pool_counts) and, like
// the other two, the window of the PSIS weights a col_offset addresses (pf_pool_weights).
//
// A workgroup is MOM_THREADS threads = MOM_WAVES waves and owns a tile of rows and a chunk of L consecutive columns of one run; grid =
// (row tiles, chunks, K).  Its threads form NS column SLOTS: slot s takes the columns n0 + s, n0 + s + NS, ... of the chunk and keeps
// its results in registers.  The slots are combined in slot order, the chunks in chunk order: (NS, L) fix the order in which the terms
// of one row are added.
//   d >= 64   lanes run along rows: a wave reads 64 V consecutive doubles of a column per load.  V = 2 (16-byte loads) needs an even d:
//             a column starts at byte 8 d s, so paired loads are aligned exactly when d is even (and the pair of an in-range even row is
//             in range); mom_geometry asks for it from d = 128, a kernel may still decline it.  The 4 waves are RW = 4 / NS row waves
//             x NS column slots.
//   d <  64   a wave holds G = 64 / d whole columns: lane = g d + i reads row i of column slot (wave G + g); NS = 4 G.  G d of the 64
//             lanes work (more than half for every d), and the wave's loads are G d consecutive doubles.
// Every thread issues MOM_BYTES_IN_FLIGHT / (8 V) independent loads before it consumes the first.
#pragma once
#include "pfmi_common.h"

#define MOM_THREADS 256
#define MOM_WAVES 4
#define MOM_BYTES_IN_FLIGHT 64      // per lane
#define MOM_WG_PER_RUN 64           // row tiles x chunks aimed at per run: 2 workgroups per CU at K = 8 on 256 CUs
#define MOM_MIN_COLS_PER_SLOT 8     // a chunk is never cut shorter than this many columns per slot

struct MomGeom {
    int V, RW, NS, G, rows_per_wg, row_tiles;
    int64_t L, C;                   // chunk length (columns), chunks per run
};

// the ONE statement of the geometry: (d, N_r) only (wg_per_run is a constant of the calling kernel file)
static inline MomGeom mom_geometry(int d, int64_t N_r, int wg_per_run = MOM_WG_PER_RUN) {
    MomGeom g;
    if (d >= 64) {
        g.V = (d % 2 == 0 && d >= 128) ? 2 : 1;
        const int nrw = (d + 64 * g.V - 1) / (64 * g.V);          // waves one column needs
        g.RW = nrw >= 4 ? 4 : nrw >= 2 ? 2 : 1;
        g.NS = MOM_WAVES / g.RW;
        g.G = 0;
        g.rows_per_wg = g.RW * 64 * g.V;
    } else {
        g.V = 1;
        g.RW = 1;
        g.G = 64 / d;
        g.NS = MOM_WAVES * g.G;
        g.rows_per_wg = d;
    }
    g.row_tiles = (d + g.rows_per_wg - 1) / g.rows_per_wg;
    const int64_t want = (wg_per_run + g.row_tiles - 1) / g.row_tiles;
    int64_t L = (N_r + want - 1) / want;
    const int64_t lmin = (int64_t)MOM_MIN_COLS_PER_SLOT * g.NS;
    if (L < lmin) L = lmin;
    if (L > N_r) L = N_r;
    g.L = L;
    g.C = (N_r + L - 1) / L;
    return g;
}

// grid = (row tiles, chunks, K): the y and z extents of one launch
static inline bool mom_grid_fits(int K, const MomGeom &g) { return K <= 65535 && g.C <= 65535; }

// the weights of the ctx's pool columns: entries [col_offset, col_offset + K N_r) of its PSIS weights (the GLOBAL pool's), run k at
// + k N_r; NULL without importance weighting
static inline const double *pf_pool_weights(const pfmi_ctx *c, int64_t col_offset, int importance) {
    return importance ? c->w.as<double>() + col_offset : nullptr;
}

// The weight rule, in its two steps.  imp: importance weighting is on; wk: the weights of one run (read only when imp); nc: an
// in-range column of the run.  pool_weight is the column's weight (1 without importance weighting); pool_counts says whether a column
// the caller owns (use) counts: a zero weight skips the column whatever it holds -- the caller SELECTS on the result, it never
// multiplies by the 0 (0 * NaN) -- and without importance weighting nothing is skipped.  (w by reference: by value the cross kernel,
// whose instructions are otherwise those of the open-coded rule, comes out with another block layout.)
__device__ __forceinline__ double pool_weight(bool imp, const double *wk, int64_t nc) { return imp ? wk[nc] : 1.0; }
__device__ __forceinline__ bool pool_counts(bool imp, bool use, const double &w) { return use && !(imp && w == 0.0); }

// the place of a thread (of the first MOM_THREADS, or of a repeat of them) in its workgroup: its column slot, its first row within the
// row tile and in the pool, and whether it holds rows at all
struct PoolLane {
    int slot, rloc, rows_per_wg, row;
    bool active;
};

template <int V>
__device__ __forceinline__ PoolLane pool_lane(int d, int G, int NS) {
    const int tid = threadIdx.x % MOM_THREADS, wave = tid >> 6, lane = tid & 63;
    PoolLane p;
    if (G == 0) {                      // d >= 64: lanes along rows
        const int RW = MOM_WAVES / NS, rw = wave % RW;
        p.slot = wave / RW;
        p.rloc = (rw * 64 + lane) * V;
        p.rows_per_wg = RW * 64 * V;
        p.active = (int64_t)blockIdx.x * p.rows_per_wg + p.rloc < d;    // (V = 2: d is even, so the pair is inside too)
    } else {                           // d < 64: G whole columns per wave
        const int g = lane / d;
        p.slot = wave * G + g;
        p.rloc = lane - g * d;
        p.rows_per_wg = d;
        p.active = g < G;
    }
    p.row = blockIdx.x * p.rows_per_wg + p.rloc;
    return p;
}

// The walk of an active thread over its slot's columns n_begin, n_begin + NS, ... < n1 of one run.  col: the thread's first row of
// the run's column 0 (column n: col + n d); wk: the run's weights or NULL.  body(const double (&x)[V], double w, bool on) is called
// once per column, in column order, with the thread's V rows of it, its weight and whether it counts (pool_counts); the columns past
// n1 that complete the last trip arrive with on = false (x and w of an in-range column).
template <int V, typename Body>
__device__ __forceinline__ void pool_walk(const double *col, const double *wk, int d, int64_t n_begin, int64_t n1, int NS, Body &&body) {
    constexpr int U = MOM_BYTES_IN_FLIGHT / (8 * V);
    const bool imp = wk != nullptr;
    for (int64_t n = n_begin; n < n1; n += (int64_t)U * NS) {
        double x[U][V], w[U];
        bool use[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {                               // every load of the trip is issued before the first use
            const int64_t nu = n + (int64_t)u * NS;
            use[u] = nu < n1;
            const int64_t nc = use[u] ? nu : n;                     // (clamped: an in-range column)
            if constexpr (V == 2) {
                const double2 t = *reinterpret_cast<const double2 *>(col + (size_t)nc * d);
                x[u][0] = t.x; x[u][V - 1] = t.y;
            } else {
                x[u][0] = col[(size_t)nc * d];
            }
            w[u] = pool_weight(imp, wk, nc);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) body(x[u], w[u], pool_counts(imp, use[u], w[u]));      // (the predicate waits for its own load only)
    }
}
