// pool_geometry.h -- how the one-pass reductions over the pool (pool_moments_kernels.hip, pool_cdf_kernels.hip) cut a run into
// workgroups.  A workgroup is MOM_THREADS threads = MOM_WAVES waves and owns a tile of rows and a chunk of L consecutive columns of
// one run.  Its threads form NS column SLOTS: slot s takes the columns n0 + s, n0 + s + NS, ... of the chunk.  The slots are combined
// in slot order, the chunks in chunk order: (NS, L) fix the order in which the terms of one row are added.
#pragma once
#include <cstdint>

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
