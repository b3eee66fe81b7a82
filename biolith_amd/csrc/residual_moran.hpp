// residual_moran.hpp -- what bl_residual_moran (biolith_hip.hip) hands to its kernels (residual_moran.hip, a translation unit of its
// own: no existing kernel is recompiled next to it).
//
// The handle is one species' occu handle built WITH the observations: its sign-folded visit records (site_posterior.hpp) give the
// observations and the masks, the raw observation covariates (up on first use) give predict's detection probabilities.
//
// Four FIELDS per (draw, period): 0 the occupancy residual, 1 its replicate, 2 the site-level detection residual, 3 its replicate.
//
// Moran side, per chunk of draws.  CELL = (draw of the chunk, period), cells = (n1 - n0) T, waves = ceil(N / 64) runs of 64 sites:
//   val   [cell][site][4]           a site's four values, one 32-byte record: what the gather reads of a neighbour in one sector;
//                                   a site outside a field's mask holds NaN there (a value never is NaN: it is its own mask)
//   part1 [cell][wave][4][4]        per field the wave's sum of the masked values, their count, their max and their min
//   stat  [cell][4][2]              per field M (as a double: an integer below 2^31) and mu; mu = NaN where the field has no I
//                                   (M < 2, or every masked value equal)
//   part3 [cell][wave][4][3]        per field the wave's num, den and W
// val is the largest: 32 T N bytes a draw; run_over_draws cuts the draws so that it stays within 256 MB.
//
// Site side.  One thread per (period, site) over ALL the draws; no workspace, nothing per draw.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/biolith_hip.h"
#include "draw_coords.hpp"
#include "site_posterior.hpp"

constexpr int BL_RM_THREADS = 256;
constexpr int BL_RM_FIELDS = 4;
constexpr size_t BL_RM_VAL_BYTES = 8 * BL_RM_FIELDS; // of val, a (draw, period, site)

struct BlResidualMoranParams {
    const float *rows;       // the handle's rows: site covariates, then the visits' sign-folded records
    const float *wraw;       // raw observation covariates [T J][Ko][ns]
    int ns, N, T, J, Ks, Ko, D;
    BlSitePostBlock a;       // the visits' records, as bl_site_posterior is told them
    BlDrawCoords c;
    const float *draws;      // [n_draws][D], device: all of them
    int n_draws;
    int n0, n1;              // the chunk's draws (Moran side)
    unsigned long long seed, seed_rep;
    const int *nbr_ptr, *nbr_idx; // CSR, device
    const double *nbr_w;     // NULL = 1
    int n_waves;             // ceil(N / 64)
    double *val, *part1, *stat, *part3; // the workspace (above)
    double *moran_occ, *moran_det; // [n1 - n0][T][2], NULL = skip
    int *det_sites;          // [n1 - n0][T][2], NULL = skip
    double *occ_mean, *det_mean; // [T][N], NULL = skip
    int *n_occupied;         // [T][N], NULL = skip
};

// the four Moran kernels over the chunk's draws; the site kernel over all the draws
extern "C" int bl_launch_residual_moran(const BlResidualMoranParams *p, int grid_y, hipStream_t st);
extern "C" int bl_launch_residual_moran_site(const BlResidualMoranParams *p, hipStream_t st);
