// trajectory_totals.hpp -- what bl_trajectory_totals (biolith_hip.hip) hands to its kernels (trajectory_totals.hip, a translation unit of
// its own: no existing kernel is recompiled next to it).
//
// The layout is regional_totals.hpp's: the host lays the sites out in SLOTS, the site indices stable-sorted by region, every region
// padded with idle slots (-1) to a whole number of 64-lane waves, so wave w of the slots serves exactly one region and
// wave_first[g] .. wave_first[g + 1] - 1 are region g's waves in site order.  The main kernel writes one float64 partial per (draw of the
// chunk, output row, wave) -- the workspace, `part`, wave-major here: a grid in one region has 15 625 partials a total, and the finish
// kernel's lanes read neighbouring doubles --, the finish kernel adds a region's partials in wave order.
//
// Output rows of a draw: the wanted outputs one after the other in the order of BlTrajectoryOutput, T rows for a per-period output,
// T - 1 for a per-pair output, one for the equilibrium.  row_first[k] is output k's first row, row_first[k + 1] - row_first[k] its
// number of rows (0: not wanted, or T = 1 for a per-pair output), row_first[BL_TT_OUTPUTS] the rows of a draw.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/biolith_hip.h"

constexpr int BL_TT_THREADS = 256;
constexpr int BL_TT_FINISH_THREADS = 64;
constexpr int BL_TT_MAX_KS = 8; // the site covariates an occu_dyn handle takes (BL_DYN_MAX_KS)

enum BlTrajectoryOutput { BL_TT_OCC = 0, BL_TT_COL, BL_TT_EXT, BL_TT_EQ, BL_TT_Z, BL_TT_ZCOL, BL_TT_ZEXT, BL_TT_OUTPUTS };

struct BlTrajectoryTotalsParams {
    const float *rows;       // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    int ns, N, T, Ks, D;     // T is the call's, not the handle's
    unsigned long long seed;
    const float *draws;      // [n_draws][D], device: [b_psi | b_col | b_ext (Ks + 1 each) | alpha]
    int n0, n1;              // the chunk's draws
    const int *slot_site;    // [n_slots]: the site of the slot, -1 = idle
    const double *slot_w;    // [n_slots]: its weight (idle: unread), NULL = 1
    const int *wave_first;   // [n_regions + 1]: the first wave of every region
    int n_slots, n_waves, n_regions; // n_slots = 64 n_waves
    int row_first[BL_TT_OUTPUTS + 1];
    double *part;            // [n_waves][n1 - n0][rows]: the workspace, wave-major (the finish kernel's reads are coalesced)
    double *out[BL_TT_OUTPUTS]; // [n1 - n0][rows of the output][n_regions], NULL = skip
};

extern "C" int bl_launch_trajectory_totals(const BlTrajectoryTotalsParams *p, int grid_y, hipStream_t st);
