// predictive_check.hpp -- what bl_predictive_check (biolith_hip.hip) hands to its kernels (predictive_check.hip, a translation unit of
// its own: no existing kernel is recompiled next to it).
//
// The kernels read what bl_predict and bl_deterministic read -- the site covariates at the head of the handle's rows and the raw,
// NaN -> 0 observation covariates -- and the observations the caller passes: the handle's sign-folded rows fold the covariate masks
// into theirs, the host check masks by the observation alone.
#pragma once
#include <hip/hip_runtime.h>

#include "draw_coords.hpp"

constexpr int BL_PC_THREADS = 256; // sites per block: four wave64

struct BlPredCheckParams {
    const float *rows;         // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    const float *wraw;         // [T J][Ko][ns], site-fastest, NaN -> 0
    int ns, N, T, J, Ks, Ko, D;
    BlDrawCoords c;            // the false-positive rate (phi = logit(rate)) and the random effects in a draw
    const float *draws;        // [n_draws][D], device
    int n0, n1;                // the draws of this launch; partials and results are indexed from n0
    unsigned long long seed;
    const unsigned char *obs;  // [J][T][N], device: 0, 1, 255 = not observed
    const int *obs_visit;      // [T J], device: the observed detections of revisit (t, j) over its seen sites
    int n_blocks;              // site blocks = gridDim.x of the first kernel
    // the first kernel's partials (device workspace), one per (draw, site block)
    double *site_part;         // [n1 - n0][n_blocks][4]: ft_obs, ft_rep, chi_obs, chi_rep over the block's sites; NULL = skip
    double *visit_exp;         // [n1 - n0][n_blocks][T J]: sum of E over the block's seen sites; NULL = skip (with visit_rep)
    int *visit_rep;            // [n1 - n0][n_blocks][T J]: the replicate's detections over the block's seen sites
    // the second kernel's results (device)
    double *by_site;           // [n1 - n0][4], NULL = skip
    double *by_revisit;        // [n1 - n0][4], NULL = skip
};

extern "C" int bl_launch_predictive_check(const BlPredCheckParams *p, int grid_y, hipStream_t st);
