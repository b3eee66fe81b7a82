// predictive_check_counts.hpp -- what bl_predictive_check_counts (biolith_hip.hip) hands to its kernels (predictive_check_counts.hip, a
// translation unit of its own: no existing kernel is recompiled next to it).
//
// The kernels read what bl_predict / bl_predict_counts and bl_deterministic read -- the site covariates at the head of the handle's
// rows, the raw, NaN -> 0 observation covariates, occu_cop's raw session durations -- and the observations the caller passes: the
// handle's rows fold the covariate masks into theirs, the check masks by the observation alone.
#pragma once
#include <hip/hip_runtime.h>

#include "draw_coords.hpp"

constexpr int BL_PCC_THREADS = 256; // sites per block: four wave64

struct BlPredCheckCountsParams {
    const float *rows;         // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    const float *wraw;         // [T J][Ko][ns], site-fastest, NaN -> 0
    const float *dur;          // occu_cop: [T J][ns]
    int ns, N, T, J, Ks, Ko, D;
    int model;                 // the plain model whose branch the handle runs: 1 occu_rn, 3 occu_cop, 4 nmixture
    int K;                     // max_abundance (occu_rn, nmixture), <= 127
    BlDrawCoords c;            // the false-positive rate (occu_rn: phi = logit(rate), occu_cop: log(rate)) and the random effects
    const float *draws;        // [n_draws][D], device
    int n0, n1;                // the draws of this launch; partials and results are indexed from n0
    unsigned long long seed;
    const int *obs;            // [J][T][N], device: the observed count, -1 = not observed
    const double *obs_visit;   // [T J], device: the observed total of revisit (t, j) over its seen sites
    int n_blocks;              // site blocks = gridDim.x of the first kernel
    // the first kernel's partials (device workspace), one per (draw, site block)
    double *site_part;         // [n1 - n0][n_blocks][4]: ft_obs, ft_rep, chi_obs, chi_rep over the block's sites; NULL = skip
    double *visit_exp;         // [n1 - n0][n_blocks][T J]: sum of E over the block's seen sites; NULL = skip (with visit_rep)
    double *visit_rep;         // [n1 - n0][n_blocks][T J]: the replicate's total over the block's seen sites (an integer: exact in any order)
    // the second kernel's results (device)
    double *by_site;           // [n1 - n0][4], NULL = skip
    double *by_revisit;        // [n1 - n0][4], NULL = skip
};

extern "C" int bl_launch_predictive_check_counts(const BlPredCheckCountsParams *p, int grid_y, hipStream_t st);
