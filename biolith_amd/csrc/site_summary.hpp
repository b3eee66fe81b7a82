// site_summary.hpp -- what bl_site_summary (biolith_hip.hip) hands to its kernels (site_summary.hip, a translation unit of its own: no
// existing kernel is recompiled next to it).
//
// The kernels read what bl_deterministic's read -- the site covariates at the head of the handle's rows, the raw observation covariates
// -- and all the draws at once; they write per cell (a site, or (j, t, site) in bl_deterministic's order) and nothing per draw.
//
// The order statistics are found on the unsigned bit pattern of the float32 values.  Every served site is a sigmoid or an exponential,
// so every value is >= +0 and the bit pattern orders the values as the values order themselves (+inf, a saturated rate, included).  What
// follows: a NaN value has no place in that order, so NaN draws are not served -- the caller keeps non-finite draws out.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/biolith_hip.h"
#include "draw_coords.hpp"

constexpr int BL_SS_THREADS = 256;

struct BlSiteSummaryParams {
    const float *rows;   // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    const float *wraw;   // [T J][Ko][ns], site-fastest, NaN -> 0 (the second site only)
    int ns, N, T, J, Ks, Ko, D;
    int model;           // the plain model whose branch the handle runs, as BlPredictParams::model
    BlDrawCoords c;
    const float *draws;  // [n_draws][D], device: all of them
    int n_draws;
    int n_ranks;         // 0 .. BL_SUMMARY_MAX_RANKS; 0 = no order statistic
    int ranks[BL_SUMMARY_MAX_RANKS]; // each in 0 .. n_draws - 1, in the caller's order
    // device, NULL = skip; cells = N (the first site) or J T N (the second)
    double *mean, *sd;   // [cells]
    float *order;        // [n_ranks][cells]
};

extern "C" int bl_launch_site_summary_psi(const BlSiteSummaryParams *p, hipStream_t st);
extern "C" int bl_launch_site_summary_prob(const BlSiteSummaryParams *p, hipStream_t st);
