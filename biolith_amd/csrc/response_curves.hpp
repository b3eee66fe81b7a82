// response_curves.hpp -- what bl_response_curves (biolith_hip.hip) hands to its kernels (response_curves.hip, a translation unit of its
// own: no existing kernel is recompiled next to it).
//
// One thread per site, the sites in site order padded with idle lanes to a whole number of 64-lane waves: wave r serves run r of
// bl_regional_totals' order for a single region.  The main kernel writes one float64 partial per (run, draw of the chunk, value) -- the
// workspace, `part`, RUN-MAJOR: part[(r * (n1 - n0) + dn) * n_values + g] --, so that the finish kernel's threads, one per (draw, value),
// read neighbouring words of a run at every step of their loop over the runs.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/biolith_hip.h"
#include "draw_coords.hpp"

constexpr int BL_RC_THREADS = 256, BL_RC_FINISH_THREADS = 64;
// the block of values a lane holds at a time.  Obs side: a visit's covariates are loaded once per block and the block's float64 sums
// over the visits live in registers.  Site side: the block's terms are reduced over the wave together (response_curves.hip:
// rc_block_sum).  A power of two, at most 64.  (Measured at 4, 8 and 16: profiles/NOTES.md.)
#ifndef BL_RC_VALUE_BLOCK
#define BL_RC_VALUE_BLOCK 8
#endif

struct BlResponseCurvesParams {
    const float *rows;       // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    const float *wraw;       // the raw observation covariates [T J][Ko][ns] (the obs side)
    int ns, N, T, J, Ks, Ko, D;
    int model;               // the plain model whose branch the handle runs, as BlPredictParams::model
    BlDrawCoords c;
    const float *draws;      // [n_draws][D], device: all of them
    int n0, n1;              // the chunk's draws
    int side, k;             // 0 site, 1 obs; the covariate that is replaced
    int n_values;
    const float *values;     // [n_values], device
    const double *weight;    // [N], device; NULL = 1
    int n_runs;              // ceil(N / 64)
    double *part;            // [n_runs][n1 - n0][n_values]: the workspace
    double *total;           // [n1 - n0][n_values]
};

extern "C" int bl_launch_response_curves(const BlResponseCurvesParams *p, int grid_y, hipStream_t st);
