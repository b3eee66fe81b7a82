// regional_totals.hpp -- what bl_regional_totals (biolith_hip.hip) hands to its kernels (regional_totals.hip, a translation unit of its
// own: no existing kernel is recompiled next to it).
//
// The host lays the sites out in SLOTS: the site indices stable-sorted by region, every region padded with idle slots (-1) to a whole
// number of 64-lane waves.  Wave w of the slots therefore serves exactly one region, wave_first[g] .. wave_first[g + 1] - 1 are region
// g's waves in site order, and a region's layout is a function of its own sites alone.  A region costs at most 63 idle lanes, so one
// region per site is served, at one wave per site.
//
// The main kernel writes one float64 partial per (draw of the chunk, output row, wave) -- the workspace, `part` --, the finish kernel
// adds a region's partials in wave order.  Output rows of a draw: row 0 the first site's total (where wanted), then one row per period
// for the latent totals (where wanted).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/biolith_hip.h"
#include "draw_coords.hpp"

constexpr int BL_RT_THREADS = 256;

struct BlRegionalTotalsParams {
    const float *rows;       // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    int ns, N, T, Ks, D;
    int model;               // the plain model whose branch the handle runs, as BlPredictParams::model
    int scores;              // occu_cs: its predict kernel draws z from the covariates' predictor alone
    int K;                   // max_abundance
    BlDrawCoords c;
    unsigned long long seed;
    const float *draws;      // [n_draws][D], device: all of them
    int n0, n1;              // the chunk's draws
    const int *slot_site;    // [n_slots]: the site of the slot, -1 = idle
    const double *slot_w;    // [n_slots]: its weight (idle: unread), NULL = 1
    const int *wave_first;   // [n_regions + 1]: the first wave of every region
    int n_slots, n_waves, n_regions; // n_slots = 64 n_waves
    int site_rows, latent_rows;      // 1 or 0; T or 0
    double *part;            // [n1 - n0][site_rows + latent_rows][n_waves]: the workspace
    double *site_total;      // [n1 - n0][n_regions], NULL = skip
    double *latent_total;    // [n1 - n0][T][n_regions], NULL = skip
};

extern "C" int bl_launch_regional_totals(const BlRegionalTotalsParams *p, int grid_y, hipStream_t st);
