// species_richness.hpp -- what bl_species_richness (biolith_hip.hip) hands to its kernels (species_richness.hip, a translation unit of
// its own: no existing kernel is recompiled next to it).
//
// The draws are stacked: draw n holds n_species coefficient blocks of the handle's D coordinates each, species s at
// draws[(n * S + s) * D].  The handle is one species'; its site covariates are every species'.
//
// Area side.  The layout is regional_totals.hpp's: the host lays the sites out in SLOTS, the site indices stable-sorted by region, every
// region padded with idle slots (-1) to a whole number of 64-lane waves, so wave w of the slots serves exactly one region and
// wave_first[g] .. wave_first[g + 1] - 1 are region g's waves in site order.  A draw has S + 1 output rows, row r the area with exactly r
// species.  The area kernel writes one float64 partial per (wave, draw of the chunk, row) -- the workspace, `part`, wave-major as
// trajectory_totals.hpp's: the finish kernel's lanes read neighbouring doubles --, the finish kernel adds a region's partials in wave
// order.
//
// Site side.  One thread per site over ALL the draws; no workspace, nothing per draw.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/biolith_hip.h"
#include "draw_coords.hpp"

constexpr int BL_SR_THREADS = 256;
constexpr int BL_SR_FINISH_THREADS = 64;
// What was measured against what is built (profiles/NOTES.md); a power of two up to 64, and 8, 16 or 32.
#ifndef BL_SR_ROW_BLOCK
#define BL_SR_ROW_BLOCK 4 // the rows the area kernel reduces at once (1: the plain tree a row)
#endif
#ifndef BL_SR_MIN_CLASS
#define BL_SR_MIN_CLASS 8 // the smallest capacity class a call is given (32: one class for every species count)
#endif

struct BlSpeciesRichnessParams {
    const float *rows;       // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    int ns, N, Ks, D;
    int S;                   // n_species, 1 .. BL_RICHNESS_MAX_SPECIES
    BlDrawCoords c;
    const float *draws;      // [n_draws][S][D], device: all of them
    int n_draws;
    int n0, n1;              // the chunk's draws (area side)
    const int *slot_site;    // [n_slots]: the site of the slot, -1 = idle
    const double *slot_w;    // [n_slots]: its weight (idle: unread), NULL = 1
    const int *wave_first;   // [n_regions + 1]: the first wave of every region
    int n_slots, n_waves, n_regions; // n_slots = 64 n_waves
    double *part;            // [n_waves][n1 - n0][S + 1]: the workspace
    double *area_total;      // [n1 - n0][S + 1][n_regions]
    double *pmf;             // [N][S + 1], NULL = skip
    double *mean, *sd;       // [N], NULL = skip
};

// the area kernel and its finish kernel over the chunk's draws; the site kernel over all the draws
extern "C" int bl_launch_species_richness_area(const BlSpeciesRichnessParams *p, int grid_y, hipStream_t st);
extern "C" int bl_launch_species_richness_site(const BlSpeciesRichnessParams *p, hipStream_t st);
