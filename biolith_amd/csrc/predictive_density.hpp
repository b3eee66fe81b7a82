// predictive_density.hpp -- what bl_predictive_density (biolith_hip.hip) hands to its kernels (predictive_density.hip, a translation
// unit of its own: no existing kernel is recompiled next to it).
//
// The kernels read what bl_predict and bl_deterministic read -- the site covariates at the head of the handle's rows and the raw,
// NaN -> 0 observation covariates -- and the observations the caller passes, into which the caller has folded every mask (255 = not a
// point).  Two reductions of the same pointwise log-likelihood ll(draw, visit, site): over the points per draw, and over the draws per
// point.
#pragma once
#include <hip/hip_runtime.h>

#include "draw_coords.hpp"

constexpr int BL_PD_THREADS = 256;    // threads per block of both main kernels: four wave64
constexpr int BL_PD_MAX_STRIPS = 64;  // the cap of the point kernel's strips of draws (grid.y); it does not depend on the draw count
constexpr int BL_PD_FILL = 256 * 2048; // threads that fill the device: the strip count is chosen so that cells * strips reaches it

struct BlPredDensityParams {
    const float *rows;         // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    const float *wraw;         // [T J][Ko][ns], site-fastest, NaN -> 0
    int ns, N, T, J, Ks, Ko, D;
    BlDrawCoords c;            // the false-positive rate (phi = logit(rate)) and the random effects in a draw
    const float *draws;        // [n_draws][D], device: all of them
    int n_draws;
    int n0, n1;                // the draws of one launch of the per-draw kernel; its partials and results are indexed from n0
    unsigned long long seed;
    const unsigned char *obs;  // [J][T][N], device: 0, 1, 255 = not a point
    int marginal;              // 0: the conditional form at predict()'s z; 1: the marginal form psi * r (no generator)
    // per draw: the sum of ll over the points
    int n_blocks;              // site blocks = gridDim.x of the per-draw kernel
    double *draw_part;         // [n1 - n0][n_blocks], device workspace
    double *per_draw;          // [n1 - n0], device
    // per point: log mean exp and variance of ll over the draws
    int strips;                // gridDim.y of the point kernel: strip r walks the draws [bl_pd_strip_begin(r), bl_pd_strip_begin(r + 1))
    double *strip_part;        // [strips][4][J T N], device workspace: running maximum, scaled sum of exponentials, mean, M2
    double *point_lse;         // [J][T][N], device; NULL = skip
    double *point_var;         // [J][T][N], device; NULL = skip
};

// the draws are dealt to the strips in order, as evenly as they go: the first n % R strips take one more
__host__ __device__ inline int bl_pd_strip_begin(int n, int R, int r)
{
    const int base = n / R, rem = n % R;
    return r * base + (r < rem ? r : rem);
}

extern "C" int bl_launch_predictive_density_draws(const BlPredDensityParams *p, int grid_y, hipStream_t st);
extern "C" int bl_launch_predictive_density_points(const BlPredDensityParams *p, hipStream_t st);
