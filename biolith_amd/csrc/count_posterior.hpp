// count_posterior.hpp -- what bl_count_posterior (biolith_hip.hip) hands to its kernel (count_posterior.hip, a translation unit of
// its own: no existing kernel is recompiled next to it).
//
// The kernel reads the rows the occu_cop samplers read: the site covariates, each visit's (y_m, d_m, w_1 .. w_Ko) -- the count and the
// session duration, both 0 where the visit is masked, and its observation covariates (0 where masked) -- and the per-period Ysum / Dsum.
// One row is its own: the parameter-free part of a cell's log-likelihood, summed in float64 by the host when the handle is made.
#pragma once
#include <hip/hip_runtime.h>

#include "draw_coords.hpp"

struct BlCountPostParams {
    const float *rows;        // [n_rows][ns], site-fastest; rows 0 .. Ks - 1 = the site covariates, visit v at rows r0 + v * vw .. + vw - 1
    const float *ccell;       // [T][ns]: sum over the cell's unmasked visits of y log d - lgamma(y + 1)
    int ns, N, T, J, Ks, Ko, D;
    int r0, vw, r_sum;        // Ysum of period t at row r_sum + t, Dsum at row r_sum + T + t
    BlDrawCoords c;           // the false-positive rate (phi = log rate) and the random effects in a draw
    const float *draws;       // [n_draws][D], device: [beta | alpha | (phi) | (log sds) | (effects)]
    int n0, n1;               // the draws of this launch; outputs are indexed from n0
    unsigned long long seed;
    float *log_lik, *z_prob;  // [n1 - n0][T][N], device, NULL = skip
    unsigned char *z;
    float *true_mean;         // [n1 - n0][J][T][N], device, NULL = skip
    int *true_count;
};

extern "C" int bl_launch_count_posterior(const BlCountPostParams *p, int grid_y, hipStream_t st);
