// path_posterior.hpp -- what bl_path_posterior (biolith_hip.hip) hands to its kernel (path_posterior.hip, a translation unit of its
// own: no existing kernel is recompiled next to it).
//
// The kernel reads the sign-folded rows the occu_dyn handle already holds (occu_device.hpp / dyn_device.hpp): a visit's record is
// (c, c w_1 .. c w_K), c = +1 detection / -1 non-detection / 0 masked, so the rows carry the observations and nothing is uploaded.
#pragma once
#include <hip/hip_runtime.h>

struct BlPathPostParams {
    const float *rows;        // [n_rows][ns], site-fastest; rows 0 .. Ks - 1 = the site covariates
    int ns, N, T, J, Ks, Ko, D;
    int r0, vw;               // first visit row, rows per visit; visit (t, j) starts at row r0 + (t J + j) vw
    const float *draws;       // [n_draws][D], device: [b_psi | b_col | b_ext (Ks + 1 each) | alpha (Ko + 1)]
    int n0, n1;               // the draws of this launch; outputs are indexed from n0
    unsigned long long seed;
    float *log_lik;           // [n1 - n0][N], device, NULL = skip
    float *z_prob;            // [n1 - n0][T][N], device, NEVER NULL: the forward pass keeps the filtered log-odds here, the backward
                              // pass overwrites them in place with the smoothed marginals
    float *col_prob, *ext_prob; // [n1 - n0][T - 1][N], device, NULL = skip
    unsigned char *z;         // [n1 - n0][T][N], device, NULL = skip
};

extern "C" int bl_launch_path_posterior(const BlPathPostParams *p, int grid_y, hipStream_t st);
