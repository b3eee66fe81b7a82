// site_posterior.hpp -- what bl_site_posterior (biolith_hip.hip) hands to its kernel (site_posterior.hip, a translation unit of
// its own: no existing kernel is recompiled next to it).
//
// The kernel reads the sign-folded rows the density kernels read (occu_device.hpp / re_kernel.hpp): a visit's record is
// (c, c w_1 .. c w_K), c = +1 detection / -1 non-detection / 0 masked, so the rows carry the observations and nothing is uploaded.
#pragma once
#include <hip/hip_runtime.h>

#include "draw_coords.hpp"

// one block of visits: first row, replicates per period, covariates, rows per visit, where its K + 1 coefficients start in a draw
struct BlSitePostBlock {
    int r0, J, K, vw, o_al;
};
struct BlSitePostParams {
    const float *rows;        // [n_rows][ns], site-fastest; rows 0 .. Ks - 1 = the site covariates
    int ns, N, T, Ks, D;
    BlSitePostBlock a;        // occu: the visits; occu_comb: the point counts (no false positives)
    BlSitePostBlock b;        // occu_comb: the ARU visits (J = 0 otherwise)
    int comb;                 // 1 = occu_comb: block b, six rows per period from r_per, the six trailing coordinates from o_x
    int r_per, o_x;
    BlDrawCoords c;           // occu: the false-positive rate (phi = logit(rate)) and the random effects in a draw
    const float *draws;       // [n_draws][D], device
    int n0, n1;               // the draws of this launch; outputs are indexed from n0
    unsigned long long seed;
    float *log_lik, *z_prob;  // [n1 - n0][T][N], device, NULL = skip
    unsigned char *z;
};

extern "C" int bl_launch_site_posterior(const BlSitePostParams *p, int grid_y, hipStream_t st);
