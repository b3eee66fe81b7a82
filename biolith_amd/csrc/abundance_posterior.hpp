// abundance_posterior.hpp -- what bl_abundance_posterior (biolith_hip.hip) hands to its kernel (abundance_posterior.hip, a translation
// unit of its own: no existing kernel is recompiled next to it).
//
// The kernel reads the rows the samplers read (occu_device.hpp / re_kernel.hpp) and nothing else is uploaded:
//   occu_rn   a visit's record is (c, c w_1 .. c w_Ko, spare), c = +1 detection / -1 non-detection / 0 masked;
//   nmixture  a visit's record is (m y, m, w_1 .. w_Ko), m = 1 unmasked / 0 masked; per period one row with the cell's largest count
//             and one with its number of unmasked visits; the table tab[t][n][site] = sum_j m log C(n, y_j).
#pragma once
#include <hip/hip_runtime.h>

#include "draw_coords.hpp"

struct BlAbundPostParams {
    const float *rows;        // [n_rows][ns], site-fastest; rows 0 .. Ks - 1 = the site covariates
    const float *tab;         // nmixture: [T][K + 1][ns]; NULL for occu_rn
    int ns, N, T, J, Ks, Ko, D;
    int r0, vw;               // first visit row, rows per visit
    int r_ymax;               // nmixture: row of period 0's largest count (period t: row r_ymax + t)
    int nmix;                 // 0 = occu_rn, 1 = nmixture
    int K;                    // max_abundance (< 128: the lgamma table)
    int o_al;                 // where the Ko + 1 detection coefficients start in a draw
    BlDrawCoords c;           // occu_rn: the false-positive rate (phi = logit(rate); the kernel asks o_fp alone), the random effects
    const float *draws;       // [n_draws][D], device
    int n0, n1;               // the draws of this launch; outputs are indexed from n0
    unsigned long long seed;
    float *log_lik, *n_mean, *occ_prob; // [n1 - n0][T][N], device, NULL = skip
    int *n_draw;
};

extern "C" int bl_launch_abundance_posterior(const BlAbundPostParams *p, int grid_y, hipStream_t st);
