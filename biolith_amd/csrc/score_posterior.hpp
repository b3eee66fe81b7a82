// score_posterior.hpp -- what bl_score_posterior (biolith_hip.hip) hands to its kernel (score_posterior.hip, a translation unit of
// its own: no existing kernel is recompiled next to it).
//
// The kernel reads what the occu_cs handle already holds: the site-covariate rows and each visit's mask c (1 = the visit has a score
// and all its covariates, 0 = masked) from the sampler's rows, the scores (0 where masked) from the handle's score rows, and the raw
// NaN -> 0 observation covariates (a masked visit still has a detection probability).  Nothing is uploaded per call.
#pragma once
#include <hip/hip_runtime.h>

struct BlScorePostParams {
    const float *rows;        // [n_rows][ns], site-fastest; rows 0 .. Ks - 1 = the site covariates, a visit's mask at row r0 + v * vw
    const float *wraw;        // [T J][Ko][ns]: the observation covariates, NaN -> 0
    const float *scores;      // [T J][ns]: the scores, 0 where masked
    int ns, N, T, J, Ks, Ko, D;
    int r0, vw;
    const float *draws;       // [n_draws][D], device: [beta | alpha | mu0 | log(mu1 - mu0) | log sigma0 | log sigma1]
    int n0, n1;               // the draws of this launch; outputs are indexed from n0
    unsigned long long seed;
    float *log_lik, *z_prob;  // [n1 - n0][T][N], device, NULL = skip
    unsigned char *z;
    float *f_prob;            // [n1 - n0][J][T][N], device, NULL = skip
    unsigned char *f;
};

extern "C" int bl_launch_score_posterior(const BlScorePostParams *p, int grid_y, hipStream_t st);
