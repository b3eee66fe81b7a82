// comb_predict.hpp -- what bl_predict_comb and bl_deterministic_comb (biolith_hip.hip) hand to their kernels (comb_predict.hip, a
// translation unit of its own: no existing kernel is recompiled next to it).
//
// occu_comb's density rows are sign-folded by the observation (c w, c = 0 where masked), so with the observations withheld they carry
// no covariates: the kernels read the raw, NaN -> 0 covariates of the two detection blocks, kept on the host at creation and sent up on
// first use, and the site covariates from the head of the handle's rows.
#pragma once
#include <hip/hip_runtime.h>

// one block of visits: replicates per period, covariates, where its K + 1 coefficients start in a draw, its raw covariates
struct BlCombPredBlock {
    int J, K, o_al;
    const float *w;           // [T J][K][ns], site-fastest, NaN -> 0
};
struct BlCombPredParams {
    const float *rows;        // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    int ns, N, T, Ks, D;
    BlCombPredBlock pc, aru;  // the point counts (no false positives), the ARU visits
    int Js;                   // scores per period
    int o_x;                  // the six trailing coordinates: logit fc, logit fu, mu0, log(mu1 - mu0), log sigma0, log sigma1
    const float *draws;       // [n_draws][D], device
    int n0, n1;               // the draws of this launch; outputs are indexed from n0
    unsigned long long seed;
    // bl_predict_comb (device, NULL = skip)
    unsigned char *z;         // [n1 - n0][T][N]
    unsigned char *y_pc;      // [n1 - n0][Jpc][T][N]
    unsigned char *y_aru;     // [n1 - n0][Jaru][T][N]
    float *scores;            // [n1 - n0][Js][T][N]
    // bl_deterministic_comb (device, NULL = skip)
    float *psi;               // [n1 - n0][T][N]
    float *pc_prob;           // [n1 - n0][Jpc][T][N]
    float *aru_prob;          // [n1 - n0][Jaru][T][N]
};

extern "C" int bl_launch_comb_predict(const BlCombPredParams *p, int grid_y, hipStream_t st);
extern "C" int bl_launch_comb_deterministic(const BlCombPredParams *p, int grid_y, hipStream_t st);
