// predict.hpp -- what bl_predict, bl_predict_counts, bl_predict_scores and bl_deterministic (biolith_hip.hip) hand to their kernels
// (predict.hip, a translation unit of its own: no sampler kernel is compiled next to them).
//
// The kernels read the site covariates at the head of the handle's rows and the raw, NaN -> 0 observation covariates (occu_cop: also the
// raw session durations), which go up on first use: with the observations withheld the sign-folded density rows carry no covariates.
#pragma once
#include <hip/hip_runtime.h>

#include "draw_coords.hpp"

struct BlPredictParams {
    const float *rows;        // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    const float *wraw;        // [T J][Ko][ns], site-fastest, NaN -> 0
    const float *dur;         // occu_cop: [T J][ns]
    int ns, N, T, J, Ks, Ko, D;
    int model;                // the plain model whose branch the handle runs: 0 occu, 1 occu_rn, 2 occu_fp, 3 occu_cop, 4 nmixture
    int K;                    // max_abundance (occu_rn, nmixture)
    BlDrawCoords c;
    const float *draws;       // [n_draws][D], device
    int n0, n1;               // the draws of this launch; outputs are indexed from n0
    unsigned long long seed;
    // device, NULL = skip; latent-level outputs are [n1 - n0][T][N], visit-level ones [n1 - n0][J][T][N]
    unsigned char *latent, *y;   // bl_predict: z (occu_rn: N), the detections
    int *count_latent, *count_y; // bl_predict_counts: z (nmixture: N), the counts
    unsigned char *f;            // bl_predict_scores (with latent): the true detections, the scores
    float *s;
    float *psi, *prob;           // bl_deterministic: psi (occu_rn, nmixture: the abundance rate), prob_detection (occu_cop: the rate)
};

extern "C" int bl_launch_predict(const BlPredictParams *p, int grid_y, hipStream_t st);
extern "C" int bl_launch_predict_counts(const BlPredictParams *p, int grid_y, hipStream_t st);
extern "C" int bl_launch_predict_scores(const BlPredictParams *p, int grid_y, hipStream_t st);
extern "C" int bl_launch_deterministic(const BlPredictParams *p, int grid_y, hipStream_t st); // a kernel per wanted output
