// psis_loo.hpp -- what bl_psis_loo (biolith_hip.hip) hands to its kernels (psis_loo.hip, a translation unit of its own: no existing
// kernel is recompiled next to it).
//
// The kernels know no model: they read a chunk of the (draws, cells) log-likelihood matrix that the conditional posteriors return, as
// it lies on the host -- [n][cells], cell-fastest -- and write three doubles per cell.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/biolith_hip.h"

constexpr int BL_PSIS_TILE = 32;      // the transpose's LDS tile: 32 x 32 floats, rows padded by one
constexpr int BL_PSIS_TAIL_MAX = 272; // ceil(3 sqrt(BL_PSIS_MAX_DRAWS)): the longest tail M, and the size of the kernel's tail arrays
constexpr int BL_PSIS_CAND_MAX = 64;  // candidates of the generalised-Pareto fit, a lane each: 30 + floor(sqrt(M')) <= 46
static_assert((long long)BL_PSIS_TAIL_MAX * BL_PSIS_TAIL_MAX >= 9LL * BL_PSIS_MAX_DRAWS, "the tail arrays hold ceil(3 sqrt(n)) draws");
static_assert(30 + 17 <= BL_PSIS_CAND_MAX && 17 * 17 > BL_PSIS_TAIL_MAX, "one lane per candidate");

struct BlPsisParams {
    int n;            // draws, 2 .. BL_PSIS_MAX_DRAWS
    int cells;        // cells of this launch
    int tail;         // M = ceil(min(n / 5, 3 sqrt(n))) <= BL_PSIS_TAIL_MAX, computed once on the host
    const float *in;  // [n][cells], device: the chunk as uploaded
    float *cols;      // [cells][n], device: its transpose, a cell's draws contiguous
    double *out;      // [3][cells], device: elpd, pareto_k, lppd
};

extern "C" int bl_launch_psis_loo(const BlPsisParams *p, hipStream_t st);
