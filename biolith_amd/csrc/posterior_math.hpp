// posterior_math.hpp -- the arithmetic and the launch geometry the conditional-posterior kernels share (site_, abundance_, path_, score_
// and count_posterior.hip; comb_predict.hip takes the geometry).  Every expression is written once, here: -ffp-contract=on fuses per
// source expression, so a helper restated in another file is a chance of last-bit differences between kernels that state the same
// quantity.  The posterior predictive's arithmetic is stated the same way in predict_math.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "nuts_kernel.hpp"

namespace {

// log of float32's smallest normal, that normal, log of float32's epsilon (numpyro's probability clamp [tiny, 1 - eps])
constexpr float POST_LOG_TINY = -87.33654475f, POST_TINY = 1.1754944e-38f, POST_LOG_EPS = -15.9423847f;

// log(1 + e) for 0 <= e <= 1, relative error of a few ulps also where e is small (log(op) e / (op - 1): the rounding of 1 + e cancels)
__device__ __forceinline__ float post_log1p(float e)
{
    const float op = 1.0f + e, d = op - 1.0f;
    const float r = bl_log(op) * (e * bl_rcp(d));
    return d == 0.0f ? e : r;
}
struct PostSum { // Kahan
    float s = 0.0f, c = 0.0f;
    __device__ __forceinline__ void add(float x)
    {
        const float y = x - c, t = s + y;
        c = (t - s) - y;
        s = t;
    }
};
// f = sigmoid(x), g = sigmoid(-x): no complement is formed as 1 - f
__device__ __forceinline__ void post_sig(float x, float &f, float &g)
{
    const float e = bl_exp(-fabsf(x)), r = bl_rcp(1.0f + e);
    f = (x > 0.0f ? 1.0f : e) * r;
    g = (x > 0.0f ? e : 1.0f) * r;
}

// One thread per site, the draws on grid.y.  A small data set would idle three quarters of a 256-thread workgroup.
inline void post_geometry(int N, int grid_y, dim3 &grid, dim3 &block)
{
    const int nt = N < 256 ? 64 : 256;
    grid = dim3((N + nt - 1) / nt, grid_y);
    block = dim3(nt);
}

} // namespace
