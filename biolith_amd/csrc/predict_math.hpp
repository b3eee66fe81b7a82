// predict_math.hpp -- the arithmetic of the posterior predictive, written once for every kernel that states it: predict.hip (bl_predict,
// bl_predict_counts, bl_predict_scores, bl_deterministic), comb_predict.hip, predictive_check.hip and predictive_density.hip.  The last
// two promise bl_predict's replicate and bl_deterministic's psi and p bit for bit, and -ffp-contract=on fuses per source expression:
// they hold that promise by calling what bl_predict calls.  (The conditional posteriors' arithmetic is posterior_math.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include "draw_coords.hpp"
#include "pred_rng.hpp"

namespace {

__device__ __forceinline__ float pm_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

// b . (1, x), the intercept first; covariate k at x[k * stride] (1: staged in registers; n_stride: read from the rows at one site)
__device__ __forceinline__ float pm_linear(const float *__restrict__ x, size_t stride, const float *__restrict__ b, int K)
{
    float s = b[0];
    for (int k = 0; k < K; k++) s = fmaf(x[k * stride], b[k + 1], s);
    return s;
}
// the site predictor eta of site i under draw th: beta . (1, x) and the site's occupancy / abundance effect
__device__ __forceinline__ float pm_site_eta(const float *__restrict__ x, size_t stride, const float *__restrict__ th, int Ks,
                                             const BlDrawCoords &c, int i)
{
    float eta = pm_linear(x, stride, th, Ks);
    if (c.o_u >= 0) eta += th[c.o_u + i];
    return eta;
}
// alpha . (1, w) of visit v at site i, w the raw covariates [visits][Ko][ns]
__device__ __forceinline__ float pm_visit_linear(const float *__restrict__ wraw, int ns, const float *__restrict__ al, int Ko, int v, int i)
{
    return pm_linear(wraw + ((size_t)v * Ko * ns + i), ns, al, Ko);
}
// the visit predictor nu of visit v = t J + j at site i: alpha . (1, w), the site's detection effect and the visit's effect
__device__ __forceinline__ float pm_visit_nu(const float *__restrict__ wraw, int ns, const float *__restrict__ th, const float *__restrict__ al,
                                             int Ko, const BlDrawCoords &c, int T, int J, int v, int i)
{
    float nu = pm_visit_linear(wraw, ns, al, Ko, v, i);
    if (c.o_v >= 0) nu += th[c.o_v + i];
    if (c.o_e >= 0) nu += th[c.o_e + (size_t)i * T * J + v];
    return nu;
}
// a detection probability pd under false positives: f_c acts on every site, f_u on unoccupied ones (ONE expression: it contracts as one)
__device__ __forceinline__ float pm_false_positives(float pd, float f_c, float f_u, int zn)
{
    return 1.0f - (1.0f - pd) * (1.0f - f_c) * (1.0f - (zn ? 0.0f : f_u));
}
// z ~ Bernoulli(psi): one uniform
__device__ __forceinline__ int pm_draw_z(BlPredRng &rng, float psi) { return rng.uniform() < psi ? 1 : 0; }
// N ~ Poisson(exp(eta)) restricted to 0 .. K: inversion over the renormalised pmf, float64 recursion p_n = p_{n-1} lambda / n; one uniform
__device__ __forceinline__ int pm_draw_abundance(BlPredRng &rng, float eta, int K)
{
    const double lam = exp((double)eta);
    double p = exp(-lam), tot = 0.0;
    for (int m = 0; m <= K; m++) { tot += p; p *= lam / (double)(m + 1); }
    const double target = (double)rng.uniform() * tot;
    p = exp(-lam);
    double cum = 0.0;
    for (int m = 0; m <= K; m++) {
        cum += p;
        if (target < cum) return m;
        p *= lam / (double)(m + 1);
    }
    return K;
}
// a standard normal by Box-Muller: two uniforms, the first floored at 2^-24
__device__ __forceinline__ float pm_normal(BlPredRng &rng)
{
    const float u1 = fmaxf(rng.uniform(), 5.9604645e-08f), u2 = rng.uniform();
    return sqrtf(-2.0f * __logf(u1)) * __cosf(6.2831853f * u2);
}

} // namespace
