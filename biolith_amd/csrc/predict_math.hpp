// predict_math.hpp -- the arithmetic of the posterior predictive, written once for every kernel that states it: predict.hip (bl_predict,
// bl_predict_counts, bl_predict_scores, bl_deterministic), comb_predict.hip, predictive_check.hip, predictive_check_counts.hip and
// predictive_density.hip, and site_summary.hip.  The last four promise bl_predict's / bl_predict_counts' replicate and bl_deterministic's
// sites bit for bit, and -ffp-contract=on fuses per source expression: they hold that promise by calling what the predict kernels call.  (The conditional
// posteriors' arithmetic is posterior_math.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include "draw_coords.hpp"
#include "pred_rng.hpp"

namespace {

// The reciprocal is the instruction itself, not `1.0f / d`: the build lets a float32 division be either that instruction or the correctly
// rounded sequence, and the compiler chose per call site (bl_predict_kernel's psi got the sequence, bl_psi_kernel's the instruction), so
// the threshold z is drawn against differed from the psi `deterministic` returns in the last bit of some cells.
__device__ __forceinline__ float pm_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

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
// what joins alpha . (1, w) of visit v = t J + j at site i: the site's detection effect and the visit's effect
__device__ __forceinline__ float pm_visit_effects(float nu, const float *__restrict__ th, const BlDrawCoords &c, int T, int J, int v, int i)
{
    if (c.o_v >= 0) nu += th[c.o_v + i];
    if (c.o_e >= 0) nu += th[c.o_e + (size_t)i * T * J + v];
    return nu;
}
// the visit predictor nu of visit v = t J + j at site i: alpha . (1, w) and the effects
__device__ __forceinline__ float pm_visit_nu(const float *__restrict__ wraw, int ns, const float *__restrict__ th, const float *__restrict__ al,
                                             int Ko, const BlDrawCoords &c, int T, int J, int v, int i)
{
    return pm_visit_effects(pm_visit_linear(wraw, ns, al, Ko, v, i), th, c, T, J, v, i);
}
// the same with the visit's covariates staged in registers, w[k] = wraw[(v Ko + k) ns + i]
__device__ __forceinline__ float pm_visit_nu_staged(const float *__restrict__ w, const float *__restrict__ th, const float *__restrict__ al,
                                                    int Ko, const BlDrawCoords &c, int T, int J, int v, int i)
{
    return pm_visit_effects(pm_linear(w, 1, al, Ko), th, c, T, J, v, i);
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
// Royle-Nichols: a visit's detection probability 1 - (1 - r)^N among N individuals, then its constant false-positive rate on top
// (occu_rn.py:214-221; fpr = 0 without one); an expression each
__device__ __forceinline__ float pm_rn_detection(float r, int zn) { return 1.0f - __powf(1.0f - r, (float)zn); }
__device__ __forceinline__ float pm_rn_false_positives(float pd, float fpr) { return 1.0f - (1.0f - pd) * (1.0f - fpr); }
// occu_cop: the false-detection rate of the draw's coordinate phi = log(rate), and a visit's Poisson rate
// dur (z exp(nu) + (1 - z) f_u + f_c)
__device__ __forceinline__ float pm_cop_fp_rate(float phi) { return __expf(phi); }
__device__ __forceinline__ double pm_cop_rate(float dur, int zn, float nu, float f_u, float f_c)
{
    return (double)dur * ((zn ? (double)__expf(nu) : (double)f_u) + (double)f_c);
}
// Poisson(lam): inversion by sequential search for lam < 10, else Hoermann's PTRS transformed rejection
// ("The transformed rejection method for generating Poisson random variables", 1993); both exact.  The number of uniforms depends on
// the data.
__device__ inline int bl_poisson(BlPredRng &rng, double lam)
{
    if (!(lam > 0.0)) return 0;
    if (lam < 10.0) {
        const double enlam = exp(-lam);
        int k = 0;
        double prod = (double)rng.uniform();
        while (prod > enlam && k < 1000) { prod *= (double)rng.uniform(); k++; }
        return k;
    }
    const double slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    for (int it = 0; it < 1000; it++) {
        const double U = (double)rng.uniform() - 0.5, V = (double)rng.uniform();
        const double us = 0.5 - fabs(U);
        const double kf = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return (int)kf;
        if (kf < 0.0 || (us < 0.013 && V > us)) continue;
        if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + kf * loglam - lgamma(kf + 1.0)) return (int)kf;
    }
    return (int)lam;
}
// a standard normal by Box-Muller: two uniforms, the first floored at 2^-24
__device__ __forceinline__ float pm_normal(BlPredRng &rng)
{
    const float u1 = fmaxf(rng.uniform(), 5.9604645e-08f), u2 = rng.uniform();
    return sqrtf(-2.0f * __logf(u1)) * __cosf(6.2831853f * u2);
}

} // namespace
