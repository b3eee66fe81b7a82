// site_cell.hpp -- the conditional of ONE cell (period t, site i) of an occu handle under one draw, stated once for every kernel that
// needs it: site_posterior.hip (bl_site_posterior) and residual_moran.hip (bl_residual_moran, whose z must be bl_site_posterior's bit
// for bit, now and after later edits).  -ffp-contract=on fuses per source expression, so the two kernels agree because they call the
// same text, not because two texts happen to compile alike.
//
//   A = log psi + log p(obs | z = 1),  B = log(1 - psi) + log p(obs | z = 0),  l = logaddexp(A, B),  q = sigmoid(A - B)
// over the cell's unmasked visits (c = 0 in a visit's record masks it); a cell without one: l = 0, q = psi.  The z = 1 sum is
// Kahan-compensated.  occu_comb adds its ARU block and its scores between sc_visits and sc_conditional (site_posterior.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "posterior_math.hpp"
#include "site_posterior.hpp"

namespace {

// f = sigmoid(phi): f, 1 - f, log f, log(1 - f)
__device__ __forceinline__ void sp_rate(float phi, float &f, float &g, float &lf, float &l1f)
{
    const float e = bl_exp(-fabsf(phi)), l = post_log1p(e), r = bl_rcp(1.0f + e);
    f = (phi > 0.0f ? 1.0f : e) * r;
    g = (phi > 0.0f ? e : 1.0f) * r;
    lf = fminf(phi, 0.0f) - l;
    l1f = -fmaxf(phi, 0.0f) - l;
}

// What a draw fixes for site i before any period: the prior's logs, the site's detection effect, and what a detection / a
// non-detection of block a costs at z = 0 and the rate that acts at z = 1 (false positives; FP = false: none, occu_comb's block a).
struct SiteCellPrior {
    float log_psi, log_1mpsi, psi, vi;
    float f1 = 0.0f, l1f1 = 0.0f, z0_det = POST_LOG_TINY, z0_non = 0.0f;
};
template <bool FP>
__device__ __forceinline__ SiteCellPrior sc_prior(const float *__restrict__ rows, int ns, int i, int Ks, const float *__restrict__ th,
                                                  const BlDrawCoords &c)
{
    SiteCellPrior s;
    float eta = th[0];
    for (int k = 0; k < Ks; k++) eta = fmaf(rows[(size_t)k * ns + i], th[k + 1], eta);
    if (c.o_u >= 0) eta += th[c.o_u + i];
    s.vi = c.o_v >= 0 ? th[c.o_v + i] : 0.0f;
    const float ee = bl_exp(-fabsf(eta)), lop = post_log1p(ee);
    s.log_psi = fminf(eta, 0.0f) - lop;
    s.log_1mpsi = fminf(-eta, 0.0f) - lop;
    s.psi = (eta > 0.0f ? 1.0f : ee) * bl_rcp(1.0f + ee);
    if constexpr (FP) {
        if (c.fp_mode) {
            float f, g;
            sp_rate(th[c.o_fp], f, g, s.z0_det, s.z0_non);
            if (c.fp_mode == 1) { s.f1 = f; s.l1f1 = s.z0_non; }
        }
    }
    return s;
}

// The record loop of block a in period t: the z = 1 terms into a1, the unmasked detections / non-detections into nd / nn.
// EFFECTS: the site's and the visits' detection effects join the predictor (occu; occu_comb's point counts have none).
template <bool EFFECTS>
__device__ __forceinline__ void sc_visits(const float *__restrict__ rows, int ns, int i, int T, int t, const BlSitePostBlock &a,
                                          const float *__restrict__ th, const BlDrawCoords &c, const SiteCellPrior &s, PostSum &a1,
                                          float &nd, float &nn)
{
    const float *__restrict__ al = th + a.o_al;
    for (int j = 0; j < a.J; j++) {
        const int v = t * a.J + j;
        const size_t r = (size_t)(a.r0 + v * a.vw) * ns + i;
        const float cc = rows[r];
        if (cc == 0.0f) continue; // masked
        float u = cc * al[0];
        for (int k = 1; k <= a.K; k++) u = fmaf(rows[r + (size_t)k * ns], al[k], u);
        if constexpr (EFFECTS) {
            float re = s.vi;
            if (c.o_e >= 0) re += th[(size_t)c.o_e + (size_t)i * T * a.J + v];
            u = fmaf(cc, re, u);
        }
        const float e = bl_exp(-fabsf(u)), lsu = fminf(u, 0.0f) - post_log1p(e); // log sigma(u)
        if (cc > 0.0f) {
            nd += 1.0f;
            if (s.f1 > 0.0f) { // log(p + f (1 - p))
                const float rop = bl_rcp(1.0f + e);
                a1.add(bl_log(fmaf(s.f1, (u > 0.0f ? e : 1.0f) * rop, (u > 0.0f ? 1.0f : e) * rop)));
            } else
                a1.add(lsu);
        } else {
            nn += 1.0f;
            a1.add(lsu);
        }
    }
}

// l and q of a cell from its A, B and its count of unmasked observations
__device__ __forceinline__ void sc_conditional(float A, float B, float nobs, float psi, float &l, float &q)
{
    const float d = A - B, e = bl_exp(-fabsf(d));
    l = fmaxf(A, B) + post_log1p(e);
    q = (d > 0.0f ? 1.0f : e) * bl_rcp(1.0f + e);
    if (nobs == 0.0f) { l = 0.0f; q = psi; } // nothing observed: the cell's likelihood is 1 and the conditional is the prior
}

// occu's cell, whole: block a alone
__device__ __forceinline__ void sc_cell(const float *__restrict__ rows, int ns, int i, int T, int t, const BlSitePostBlock &a,
                                        const float *__restrict__ th, const BlDrawCoords &c, const SiteCellPrior &s, float &l, float &q)
{
    PostSum a1;
    a1.add(s.log_psi);
    float nd = 0.0f, nn = 0.0f;
    sc_visits<true>(rows, ns, i, T, t, a, th, c, s, a1, nd, nn);
    a1.add(nn * s.l1f1);
    const float B = s.log_1mpsi + fmaf(nd, s.z0_det, nn * s.z0_non);
    sc_conditional(a1.s, B, nd + nn, s.psi, l, q);
}

} // namespace
