// score_posterior.hip -- the kernel of bl_score_posterior: the two enumerated layers of occu_cs given the data, per posterior draw.
// Per (period, site) cell, with p_j = sigmoid(alpha . (1, w_j)), n0_j / n1_j = log Normal(s_j; mu0, sigma0) / (s_j; mu1, sigma1) and the
// sums over the cell's unmasked visits:
//   mix_j = logaddexp(log p_j + n1_j, log(1 - p_j) + n0_j)          log p(s_j | z = 1)
//   A = log psi + sum mix_j,   B = log(1 - psi) + sum n0_j          (z = 0 forces every f_j = 0)
//   log_lik = logaddexp(A, B),  z_prob = sigmoid(A - B),  r_j = sigmoid((log p_j + n1_j) - (log(1 - p_j) + n0_j)) = P(f_j = 1 | z = 1, s_j)
//   f_prob_j = z_prob r_j;  a masked visit has no score to condition on: r_j = p_j.
// A cell without an unmasked visit has log_lik = 0 and z_prob = psi.  log p, log(1 - p), log psi and log(1 - psi) are the exact
// log-sigmoid forms (min(x, 0) - log1p(exp(-|x|))), never the log of a rounded probability.
//
// One thread per site, the draws on grid.y: a visit's rows are read by 64 neighbouring sites at once and f_prob / f are written the
// same way; a draw's coefficients are wave-uniform.  Two passes over a cell's visits: the first sums A and B, the second recomputes
// each visit's terms (sp_visit, one statement of them for both passes) and writes f_prob_j and f_j, which need the cell's z_prob and z.
// Nothing is kept per visit between the passes (J reaches 52), so no array with a run-time index exists and nothing goes to scratch.
//
// Random numbers: one BlPredRng(seed, ((n T) + t) N + i) per cell, n the ABSOLUTE draw index.  Order of its uniforms: the first decides
// z = [u < z_prob]; then one per visit in j order, masked visits included and whatever z is, f_j = z [u_j < r_j].  The draws are joint:
// f_j <= z.  The second pass (and its uniforms) is skipped when neither f_prob nor f is wanted; z does not depend on that.
#include "score_posterior.hpp"

#include "posterior_math.hpp"
#include "pred_rng.hpp"

namespace {

constexpr float SC_HL2PI = 0.9189385f;

// a draw's score distributions: the means, 1 / sigma, log sigma + log(2 pi) / 2
struct ScDraw {
    float mu0, mu1, is0, is1, c0, c1;
};
// a visit: the mask, log p(s | z = 1), log p(s | z = 0), P(f = 1 | z = 1, s) (the detection probability itself where masked)
struct ScVisit {
    float c, mix, n0, r;
};

__device__ __forceinline__ ScVisit sc_visit(const BlScorePostParams &p, const float *__restrict__ al, const ScDraw &d, int v, int i)
{
    const int ns = p.ns, Ko = p.Ko;
    ScVisit o;
    o.c = p.rows[(size_t)(p.r0 + v * p.vw) * ns + i];
    const float s = p.scores[(size_t)v * ns + i];
    float nu = al[0];
    for (int k = 0; k < Ko; k++) nu = fmaf(p.wraw[((size_t)v * Ko + k) * ns + i], al[k + 1], nu);
    const float e = bl_exp(-fabsf(nu)), l = post_log1p(e);
    const float lp = fminf(nu, 0.0f) - l, l1p = -fmaxf(nu, 0.0f) - l; // log p, log(1 - p)
    const float e0 = (s - d.mu0) * d.is0, e1 = (s - d.mu1) * d.is1;
    const float n1 = fmaf(-0.5f * e1, e1, -d.c1);
    o.n0 = fmaf(-0.5f * e0, e0, -d.c0);
    const float t1 = lp + n1, t0 = l1p + o.n0, dt = t1 - t0, ed = bl_exp(-fabsf(dt));
    o.mix = fmaxf(t1, t0) + post_log1p(ed);
    o.r = (dt > 0.0f ? 1.0f : ed) * bl_rcp(1.0f + ed);
    if (o.c == 0.0f) o.r = (nu > 0.0f ? 1.0f : e) * bl_rcp(1.0f + e);
    return o;
}

} // namespace

__global__ void bl_score_posterior_kernel(const BlScorePostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const float *__restrict__ rows = p.rows;
    const int ns = p.ns, N = p.N, T = p.T, J = p.J;
    const bool visits = p.f_prob || p.f;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        const float *__restrict__ al = th + p.Ks + 1, *__restrict__ ex = al + p.Ko + 1;
        float eta = th[0];
        for (int k = 0; k < p.Ks; k++) eta = fmaf(rows[(size_t)k * ns + i], th[k + 1], eta);
        const float ee = bl_exp(-fabsf(eta)), lop = post_log1p(ee);
        const float log_psi = fminf(eta, 0.0f) - lop, log_1mpsi = fminf(-eta, 0.0f) - lop;
        const float psi = (eta > 0.0f ? 1.0f : ee) * bl_rcp(1.0f + ee);
        ScDraw d;
        d.mu0 = ex[0]; d.mu1 = ex[0] + bl_exp(ex[1]);
        d.is0 = bl_exp(-ex[2]); d.is1 = bl_exp(-ex[3]);
        d.c0 = ex[2] + SC_HL2PI; d.c1 = ex[3] + SC_HL2PI;
        for (int t = 0; t < T; t++) {
            PostSum a1, a0;
            a1.add(log_psi);
            a0.add(log_1mpsi);
            float nobs = 0.0f;
            for (int j = 0; j < J; j++) {
                const ScVisit w = sc_visit(p, al, d, t * J + j, i);
                if (w.c == 0.0f) continue; // masked
                nobs += 1.0f;
                a1.add(w.mix);
                a0.add(w.n0);
            }
            const float A = a1.s, B = a0.s;
            const float dd = A - B, e = bl_exp(-fabsf(dd));
            float l = fmaxf(A, B) + post_log1p(e);
            float q = (dd > 0.0f ? 1.0f : e) * bl_rcp(1.0f + e);
            if (nobs == 0.0f) { l = 0.0f; q = psi; } // nothing observed: the cell's likelihood is 1 and the conditional is the prior
            const size_t o = ((size_t)(n - p.n0) * T + t) * N + i;
            if (p.log_lik) p.log_lik[o] = l;
            if (p.z_prob) p.z_prob[o] = q;
            if (!p.z && !visits) continue;
            BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, i);
            const bool zn = rng.uniform() < q;
            if (p.z) p.z[o] = zn ? 1 : 0;
            if (!visits) continue;
            for (int j = 0; j < J; j++) {
                const ScVisit w = sc_visit(p, al, d, t * J + j, i);
                const float u = rng.uniform();
                const size_t ov = (((size_t)(n - p.n0) * J + j) * T + t) * N + i;
                if (p.f_prob) p.f_prob[ov] = q * w.r;
                if (p.f) p.f[ov] = (zn && u < w.r) ? 1 : 0;
            }
        }
    }
}

extern "C" int bl_launch_score_posterior(const BlScorePostParams *p, int grid_y, hipStream_t st)
{
    dim3 grid, block;
    post_geometry(p->N, grid_y, grid, block);
    hipLaunchKernelGGL(bl_score_posterior_kernel, grid, block, 0, st, *p);
    return (int)hipGetLastError();
}
