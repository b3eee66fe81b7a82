// site_posterior.hip -- the kernel of bl_site_posterior: per posterior draw and (period, site) the z-marginalised log-likelihood
// l = logaddexp(A, B), the conditional occupancy probability q = sigmoid(A - B) and one draw z ~ Bernoulli(q), with
//   A = log psi + log p(obs | z = 1),  B = log(1 - psi) + log p(obs | z = 0)
// as the density kernels define them (occu_device.hpp: bl_eval_sites_hbm / _fp; re_kernel.hpp: bl_re_site_pass, bl_comb_site_pass):
// the same terms, the same clamps (a detection at z = 0 without a false-positive rate costs log tiny; occu_comb's z = 0 ARU
// probability is clamped to [tiny, 1 - eps]), the same masks (c = 0 in a visit's record, n = 0 in a period's score row).
//
// One thread per site, the draws on grid.y: a visit row is read by 64 neighbouring sites at once, a draw's coefficients are
// wave-uniform.  Nothing is kept per covariate: the rows are read where they are used (the data set is L2-resident), so no array
// with a run-time index exists and nothing goes to scratch.  The z = 1 sum is Kahan-compensated and log(1 + e) keeps its low bits,
// so that a cell's error stays a few ulps of its largest term however many visits it has.
#include "site_posterior.hpp"

#include "posterior_math.hpp"
#include "pred_rng.hpp"
#include "site_cell.hpp"

namespace {

constexpr float SP_HL2PI = 0.9189385f;

} // namespace

template <bool COMB>
__global__ void bl_site_posterior_kernel(const BlSitePostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const float *__restrict__ rows = p.rows;
    const int ns = p.ns, N = p.N, T = p.T;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        // the draw's scalars for this site (site_cell.hpp); occu_comb's point counts take no false-positive rate of the draw's layout
        const SiteCellPrior s = sc_prior<!COMB>(rows, ns, i, p.Ks, th, p.c);
        float fc = 0.0f, lgc = 0.0f, lp0 = 0.0f, lq0 = 0.0f, mu0 = 0.0f, mu1 = 0.0f, c0 = 0.0f, c1 = 0.0f, is0 = 0.0f, is1 = 0.0f;
        if constexpr (COMB) {
            float gc, fu, gu, lfc, lfu, lgu;
            sp_rate(th[p.o_x], fc, gc, lfc, lgc);
            sp_rate(th[p.o_x + 1], fu, gu, lfu, lgu);
            lp0 = bl_log(fmaxf(fmaf(fu, gc, fc), POST_TINY)); // p0 = 1 - (1 - fc)(1 - fu), clamped to [tiny, 1 - eps]
            lq0 = fmaxf(lgc + lgu, POST_LOG_EPS);
            mu0 = th[p.o_x + 2]; mu1 = mu0 + bl_exp(th[p.o_x + 3]);
            c0 = th[p.o_x + 4] + SP_HL2PI; c1 = th[p.o_x + 5] + SP_HL2PI;              // log sigma + log(2 pi) / 2
            is0 = bl_exp(-2.0f * th[p.o_x + 4]); is1 = bl_exp(-2.0f * th[p.o_x + 5]);  // 1 / sigma^2
        }
        for (int t = 0; t < T; t++) {
            float l, q;
            if constexpr (!COMB) {
                sc_cell(rows, ns, i, T, t, p.a, th, p.c, s, l, q); // (the statement bl_residual_moran's kernels share)
            } else {
                PostSum a1;
                a1.add(s.log_psi);
                float nd = 0.0f, nn = 0.0f; // unmasked detections / non-detections of block a
                sc_visits<false>(rows, ns, i, T, t, p.a, th, p.c, s, a1, nd, nn);
                a1.add(nn * s.l1f1);
                float B = s.log_1mpsi + fmaf(nd, s.z0_det, nn * s.z0_non);
                float nobs = nd + nn;
                float ad = 0.0f, an = 0.0f;
                const float *__restrict__ aar = th + p.b.o_al;
                for (int j = 0; j < p.b.J; j++) {
                    const size_t r = (size_t)(p.b.r0 + (t * p.b.J + j) * p.b.vw) * ns + i;
                    const float c = rows[r];
                    if (c == 0.0f) continue;
                    float u = c * aar[0];
                    for (int k = 1; k <= p.b.K; k++) u = fmaf(rows[r + (size_t)k * ns], aar[k], u);
                    const float e = bl_exp(-fabsf(u));
                    if (c > 0.0f) { // log(p + fc (1 - p))
                        const float rop = bl_rcp(1.0f + e);
                        ad += 1.0f;
                        a1.add(bl_log(fmaf(fc, (u > 0.0f ? e : 1.0f) * rop, (u > 0.0f ? 1.0f : e) * rop)));
                    } else {        // log(1 - p) + log(1 - fc)
                        an += 1.0f;
                        a1.add(fminf(u, 0.0f) - post_log1p(e));
                    }
                }
                a1.add(an * lgc);
                // the period's unmasked scores as count, mean and sum of squared deviations: sum log N(s; mu, sigma) without per-score work
                const size_t rp = (size_t)(p.r_per + 6 * t) * ns + i;
                const float sc_n = rows[rp + (size_t)3 * ns], sc_m = rows[rp + (size_t)4 * ns], sc_m2 = rows[rp + (size_t)5 * ns];
                const float d1 = sc_m - mu1, d0 = sc_m - mu0;
                const float q1 = fmaf(sc_n * d1, d1, sc_m2) * is1, q0 = fmaf(sc_n * d0, d0, sc_m2) * is0;
                a1.add(fmaf(-0.5f, q1, -sc_n * c1));
                B += fmaf(ad, lp0, an * lq0) + fmaf(-0.5f, q0, -sc_n * c0);
                nobs += ad + an + sc_n;
                sc_conditional(a1.s, B, nobs, s.psi, l, q);
            }
            const size_t o = ((size_t)(n - p.n0) * T + t) * N + i;
            if (p.log_lik) p.log_lik[o] = l;
            if (p.z_prob) p.z_prob[o] = q;
            if (p.z) {
                BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, i);
                p.z[o] = rng.uniform() < q ? 1 : 0;
            }
        }
    }
}

extern "C" int bl_launch_site_posterior(const BlSitePostParams *p, int grid_y, hipStream_t st)
{
    dim3 grid, block;
    post_geometry(p->N, grid_y, grid, block);
    if (p->comb) hipLaunchKernelGGL(bl_site_posterior_kernel<true>, grid, block, 0, st, *p);
    else hipLaunchKernelGGL(bl_site_posterior_kernel<false>, grid, block, 0, st, *p);
    return (int)hipGetLastError();
}
