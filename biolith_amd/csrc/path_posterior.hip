// path_posterior.hip -- the kernel of bl_path_posterior: per posterior draw and site of the dynamic occupancy model (dyn_device.hpp)
// the path-marginalised log-likelihood, the smoothed marginals rho_t = P(z_t = 1 | y_1..T), the pairwise terms xi_t(0,1) (colonised
// between t and t + 1) and xi_t(1,0) (went extinct), and one joint draw of the path z_1..T by forward filtering, backward sampling.
//
// Forward, t = 0 .. T-1:   a_t = sum_j log sigma(c_j u_j) over the unmasked visits,  kb_t = n_detections log tiny,
//     A = log pi_t + a_t,  B = log(1 - pi_t) + kb_t,  log_lik += logaddexp(A, B),  d_t = A - B  (the filtered log-odds: phi_t = sigmoid(d_t)),
//     pi_t+1 = phi_t (1 - eps) + (1 - phi_t) gamma,   1 - pi_t+1 = phi_t eps + (1 - phi_t)(1 - gamma)        -- two POSITIVE sums.
// A season without an unmasked visit adds nothing (its normaliser is pi + (1 - pi) = 1) and leaves d_t = logit pi_t.
// Backward, t = T-2 .. 0, from rho_T-1 = phi_T-1:  with the backward kernels
//     b_1 = P(z_t = 1 | z_t+1 = 1, y_1..t) = phi (1 - eps) / (phi (1 - eps) + (1 - phi) gamma),   b_0 = phi eps / (phi eps + (1 - phi)(1 - gamma))
//     xi(1,1) = rho_t+1 b_1,  xi(0,1) = rho_t+1 (1 - b_1),  xi(1,0) = (1 - rho_t+1) b_0,  xi(0,0) = (1 - rho_t+1)(1 - b_0),
//     rho_t = xi(1,1) + xi(1,0),  1 - rho_t = xi(0,1) + xi(0,0),   z_t | z_t+1 = b ~ Bernoulli(b_b).
// No complement is ever formed as 1 - x: sigmoid(-eta) gives 1 - eps and 1 - gamma, sigmoid(-d_t) gives 1 - phi_t, and every pair
// (p, 1 - p) that comes out of a ratio is normalised from its two positive parts (pp_norm2), so the smaller side keeps its relative
// precision and the larger one is exactly 1 where the smaller vanishes (a season with a detection: rho_t = 1, z_t = 1).
//
// One thread per site, the draws on grid.y: a visit row is read by 64 neighbouring sites at once, a draw's coefficients are
// wave-uniform.  T is a run-time value: the T filtered log-odds of a site live in the z_prob buffer ([t][N], coalesced), one float a
// cell, and the backward pass overwrites them in place; nothing is kept per period or per covariate in registers, so no array with a
// run-time index exists and nothing goes to scratch.  No LDS.
#include "path_posterior.hpp"

#include "posterior_math.hpp"
#include "pred_rng.hpp"

namespace {

// pa = a / (a + b), pb = b / (a + b) for a, b >= 0 from the ratio of the smaller to the larger
__device__ __forceinline__ void pp_norm2(float a, float b, float &pa, float &pb)
{
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    const float e = hi > 0.0f ? lo * bl_rcp(hi) : 1.0f, r = bl_rcp(1.0f + e);
    pa = (a >= b ? 1.0f : e) * r;
    pb = (a >= b ? e : 1.0f) * r;
}

} // namespace

__global__ void bl_path_posterior_kernel(const BlPathPostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const float *__restrict__ rows = p.rows;
    const int ns = p.ns, N = p.N, T = p.T, J = p.J, Ks = p.Ks, Ko = p.Ko;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        const float *__restrict__ al = th + 3 * (Ks + 1);
        float e_psi = th[0], e_gam = th[Ks + 1], e_eps = th[2 * (Ks + 1)];
        for (int k = 0; k < Ks; k++) {
            const float x = rows[(size_t)k * ns + i];
            e_psi = fmaf(x, th[k + 1], e_psi);
            e_gam = fmaf(x, th[Ks + 1 + k + 1], e_gam);
            e_eps = fmaf(x, th[2 * (Ks + 1) + k + 1], e_eps);
        }
        float gam, ngam, eps, neps;
        post_sig(e_gam, gam, ngam);
        post_sig(e_eps, eps, neps);
        const float lop = post_log1p(bl_exp(-fabsf(e_psi)));
        float lpi = fminf(e_psi, 0.0f) - lop, l1m = fminf(-e_psi, 0.0f) - lop; // log pi_t, log(1 - pi_t)
        const size_t o_site = (size_t)(n - p.n0) * N + i;   // [n][N]
        const size_t o_cell = (size_t)(n - p.n0) * T * N + i; // [n][T][N], period 0
        const size_t o_pair = (size_t)(n - p.n0) * (T - 1) * N + i; // [n][T - 1][N], period 0
        float *__restrict__ dq = p.z_prob + o_cell;
        // ---- forward: the filter ----
        PostSum ll;
        float d = 0.0f;
        for (int t = 0; t < T; t++) {
            PostSum a1;
            a1.add(lpi);
            float nd = 0.0f, nobs = 0.0f;
            for (int j = 0; j < J; j++) {
                const size_t r = (size_t)(p.r0 + (t * J + j) * p.vw) * ns + i;
                const float c = rows[r];
                if (c == 0.0f) continue; // masked
                float u = c * al[0];
                for (int k = 1; k <= Ko; k++) u = fmaf(rows[r + (size_t)k * ns], al[k], u);
                a1.add(fminf(u, 0.0f) - post_log1p(bl_exp(-fabsf(u)))); // log sigma(c u)
                nobs += 1.0f;
                if (c > 0.0f) nd += 1.0f;
            }
            const float A = a1.s, B = fmaf(nd, POST_LOG_TINY, l1m);
            d = A - B;
            if (nobs > 0.0f) ll.add(fmaxf(A, B) + post_log1p(bl_exp(-fabsf(d)))); // (nothing observed: the season's likelihood is 1)
            dq[(size_t)t * N] = d;
            if (t + 1 < T) {
                float f, g;
                post_sig(d, f, g);
                lpi = bl_log(fmaxf(fmaf(f, neps, g * gam), POST_TINY));
                l1m = bl_log(fmaxf(fmaf(f, eps, g * ngam), POST_TINY));
            }
        }
        if (p.log_lik) p.log_lik[o_site] = ll.s;
        // ---- backward: the smoother, and the path drawn from its far end ----
        float rho, nrho;
        post_sig(d, rho, nrho);
        bool zb = false;
        if (p.z) {
            BlPredRng rng = bl_cell_rng(p.seed, n, T, T - 1, N, i);
            zb = rng.uniform() < rho;
            p.z[o_cell + (size_t)(T - 1) * N] = zb ? 1 : 0;
        }
        for (int t = T - 2; t >= 0; t--) {
            float f, g, b1, nb1, b0, nb0;
            post_sig(dq[(size_t)t * N], f, g);
            pp_norm2(f * neps, g * gam, b1, nb1);
            pp_norm2(f * eps, g * ngam, b0, nb0);
            const float xi01 = rho * nb1, xi10 = nrho * b0;
            const float r1 = fmaf(rho, b1, xi10), r0 = fmaf(nrho, nb0, xi01);
            dq[(size_t)(t + 1) * N] = rho;
            if (p.col_prob) p.col_prob[o_pair + (size_t)t * N] = xi01;
            if (p.ext_prob) p.ext_prob[o_pair + (size_t)t * N] = xi10;
            if (p.z) {
                BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, i);
                zb = rng.uniform() < (zb ? b1 : b0);
                p.z[o_cell + (size_t)t * N] = zb ? 1 : 0;
            }
            pp_norm2(r1, r0, rho, nrho);
        }
        dq[0] = rho;
    }
}

extern "C" int bl_launch_path_posterior(const BlPathPostParams *p, int grid_y, hipStream_t st)
{
    dim3 grid, block;
    post_geometry(p->N, grid_y, grid, block);
    hipLaunchKernelGGL(bl_path_posterior_kernel, grid, block, 0, st, *p);
    return (int)hipGetLastError();
}
