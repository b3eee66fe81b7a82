// predict.hip -- the kernels of bl_predict, bl_predict_counts, bl_predict_scores and bl_deterministic: the posterior predictive of the
// plain and the random-effects models with the observations withheld, and their deterministic sites, per posterior draw.
//
// One thread per site, 256-thread blocks, the draws on grid.y, the periods in a loop: every global access of a wavefront is contiguous, a
// draw's coefficients are wave-uniform.  The three predictive kernels keep the site's covariates in registers over the draws.  The
// cell's generator is bl_cell_rng (pred_rng.hpp): one per (draw, period, site), the latent state first, then the visits in j order, so a
// sample does not depend on the launch geometry, on how the draws are chunked or on which outputs are wanted.  The arithmetic is
// predict_math.hpp's: predictive_check.hip and predictive_density.hip regenerate these kernels' values from the same statements.
#include "predict.hpp"

#include "../../include/biolith_hip.h"
#include "predict_math.hpp"

// occu (occu.py:207-241 with obs=None):  z ~ Bernoulli(psi),  y_j ~ Bernoulli(z * p_j)
// occu_rn (occu_rn.py:192-221):          N ~ Categorical(Poisson(lambda) pmf on 0..K),  y_j ~ Bernoulli(1 - (1 - r_j)^N)
__global__ void bl_predict_kernel(const BlPredictParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const int ns = p.ns, N = p.N, T = p.T, J = p.J, Ks = p.Ks, Ko = p.Ko, model = p.model;
    const BlDrawCoords c = p.c;
    unsigned char *__restrict__ latent = p.latent, *__restrict__ y = p.y;
    float x[BL_MAX_COVS];
    for (int k = 0; k < Ks; k++) x[k] = p.rows[(size_t)k * ns + i];
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *th = p.draws + (size_t)n * p.D;
        const float *al = th + Ks + 1;
        const float eta = pm_site_eta(x, 1, th, Ks, c, i);
        // false-positive rate: occu_fp's acts on every site ("constant") or on unoccupied ones only; Royle-Nichols' is constant
        const float fpr = c.fp_mode ? pm_sigmoid(th[c.o_fp]) : 0.0f;
        const float f_c = c.fp_mode == BL_FP_CONSTANT ? fpr : 0.0f, f_u = c.fp_mode == BL_FP_UNOCCUPIED ? fpr : 0.0f;
        for (int t = 0; t < T; t++) {
            BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, i);
            const int zn = model == 1 ? pm_draw_abundance(rng, eta, p.K) : pm_draw_z(rng, pm_sigmoid(eta));
            if (latent) latent[((size_t)(n - p.n0) * T + t) * N + i] = (unsigned char)zn;
            if (!y) continue;
            for (int j = 0; j < J; j++) {
                const float r = pm_sigmoid(pm_visit_nu(p.wraw, ns, th, al, Ko, c, T, J, t * J + j, i));
                float pd = model == 1 ? pm_rn_detection(r, zn) : (float)zn * r;
                if (model == 2) pd = pm_false_positives(pd, f_c, f_u, zn);
                if (model == 1) pd = pm_rn_false_positives(pd, fpr); // (Royle-Nichols with a false-positive rate: occu_rn.py:214-221; fpr = 0 without)
                const float u = rng.uniform();
                y[(((size_t)(n - p.n0) * J + j) * T + t) * N + i] = (u < pd) ? 1 : 0;
            }
        }
    }
}

// occu_cop (occu_cop.py:222-255, obs withheld):  z ~ Bernoulli(psi),  y_j ~ Poisson(dur_j (z lambda_j + (1 - z) f_u + f_c))
// nmixture (nmixture.py:183-220, obs withheld):  N ~ Poisson(lambda) restricted to 0..K,  y_j ~ Binomial(N, p_j)
__global__ void bl_predict_counts_kernel(const BlPredictParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const int ns = p.ns, N = p.N, T = p.T, J = p.J, Ks = p.Ks, Ko = p.Ko, model = p.model;
    const BlDrawCoords c = p.c;
    int *__restrict__ latent = p.count_latent, *__restrict__ y = p.count_y;
    float x[BL_MAX_COVS];
    for (int k = 0; k < Ks; k++) x[k] = p.rows[(size_t)k * ns + i];
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *th = p.draws + (size_t)n * p.D;
        const float *al = th + Ks + 1;
        const float eta = pm_site_eta(x, 1, th, Ks, c, i);
        const float f = c.fp_mode ? pm_cop_fp_rate(th[c.o_fp]) : 0.0f; // occu_cop's rate of false detections
        const float f_c = c.fp_mode == BL_FP_CONSTANT ? f : 0.0f, f_u = c.fp_mode == BL_FP_UNOCCUPIED ? f : 0.0f;
        for (int t = 0; t < T; t++) {
            BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, i);
            const int zn = model == 4 ? pm_draw_abundance(rng, eta, p.K) : pm_draw_z(rng, pm_sigmoid(eta));
            if (latent) latent[((size_t)(n - p.n0) * T + t) * N + i] = zn;
            if (!y) continue;
            for (int j = 0; j < J; j++) {
                const int v = t * J + j;
                const float nu = pm_visit_nu(p.wraw, ns, th, al, Ko, c, T, J, v, i);
                int cnt = 0;
                if (model == 4) {
                    cnt = bl_binomial(rng, zn, pm_sigmoid(nu)); // Binomial(N, p), N <= 127 (pred_rng.hpp)
                } else {
                    cnt = bl_poisson(rng, pm_cop_rate(p.dur[(size_t)v * ns + i], zn, nu, f_u, f_c)); // (Poisson by inversion or PTRS: predict_math.hpp)
                }
                y[(((size_t)(n - p.n0) * J + j) * T + t) * N + i] = cnt;
            }
        }
    }
}

// occu_cs (occu_cs.py:196-232 with obs=None):  z ~ Bernoulli(psi);  f_j ~ Bernoulli(z p_j);  s_j ~ Normal(mu_f, sigma_f)
// (draw = [beta, alpha, mu0, log(mu1 - mu0), log sigma0, log sigma1])
__global__ void bl_predict_scores_kernel(const BlPredictParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const int ns = p.ns, N = p.N, T = p.T, J = p.J, Ks = p.Ks, Ko = p.Ko;
    unsigned char *__restrict__ latent = p.latent, *__restrict__ f_out = p.f;
    float *__restrict__ s_out = p.s;
    float x[BL_MAX_COVS];
    for (int k = 0; k < Ks; k++) x[k] = p.rows[(size_t)k * ns + i];
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *th = p.draws + (size_t)n * p.D, *al = th + Ks + 1, *ex = th + Ks + Ko + 2;
        const float mu0 = ex[0], mu1 = ex[0] + __expf(ex[1]), sg0 = __expf(ex[2]), sg1 = __expf(ex[3]);
        const float psi = pm_sigmoid(pm_linear(x, 1, th, Ks));
        for (int t = 0; t < T; t++) {
            BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, i);
            const int zn = pm_draw_z(rng, psi);
            if (latent) latent[((size_t)(n - p.n0) * T + t) * N + i] = (unsigned char)zn;
            for (int j = 0; j < J; j++) {
                const float nu = pm_visit_linear(p.wraw, ns, al, Ko, t * J + j, i);
                const int fn = rng.uniform() < (float)zn * pm_sigmoid(nu) ? 1 : 0; // (z p_j, as bl_predict_kernel states it)
                const float g = pm_normal(rng); // one normal per replicate
                const size_t o = (((size_t)(n - p.n0) * J + j) * T + t) * N + i;
                if (f_out) f_out[o] = (unsigned char)fn;
                if (s_out) s_out[o] = fn ? fmaf(sg1, g, mu1) : fmaf(sg0, g, mu0);
            }
        }
    }
}

// psi[n][t][i] = sigmoid(beta0 + x_i . beta)      (occu.py:198-207; constant over t)
// With random effects the site's occupancy effect joins eta, its detection effect and the replicate's effect join nu (occu.py:198-202,
// 221-228).
__global__ void bl_psi_kernel(const BlPredictParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const int ns = p.ns, N = p.N, T = p.T, Ks = p.Ks;
    float *__restrict__ psi = p.psi;
    float x[BL_MAX_COVS];
    for (int k = 0; k < Ks; k++) x[k] = p.rows[(size_t)k * ns + i];
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float eta = pm_site_eta(x, 1, p.draws + (size_t)n * p.D, Ks, p.c, i);
        // occu: psi = sigmoid(eta) (occu.py:207); occu_rn, nmixture: abundance = exp(eta) (occu_rn.py:192)
        const float v = (p.model == 1 || p.model == 4) ? __expf(eta) : pm_sigmoid(eta);
        for (int t = 0; t < T; t++) psi[((size_t)(n - p.n0) * T + t) * N + i] = v;
    }
}
// prob_detection[n][j][t][i] = sigmoid(alpha0 + w_itj . alpha)   (occu.py:221-228)
__global__ void bl_pdet_kernel(const BlPredictParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const int N = p.N, T = p.T, J = p.J;
    float *__restrict__ out = p.prob;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *th = p.draws + (size_t)n * p.D;
        for (int t = 0; t < T; t++)
            for (int j = 0; j < J; j++) {
                const float nu = pm_visit_nu(p.wraw, p.ns, th, th + p.Ks + 1, p.Ko, p.c, T, J, t * J + j, i);
                // occu / occu_rn: prob_detection = sigmoid(nu); occu_cop: rate_detection = exp(nu) (occu_cop.py:236-243)
                out[(((size_t)(n - p.n0) * J + j) * T + t) * N + i] = p.model == 3 ? __expf(nu) : pm_sigmoid(nu);
            }
    }
}

template <class Kernel>
static int pr_launch(Kernel kernel, const BlPredictParams *p, int grid_y, hipStream_t st)
{
    hipLaunchKernelGGL(kernel, dim3((p->N + 255) / 256, grid_y), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int bl_launch_predict(const BlPredictParams *p, int grid_y, hipStream_t st) { return pr_launch(bl_predict_kernel, p, grid_y, st); }
extern "C" int bl_launch_predict_counts(const BlPredictParams *p, int grid_y, hipStream_t st) { return pr_launch(bl_predict_counts_kernel, p, grid_y, st); }
extern "C" int bl_launch_predict_scores(const BlPredictParams *p, int grid_y, hipStream_t st) { return pr_launch(bl_predict_scores_kernel, p, grid_y, st); }
extern "C" int bl_launch_deterministic(const BlPredictParams *p, int grid_y, hipStream_t st)
{
    int rc = p->psi ? pr_launch(bl_psi_kernel, p, grid_y, st) : 0;
    if (!rc && p->prob) rc = pr_launch(bl_pdet_kernel, p, grid_y, st);
    return rc;
}
