// comb_predict.hip -- the kernels of bl_predict_comb and bl_deterministic_comb: occu_comb's posterior predictive and its deterministic
// sites, per posterior draw (biolith/models/occu_comb.py:224-349 with all three observed sites withheld).
//   psi = sigmoid(beta . (1, x)),  p_pc = sigmoid(alpha_PC . (1, w_pc)),  p_aru = sigmoid(alpha_ARU . (1, w_aru))
//   z ~ Bernoulli(psi);  y_pc ~ Bernoulli(z p_pc);  y_aru ~ Bernoulli(1 - (1 - z p_aru)(1 - fc)(1 - (1 - z) fu));
//   score ~ Normal(z ? mu1 : mu0, z ? sigma1 : sigma0)
// The sigmoid, the predictors, the false-positive composition and the normal are predict_math.hpp's: the other models' kernels call the
// same statements, so the sites agree with theirs to the same bound.
//
// One thread per site, the draws on grid.y, the periods in a loop: every global access of a wavefront is contiguous, a draw's
// coefficients are wave-uniform.  Nothing is kept per covariate (the rows are read where they are used), so no array with a run-time
// index exists and nothing goes to scratch.  The cell's generator is bl_predict's (bl_cell_rng), and it is consumed
// in one fixed order -- one uniform for z, one per point-count visit, one per ARU visit, two per score (Box-Muller, as
// bl_predict_scores) -- whichever outputs are wanted: a NULL output never changes another one.
#include "comb_predict.hpp"

#include "posterior_math.hpp"
#include "predict_math.hpp"

__global__ void bl_comb_predict_kernel(const BlCombPredParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const int ns = p.ns, N = p.N, T = p.T, Jp = p.pc.J, Ja = p.aru.J, Js = p.Js;
    // what is still to be written behind each block: the generator is only advanced while something behind it needs it
    const bool need_sc = p.scores != nullptr && Js > 0, need_aru = need_sc || (p.y_aru != nullptr && Ja > 0);
    const bool need_pc = need_aru || (p.y_pc != nullptr && Jp > 0);
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        const float *__restrict__ apc = th + p.pc.o_al, *__restrict__ aar = th + p.aru.o_al, *__restrict__ ex = th + p.o_x;
        const float psi = pm_sigmoid(pm_linear(p.rows + i, ns, th, p.Ks));
        const float fc = pm_sigmoid(ex[0]), fu = pm_sigmoid(ex[1]);
        const float mu0 = ex[2], mu1 = ex[2] + __expf(ex[3]), sg0 = __expf(ex[4]), sg1 = __expf(ex[5]);
        const size_t nb = (size_t)(n - p.n0);
        for (int t = 0; t < T; t++) {
            BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, i);
            const int zn = pm_draw_z(rng, psi);
            if (p.z) p.z[(nb * T + t) * N + i] = (unsigned char)zn;
            if (!need_pc) continue;
            for (int j = 0; j < Jp; j++) {
                const float u = rng.uniform();
                if (!p.y_pc) continue;
                const float pd = (float)zn * pm_sigmoid(pm_visit_linear(p.pc.w, ns, apc, p.pc.K, t * Jp + j, i));
                p.y_pc[((nb * Jp + j) * T + t) * N + i] = u < pd ? 1 : 0;
            }
            if (!need_aru) continue;
            for (int j = 0; j < Ja; j++) {
                const float u = rng.uniform();
                if (!p.y_aru) continue;
                const float r = (float)zn * pm_sigmoid(pm_visit_linear(p.aru.w, ns, aar, p.aru.K, t * Ja + j, i));
                const float pd = pm_false_positives(r, fc, fu, zn);
                p.y_aru[((nb * Ja + j) * T + t) * N + i] = u < pd ? 1 : 0;
            }
            if (!need_sc) continue;
            for (int j = 0; j < Js; j++) {
                const float g = pm_normal(rng); // one normal per score
                p.scores[((nb * Js + j) * T + t) * N + i] = zn ? fmaf(sg1, g, mu1) : fmaf(sg0, g, mu0);
            }
        }
    }
}

// psi [n][T][N] (constant over the periods), PC_prob_detection [n][Jpc][T][N], ARU_prob_detection [n][Jaru][T][N]
__global__ void bl_comb_deterministic_kernel(const BlCombPredParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const int ns = p.ns, N = p.N, T = p.T, Jp = p.pc.J, Ja = p.aru.J;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        const size_t nb = (size_t)(n - p.n0);
        if (p.psi) {
            const float psi = pm_sigmoid(pm_linear(p.rows + i, ns, th, p.Ks));
            for (int t = 0; t < T; t++) p.psi[(nb * T + t) * N + i] = psi;
        }
        if (p.pc_prob)
            for (int t = 0; t < T; t++)
                for (int j = 0; j < Jp; j++)
                    p.pc_prob[((nb * Jp + j) * T + t) * N + i] = pm_sigmoid(pm_visit_linear(p.pc.w, ns, th + p.pc.o_al, p.pc.K, t * Jp + j, i));
        if (p.aru_prob)
            for (int t = 0; t < T; t++)
                for (int j = 0; j < Ja; j++)
                    p.aru_prob[((nb * Ja + j) * T + t) * N + i] = pm_sigmoid(pm_visit_linear(p.aru.w, ns, th + p.aru.o_al, p.aru.K, t * Ja + j, i));
    }
}

extern "C" int bl_launch_comb_predict(const BlCombPredParams *p, int grid_y, hipStream_t st)
{
    dim3 grid, block;
    post_geometry(p->N, grid_y, grid, block);
    hipLaunchKernelGGL(bl_comb_predict_kernel, grid, block, 0, st, *p);
    return (int)hipGetLastError();
}

extern "C" int bl_launch_comb_deterministic(const BlCombPredParams *p, int grid_y, hipStream_t st)
{
    dim3 grid, block;
    post_geometry(p->N, grid_y, grid, block);
    hipLaunchKernelGGL(bl_comb_deterministic_kernel, grid, block, 0, st, *p);
    return (int)hipGetLastError();
}
