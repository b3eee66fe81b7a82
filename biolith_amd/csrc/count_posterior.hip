// count_posterior.hip -- the kernel of bl_count_posterior: occupancy and the true detections of occu_cop given the counts, per
// posterior draw.  Per (period, site) cell, over the cell's unmasked visits, with lambda_j = exp(min(nu_j, 80)), f the sampled
// false-positive rate (0 without one), f1 = f in "constant" mode else 0, f0 = f, c = sum_j (y_j log d_j - lgamma(y_j + 1)):
//   A = log psi + sum_j [y_j log(lambda_j + f1) - d_j (lambda_j + f1)] + c
//   B = log(1 - psi) + Ysum log f0 - Dsum f0 + c          (f0 = 0: log(1 - psi) + c if Ysum = 0, else -inf: Poisson(0))
//   log_lik = logaddexp(A, B),  z_prob = sigmoid(A - B),  rho_j = lambda_j / (lambda_j + f1) = P(a counted detection was real | z = 1)
//   true_mean_j = z_prob y_j rho_j;  true_count_j = z Binomial(y_j, rho_j): the Poisson thinning of the count.
// A cell without an unmasked visit has log_lik = 0 and z_prob = psi; a masked visit has no count: both visit-level outputs are 0.
// log psi and log(1 - psi) are the exact log-sigmoid forms; y log(lambda + f1) is y nu when f1 = 0 (no log of a rounded rate), as in
// the sampler (occu_device.hpp: bl_eval_sites_cop).  c comes from the host, summed in float64 (count_posterior.hpp).
//
// One thread per site, the draws on grid.y: a visit's rows are read by 64 neighbouring sites at once and the visit-level outputs are
// written the same way; a draw's coefficients are wave-uniform.  Two passes over a cell's visits: the first sums A, the second
// recomputes each visit's terms (cp_visit, one statement of them for both passes) and writes true_mean_j and true_count_j, which need
// the cell's z_prob and z.  Nothing is kept per visit between the passes (J is 52 at simulate_cop()'s defaults), so no array with a
// run-time index exists and nothing goes to scratch.
//
// Random numbers: one BlPredRng(seed, ((n T) + t) N + i) per cell, n the ABSOLUTE draw index.  Order of its uniforms: the first decides
// z = [u < z_prob]; then the visits in j order, whatever z is: in "constant" mode visit j takes y_j uniforms, one Bernoulli(rho_j) trial
// per counted detection (bl_binomial, exact; a masked visit has y_j = 0 and takes none); in the other modes rho_j = 1 and no visit
// takes any.  HOW MANY uniforms a cell takes therefore depends on the data and the handle's mode only, never on theta or z.  The
// draws are joint: true_count_j <= z y_j.  The second pass (and its uniforms) is skipped when neither visit-level output is wanted; z
// does not depend on that.
#include "count_posterior.hpp"

#include "posterior_math.hpp"
#include "pred_rng.hpp"

namespace {

// a visit: the count and the duration (both 0 where masked), its term of the z = 1 branch, rho
struct CpVisit {
    float y, d, a, rho;
};

__device__ __forceinline__ CpVisit cp_visit(const BlCountPostParams &p, const float *__restrict__ th, const float *__restrict__ al,
                                            float f1, int v, int i)
{
    const int ns = p.ns, Ko = p.Ko;
    const float *__restrict__ rec = p.rows + (size_t)(p.r0 + v * p.vw) * ns + i;
    CpVisit o;
    o.y = rec[0];
    o.d = rec[ns];
    float nu = al[0];
    for (int k = 0; k < Ko; k++) nu = fmaf(rec[(size_t)(2 + k) * ns], al[k + 1], nu);
    if (p.c.o_v >= 0) nu += th[p.c.o_v + i];
    if (p.c.o_e >= 0) nu += th[p.c.o_e + (size_t)i * p.T * p.J + v];
    nu = fminf(nu, 80.0f); // the sampler's clamp: lambda stays finite
    const float lam = bl_exp(nu), tt = lam + f1;
    const bool with_f1 = p.c.fp_mode == 1 /* BL_FP_CONSTANT */;
    const float lt = with_f1 ? bl_log(tt) : nu;
    o.a = fmaf(o.y, lt, -(o.d * tt));
    o.rho = with_f1 ? lam * bl_rcp(tt) : 1.0f;
    return o;
}

} // namespace

__global__ void bl_count_posterior_kernel(const BlCountPostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const float *__restrict__ rows = p.rows;
    const int ns = p.ns, N = p.N, T = p.T, J = p.J;
    const bool visits = p.true_mean || p.true_count;
    const bool with_f1 = p.c.fp_mode == 1 /* BL_FP_CONSTANT */;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        const float *__restrict__ al = th + p.Ks + 1;
        float eta = th[0];
        for (int k = 0; k < p.Ks; k++) eta = fmaf(rows[(size_t)k * ns + i], th[k + 1], eta);
        if (p.c.o_u >= 0) eta += th[p.c.o_u + i];
        const float ee = bl_exp(-fabsf(eta)), lop = post_log1p(ee);
        const float log_psi = fminf(eta, 0.0f) - lop, log_1mpsi = fminf(-eta, 0.0f) - lop;
        const float psi = (eta > 0.0f ? 1.0f : ee) * bl_rcp(1.0f + ee);
        const float phi = p.c.fp_mode ? th[p.c.o_fp] : 0.0f;
        const float f = p.c.fp_mode ? bl_exp(fminf(phi, 80.0f)) : 0.0f, f1 = with_f1 ? f : 0.0f;
        for (int t = 0; t < T; t++) {
            PostSum a1, a0;
            a1.add(log_psi);
            a0.add(log_1mpsi);
            float nobs = 0.0f;
            for (int j = 0; j < J; j++) {
                const CpVisit w = cp_visit(p, th, al, f1, t * J + j, i);
                if (w.d == 0.0f) continue; // masked
                nobs += 1.0f;
                a1.add(w.a);
            }
            const float ysum = rows[(size_t)(p.r_sum + t) * ns + i], dsum = rows[(size_t)(p.r_sum + T + t) * ns + i];
            const float cc = p.ccell[(size_t)t * ns + i];
            a1.add(cc);
            const bool dead0 = !p.c.fp_mode && ysum > 0.0f; // Poisson(0) met a positive count (a Kahan step on -inf would leave inf - inf)
            if (p.c.fp_mode) a0.add(fmaf(ysum, phi, -(dsum * f)));
            a0.add(cc);
            const float A = a1.s, B = dead0 ? -INFINITY : a0.s;
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
                const CpVisit w = cp_visit(p, th, al, f1, t * J + j, i);
                const int y = (int)w.y;
                const int real = with_f1 ? bl_binomial(rng, y, w.rho) : y;
                const size_t ov = (((size_t)(n - p.n0) * J + j) * T + t) * N + i;
                if (p.true_mean) p.true_mean[ov] = q * w.y * w.rho;
                if (p.true_count) p.true_count[ov] = zn ? real : 0;
            }
        }
    }
}

extern "C" int bl_launch_count_posterior(const BlCountPostParams *p, int grid_y, hipStream_t st)
{
    dim3 grid, block;
    post_geometry(p->N, grid_y, grid, block);
    hipLaunchKernelGGL(bl_count_posterior_kernel, grid, block, 0, st, *p);
    return (int)hipGetLastError();
}
