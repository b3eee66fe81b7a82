// predictive_check_counts.hip -- the kernels of bl_predictive_check_counts: the posterior predictive check's two discrepancies per
// posterior draw for occu_rn, nmixture and occu_cop (BUILDER-DEFINED: the reference's check is occu's), without the replicate-level
// arrays it is stated on.
//   y_rep = bl_predict's (occu_rn) / bl_predict_counts' (nmixture, occu_cop) replicate, regenerated: the cell's generator (bl_cell_rng),
//           the latent state first, then EVERY visit in j order, seen or not (a Binomial takes N uniforms, a Poisson a data-dependent
//           number: a skipped visit would shift every later one), through the statements those kernels call (predict_math.hpp)
//   E     = the model's mean of y_itj with the latent state summed out, float64, from the float32 sites of bl_deterministic
//           (lambda = abundance, p = prob_detection, psi, rate = rate_detection: the same calls into predict_math.hpp):
//             nmixture  E = m p,  m = sum n w_n / sum w_n,  w_n = lambda^n / n!  over n = 0 .. K
//             occu_rn   E = 1 - (1 - f) sum w_n (1 - p)^n / sum w_n
//             occu_cop  E = dur (psi rate + (1 - psi) f_u + f_c)
//           f the float32 site value of the draw's coordinate phi: (float)(1 / (1 + exp(-(double)phi))) (occu_rn), (float)exp((double)phi)
//           (occu_cop) -- the host cannot restate __expf; the REPLICATE keeps bl_predict*'s own rate, __expf included
//   seen  = the caller's observation is not negative; nothing else masks
//   ft(o, e) = (sqrt o - sqrt e)^2,  chi(o, e) = (o - e)^2 / (e + 1e-10),  float64
// by site:    o, y_rep and E are summed over the site's seen visits, then the statistic, then the sum over sites
// by revisit: y_rep and E of revisit (t, j) are summed over its seen sites, then the statistic, then the sum over (t, j)
//
// The kernels' shape is predictive_check.hip's.  First kernel: one thread per site, 256-thread blocks, the draws on grid.y.  A block
// reduces in a fixed order -- the wave64 in registers (__shfl_down), its four waves through LDS -- and writes one partial per (draw,
// block): the four site statistics, and per (t, j) the replicate total and the sum of E.  Counts are summed as float64: integers below
// 2^53 add exactly in any order (a revisit's total over 10^4 sites at a high rate does not fit 32 bits safely).  Second kernel: one thread
// per draw adds the blocks' partials in block order and applies the revisit statistics.  No floating-point atomic anywhere: two runs give
// the same bits.  Nothing of size (n, J, T, N) exists.
#include "predictive_check_counts.hpp"

#include <cfloat>

#include "predict_math.hpp"

namespace {

constexpr int PCC_WAVES = BL_PCC_THREADS / 64;

__device__ __forceinline__ double pcc_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v; // lane 0: the wave's sum, in one fixed order
}
__device__ __forceinline__ double pcc_ft(double o, double e)
{
    const double d = sqrt(o) - sqrt(e);
    return d * d;
}
__device__ __forceinline__ double pcc_chi(double o, double e)
{
    const double d = o - e;
    return d * d / (e + 1e-10);
}

// The sums over Poisson(lambda) restricted to 0 .. K, with w_n = lambda^n / n! by the recursion w_n = w_{n-1} lambda / n from w_0 = 1: the
// common factor exp(-lambda) cancels in every ratio and is never formed.  lambda^n / n! overflows float64 (lambda = 3e4, K = 100), so
// whenever the running term passes 1e100 every accumulator is scaled by 1e-200: a term grows by at most lambda <= FLT_MAX a step, so
// nothing passes 1e139, and what a scaling flushes to zero is below 1e-200 of the largest term.  Finite for any float32 lambda (an
// infinite one reads as FLT_MAX) and any K.
constexpr double PCC_BIG = 1e100, PCC_DOWN = 1e-200;

// m(lambda, K) = sum n w_n / sum w_n: the mean of the restricted Poisson
__device__ __forceinline__ double pcc_trunc_mean(double lam, int K)
{
    double w = 1.0, a = 1.0, b = 0.0;
    for (int n = 1; n <= K; n++) {
        w *= lam / (double)n;
        a += w;
        b += (double)n * w;
        if (w > PCC_BIG) { w *= PCC_DOWN; a *= PCC_DOWN; b *= PCC_DOWN; }
    }
    return b / a;
}
// sum w_n q^n / sum w_n: the restricted Poisson's probability generating function at q
__device__ __forceinline__ double pcc_trunc_pgf(double lam, double q, int K)
{
    double w = 1.0, v = 1.0, a = 1.0, b = 1.0;
    for (int n = 1; n <= K; n++) {
        const double r = lam / (double)n;
        w *= r;
        v *= r * q;
        a += w;
        b += v;
        if (w > PCC_BIG) { w *= PCC_DOWN; v *= PCC_DOWN; a *= PCC_DOWN; b *= PCC_DOWN; }
    }
    return b / a;
}

} // namespace

__global__ __launch_bounds__(BL_PCC_THREADS) void bl_predictive_check_counts_kernel(const BlPredCheckCountsParams p)
{
    __shared__ double sh_e[2][PCC_WAVES]; // a revisit's wave sums, two sets in turn: one barrier per revisit
    __shared__ double sh_c[2][PCC_WAVES];
    __shared__ double sh_s[4][PCC_WAVES]; // the four site statistics' wave sums
    const int i = blockIdx.x * BL_PCC_THREADS + threadIdx.x;
    const bool live = i < p.N;            // the tail block's idle threads add zeros: every thread reaches every barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ns = p.ns, N = p.N, T = p.T, J = p.J, Ks = p.Ks, Ko = p.Ko, TJ = p.T * p.J, model = p.model, K = p.K;
    const bool by_visit = p.visit_exp != nullptr;
    int set = 0;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        const float *__restrict__ al = th + Ks + 1;
        const size_t part = (size_t)(n - p.n0) * p.n_blocks + blockIdx.x;
        // the draw's false-positive rate: as the predict kernels form it (the replicate's), and as the layout's transform gives the
        // site (E's)
        float rep_f = 0.0f, site_f = 0.0f;
        if (p.c.fp_mode) {
            const float phi = th[p.c.o_fp];
            rep_f = model == 3 ? pm_cop_fp_rate(phi) : pm_sigmoid(phi);
            site_f = model == 3 ? (float)exp((double)phi) : (float)(1.0 / (1.0 + exp(-(double)phi)));
        }
        const float rep_fc = p.c.fp_mode == 1 ? rep_f : 0.0f, rep_fu = p.c.fp_mode == 2 ? rep_f : 0.0f; // (occu_cop's two modes)
        const double e_fc = p.c.fp_mode == 1 ? (double)site_f : 0.0, e_fu = p.c.fp_mode == 2 ? (double)site_f : 0.0;
        float eta = 0.0f;
        double lam = 0.0, psi = 0.0, mean_n = 0.0; // bl_deterministic's site of the draw: abundance (occu_rn, nmixture) or psi (occu_cop)
        if (live) {
            eta = pm_site_eta(p.rows + i, ns, th, Ks, p.c, i);
            if (model == 3) {
                psi = (double)pm_sigmoid(eta);
            } else {
                lam = fmin((double)__expf(eta), (double)FLT_MAX);
                if (model == 4) mean_n = pcc_trunc_mean(lam, K);
            }
        }
        double s_obs = 0.0, s_rep = 0.0, s_exp = 0.0; // the site's seen visits: observed and replicate totals, expectation
        for (int t = 0; t < T; t++) {
            BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, live ? i : 0);
            int zn = 0;
            if (live) zn = model == 3 ? pm_draw_z(rng, pm_sigmoid(eta)) : pm_draw_abundance(rng, eta, K);
            for (int j = 0; j < J; j++) {
                const int v = t * J + j;
                double c = 0.0, e = 0.0;
                if (live) {
                    const float nu = pm_visit_nu(p.wraw, ns, th, al, Ko, p.c, T, J, v, i);
                    int cnt;
                    double ev;
                    if (model == 4) {        // nmixture
                        const float r = pm_sigmoid(nu);
                        cnt = bl_binomial(rng, zn, r);
                        ev = mean_n * (double)r;
                    } else if (model == 1) { // occu_rn
                        const float r = pm_sigmoid(nu);
                        float pd = pm_rn_detection(r, zn);
                        pd = pm_rn_false_positives(pd, rep_f);
                        cnt = rng.uniform() < pd ? 1 : 0;
                        const double miss = (1.0 - (double)site_f) * pcc_trunc_pgf(lam, 1.0 - (double)r, K);
                        ev = 1.0 - miss;
                    } else {                 // occu_cop
                        const float d = p.dur[(size_t)v * ns + i];
                        cnt = bl_poisson(rng, pm_cop_rate(d, zn, nu, rep_fu, rep_fc));
                        const double occupied = psi * (double)__expf(nu);
                        const double empty = (1.0 - psi) * e_fu;
                        const double both = occupied + empty;
                        ev = (double)d * (both + e_fc);
                    }
                    const int o = p.obs[((size_t)j * T + t) * N + i];
                    if (o >= 0) {
                        c = (double)cnt;
                        e = ev;
                        s_obs += (double)o; s_rep += c; s_exp += e;
                    }
                }
                if (by_visit) {
                    const double we = pcc_wave_sum(e), wc = pcc_wave_sum(c);
                    if (lane == 0) { sh_e[set][wave] = we; sh_c[set][wave] = wc; }
                    __syncthreads();
                    if (threadIdx.x == 0) {
                        double be = sh_e[set][0], bc = sh_c[set][0];
                        for (int w = 1; w < PCC_WAVES; w++) { be += sh_e[set][w]; bc += sh_c[set][w]; }
                        p.visit_exp[part * TJ + v] = be;
                        p.visit_rep[part * TJ + v] = bc;
                    }
                    set ^= 1; // the next revisit writes the other set; this one is written again two barriers on
                }
            }
        }
        if (p.site_part) {
            const double st[4] = {pcc_ft(s_obs, s_exp), pcc_ft(s_rep, s_exp), pcc_chi(s_obs, s_exp), pcc_chi(s_rep, s_exp)}; // (an idle thread: 0, 0, 0, 0)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double w = pcc_wave_sum(st[k]);
                if (lane == 0) sh_s[k][wave] = w;
            }
            __syncthreads();
            if (threadIdx.x < 4) {
                double b = sh_s[threadIdx.x][0];
                for (int w = 1; w < PCC_WAVES; w++) b += sh_s[threadIdx.x][w];
                p.site_part[part * 4 + threadIdx.x] = b;
            }
            __syncthreads(); // (the next draw's site sums overwrite sh_s)
        }
    }
}

// one thread per draw: the blocks' partials in block order, then the revisit statistics in (t, j) order
__global__ void bl_predictive_check_counts_finish_kernel(const BlPredCheckCountsParams p)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= p.n1 - p.n0) return;
    const int NB = p.n_blocks, TJ = p.T * p.J;
    if (p.by_site) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < NB; b++)
            for (int k = 0; k < 4; k++) a[k] += p.site_part[((size_t)m * NB + b) * 4 + k];
        for (int k = 0; k < 4; k++) p.by_site[(size_t)m * 4 + k] = a[k];
    }
    if (p.by_revisit) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int v = 0; v < TJ; v++) {
            double e = 0.0, r = 0.0;
            for (int b = 0; b < NB; b++) {
                e += p.visit_exp[((size_t)m * NB + b) * TJ + v];
                r += p.visit_rep[((size_t)m * NB + b) * TJ + v];
            }
            const double o = p.obs_visit[v];
            a[0] += pcc_ft(o, e); a[1] += pcc_ft(r, e); a[2] += pcc_chi(o, e); a[3] += pcc_chi(r, e);
        }
        for (int k = 0; k < 4; k++) p.by_revisit[(size_t)m * 4 + k] = a[k];
    }
}

extern "C" int bl_launch_predictive_check_counts(const BlPredCheckCountsParams *p, int grid_y, hipStream_t st)
{
    hipLaunchKernelGGL(bl_predictive_check_counts_kernel, dim3(p->n_blocks, grid_y), dim3(BL_PCC_THREADS), 0, st, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const int n = p->n1 - p->n0;
    hipLaunchKernelGGL(bl_predictive_check_counts_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, *p);
    return (int)hipGetLastError();
}
