// predictive_check.hip -- the kernels of bl_predictive_check: the posterior predictive check's two discrepancies per posterior draw
// (biolith/evaluation/posterior_predictive_check.py:17-160), without the replicate-level arrays it is stated on.
//   y_rep = bl_predict's replicate, regenerated: the cell's generator (bl_cell_rng), z first, one uniform per visit, through the
//           statements bl_predict_kernel calls (predict_math.hpp: occu, false positives, random effects) -- bit for bit its y
//   E     = (double)psi (double)p, psi and p the float32 values of bl_deterministic (the same calls into predict_math.hpp):
//           the product of two float32 is exact in float64, so E is what the host check forms from predict()'s arrays
//   seen  = the caller's observation is not 255; nothing else masks
//   ft(o, e) = (sqrt o - sqrt e)^2,  chi(o, e) = (o - e)^2 / (e + 1e-10),  float64
// by site:    o, y_rep and E are summed over the site's seen visits, then the statistic, then the sum over sites
// by revisit: y_rep and E of revisit (t, j) are summed over its seen sites, then the statistic, then the sum over (t, j)
//
// First kernel: one thread per site, 256-thread blocks, the draws on grid.y.  A block reduces in a fixed order -- the wave64 in registers
// (__shfl_down), its four waves through LDS -- and writes one partial per (draw, block): the four site statistics, and per (t, j) the
// replicate count (an integer) and the sum of E.  Second kernel: one thread per draw adds the blocks' partials in block order and applies
// the revisit statistics.  No floating-point atomic anywhere: two runs give the same bits.  Nothing of size (n, J, T, N) exists.
#include "predictive_check.hpp"

#include "predict_math.hpp"

namespace {

constexpr int PC_WAVES = BL_PC_THREADS / 64;

__device__ __forceinline__ double pc_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v; // lane 0: the wave's sum, in one fixed order
}
__device__ __forceinline__ int pc_wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
__device__ __forceinline__ double pc_ft(double o, double e)
{
    const double d = sqrt(o) - sqrt(e);
    return d * d;
}
__device__ __forceinline__ double pc_chi(double o, double e)
{
    const double d = o - e;
    return d * d / (e + 1e-10);
}

} // namespace

__global__ __launch_bounds__(BL_PC_THREADS) void bl_predictive_check_kernel(const BlPredCheckParams p)
{
    __shared__ double sh_e[2][PC_WAVES]; // a revisit's wave sums, two sets in turn: one barrier per revisit
    __shared__ int sh_c[2][PC_WAVES];
    __shared__ double sh_s[4][PC_WAVES]; // the four site statistics' wave sums
    const int i = blockIdx.x * BL_PC_THREADS + threadIdx.x;
    const bool live = i < p.N;           // the tail block's idle threads add zeros: every thread reaches every barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ns = p.ns, N = p.N, T = p.T, J = p.J, Ks = p.Ks, Ko = p.Ko, TJ = p.T * p.J;
    const bool by_visit = p.visit_exp != nullptr;
    int set = 0;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        const float *__restrict__ al = th + Ks + 1;
        const size_t part = (size_t)(n - p.n0) * p.n_blocks + blockIdx.x;
        float psi = 0.0f, f_c = 0.0f, f_u = 0.0f;
        if (live) {
            psi = pm_sigmoid(pm_site_eta(p.rows + i, ns, th, Ks, p.c, i));
            const float fpr = p.c.fp_mode ? pm_sigmoid(th[p.c.o_fp]) : 0.0f;
            f_c = p.c.fp_mode == 1 ? fpr : 0.0f;
            f_u = p.c.fp_mode == 2 ? fpr : 0.0f;
        }
        int s_obs = 0, s_rep = 0; // the site's seen visits: observed and replicate detections, expectation
        double s_exp = 0.0;
        for (int t = 0; t < T; t++) {
            BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, live ? i : 0);
            const int zn = live ? pm_draw_z(rng, psi) : 0;
            for (int j = 0; j < J; j++) {
                const int v = t * J + j;
                int c = 0;
                double e = 0.0;
                if (live) {
                    const float r = pm_sigmoid(pm_visit_nu(p.wraw, ns, th, al, Ko, p.c, T, J, v, i));
                    float pd = (float)zn * r;
                    if (p.c.fp_mode) pd = pm_false_positives(pd, f_c, f_u, zn);
                    const float u = rng.uniform();
                    const int o = p.obs[((size_t)j * T + t) * N + i];
                    if (o != 255) {
                        c = u < pd ? 1 : 0;
                        e = (double)psi * (double)r;
                        s_obs += o; s_rep += c; s_exp += e;
                    }
                }
                if (by_visit) {
                    const double we = pc_wave_sum(e);
                    const int wc = pc_wave_sum(c);
                    if (lane == 0) { sh_e[set][wave] = we; sh_c[set][wave] = wc; }
                    __syncthreads();
                    if (threadIdx.x == 0) {
                        double be = sh_e[set][0];
                        int bc = sh_c[set][0];
                        for (int w = 1; w < PC_WAVES; w++) { be += sh_e[set][w]; bc += sh_c[set][w]; }
                        p.visit_exp[part * TJ + v] = be;
                        p.visit_rep[part * TJ + v] = bc;
                    }
                    set ^= 1; // the next revisit writes the other set; this one is written again two barriers on
                }
            }
        }
        if (p.site_part) {
            const double o = (double)s_obs, r = (double)s_rep;
            const double st[4] = {pc_ft(o, s_exp), pc_ft(r, s_exp), pc_chi(o, s_exp), pc_chi(r, s_exp)}; // (an idle thread: 0, 0, 0, 0)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double w = pc_wave_sum(st[k]);
                if (lane == 0) sh_s[k][wave] = w;
            }
            __syncthreads();
            if (threadIdx.x < 4) {
                double b = sh_s[threadIdx.x][0];
                for (int w = 1; w < PC_WAVES; w++) b += sh_s[threadIdx.x][w];
                p.site_part[part * 4 + threadIdx.x] = b;
            }
            __syncthreads(); // (the next draw's site sums overwrite sh_s)
        }
    }
}

// one thread per draw: the blocks' partials in block order, then the revisit statistics in (t, j) order
__global__ void bl_predictive_check_finish_kernel(const BlPredCheckParams p)
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
            double e = 0.0;
            int c = 0;
            for (int b = 0; b < NB; b++) {
                e += p.visit_exp[((size_t)m * NB + b) * TJ + v];
                c += p.visit_rep[((size_t)m * NB + b) * TJ + v];
            }
            const double o = (double)p.obs_visit[v], r = (double)c;
            a[0] += pc_ft(o, e); a[1] += pc_ft(r, e); a[2] += pc_chi(o, e); a[3] += pc_chi(r, e);
        }
        for (int k = 0; k < 4; k++) p.by_revisit[(size_t)m * 4 + k] = a[k];
    }
}

extern "C" int bl_launch_predictive_check(const BlPredCheckParams *p, int grid_y, hipStream_t st)
{
    hipLaunchKernelGGL(bl_predictive_check_kernel, dim3(p->n_blocks, grid_y), dim3(BL_PC_THREADS), 0, st, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const int n = p->n1 - p->n0;
    hipLaunchKernelGGL(bl_predictive_check_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, *p);
    return (int)hipGetLastError();
}
