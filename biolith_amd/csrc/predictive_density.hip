// predictive_density.hip -- the kernels of bl_predictive_density: the pointwise log-likelihood of the observations under every posterior
// draw, reduced two ways without ever being stored (biolith/evaluation/log_likelihood.py:10-96 and what lppd.py, waic.py and deviance.py
// reduce it to).  Per draw n, visit (t, j) and site i, in float64:
//   psi, r = the float32 values of bl_deterministic (the same calls into predict_math.hpp)
//   conditional:  z = bl_predict's draw: the first uniform of the cell's generator (bl_cell_rng) < psi
//                 prob = z r, or with a false-positive rate f (constant: f_c = f; unoccupied: f_u = f)
//                 prob = 1 - (1 - z r)(1 - f_c)(1 - (1 - z) f_u), each product rounded once (the expression as NumPy evaluates it)
//                 f = (float)(1 / (1 + exp(-(double)phi))): the float32 site value that the layout's sigmoid transform gives the
//                 coordinate phi -- float64 exp, so that the host can restate it (__expf cannot be restated there)
//                 ll = y log(clamp(prob, FLT_MIN, 1 - FLT_EPSILON)) + (1 - y) log1p(-clamp(prob, ...))
//   marginal:     q = (double)psi (double)r (exact);  ll = y log(clip(q, 1e-10, 1 - 1e-10)) + (1 - y) log(clip(1 - q, 1e-10, 1 - 1e-10))
// y is 0 or 1 and both logarithms are finite, so the sum of the two terms is the selected one exactly.  A point is a cell whose obs byte
// is not 255; anything else contributes nothing and draws nothing.
//
// Per draw (bl_predictive_density_draws_kernel): one thread per site, 256-thread blocks, the draws on grid.y.  A thread adds its site's
// points in (t, j) order; the block reduces in a fixed order -- the wave64 in registers (__shfl_down), its four waves through LDS -- and
// writes one partial per (draw, block).  bl_predictive_density_draws_finish_kernel adds the blocks in block order.
//
// Per point (bl_predictive_density_points_kernel): one thread per cell (j, t, i), site fastest; grid.y = R strips of consecutive draws.
// A thread walks its strip in draw order and keeps in registers the running maximum m, s = sum exp(ll - m), and Welford's mean and M2;
// it writes the four once.  bl_predictive_density_points_finish_kernel merges the R strips of a cell in strip order (log-sum-exp merge;
// Chan's pairwise mean / M2 merge) and writes log mean exp = m + log s - log n and M2 / (n - 1).
//
// No floating-point atomic anywhere: two runs give the same bits.  Nothing of size (n, J, T, N) exists.
#include "predictive_density.hpp"

#include <cfloat>

#include "predict_math.hpp"

namespace {

constexpr int PD_WAVES = BL_PD_THREADS / 64;

__device__ __forceinline__ double pd_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v; // lane 0: the wave's sum, in one fixed order
}

// what of a draw is the same for every site
struct PdDraw {
    const float *th, *al;
    float f_c, f_u;
};
__device__ __forceinline__ PdDraw pd_draw(const BlPredDensityParams &p, int n)
{
    PdDraw d;
    d.th = p.draws + (size_t)n * p.D;
    d.al = d.th + p.Ks + 1;
    d.f_c = d.f_u = 0.0f;
    if (p.c.fp_mode && !p.marginal) {
        const double e = exp(-(double)d.th[p.c.o_fp]); // (float64 on purpose: see the header)
        const float f = (float)(1.0 / (1.0 + e));
        if (p.c.fp_mode == 1) d.f_c = f; else d.f_u = f;
    }
    return d;
}
__device__ __forceinline__ float pd_psi(const BlPredDensityParams &p, const PdDraw &d, int i)
{
    return pm_sigmoid(pm_site_eta(p.rows + i, p.ns, d.th, p.Ks, p.c, i));
}
__device__ __forceinline__ float pd_r(const BlPredDensityParams &p, const PdDraw &d, int i, int v)
{
    return pm_sigmoid(pm_visit_nu(p.wraw, p.ns, d.th, d.al, p.Ko, p.c, p.T, p.J, v, i));
}
__device__ __forceinline__ int pd_z(const BlPredDensityParams &p, int n, int t, int i, float psi)
{
    BlPredRng rng = bl_cell_rng(p.seed, n, p.T, t, p.N, i);
    return pm_draw_z(rng, psi);
}
__device__ __forceinline__ double pd_loglik(const BlPredDensityParams &p, const PdDraw &d, int y, float psi, float r, int zn)
{
    if (p.marginal) {
        const double q = (double)psi * (double)r;
        const double a = y ? q : 1.0 - q;
        return log(fmin(fmax(a, 1e-10), 1.0 - 1e-10));
    }
    double prob = zn ? (double)r : 0.0;
    if (p.c.fp_mode) {
        const double a = 1.0 - prob, b = 1.0 - (double)d.f_c, c = 1.0 - (zn ? 0.0 : (double)d.f_u);
        const double ab = a * b; // (a statement each: nothing contracts into an fma, the products round as on the host)
        const double abc = ab * c;
        prob = 1.0 - abc;
    }
    prob = fmin(fmax(prob, (double)FLT_MIN), (double)(1.0f - FLT_EPSILON));
    return y ? log(prob) : log1p(-prob);
}

} // namespace

__global__ __launch_bounds__(BL_PD_THREADS) void bl_predictive_density_draws_kernel(const BlPredDensityParams p)
{
    __shared__ double sh[PD_WAVES];
    const int i = blockIdx.x * BL_PD_THREADS + threadIdx.x;
    const bool live = i < p.N; // the tail block's idle threads add zeros: every thread reaches every barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = p.N, T = p.T, J = p.J;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const PdDraw d = pd_draw(p, n);
        double sum = 0.0;
        if (live) {
            const float psi = pd_psi(p, d, i);
            for (int t = 0; t < T; t++) {
                int zn = -1; // drawn at the period's first point, and not at all in the marginal form
                for (int j = 0; j < J; j++) {
                    const int y = p.obs[((size_t)j * T + t) * N + i];
                    if (y == 255) continue;
                    if (zn < 0) zn = p.marginal ? 0 : pd_z(p, n, t, i, psi);
                    sum += pd_loglik(p, d, y, psi, pd_r(p, d, i, t * J + j), zn);
                }
            }
        }
        const double w = pd_wave_sum(sum);
        if (lane == 0) sh[wave] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            double b = sh[0];
            for (int k = 1; k < PD_WAVES; k++) b += sh[k];
            p.draw_part[(size_t)(n - p.n0) * p.n_blocks + blockIdx.x] = b;
        }
        __syncthreads(); // (the next draw's wave sums overwrite sh)
    }
}

// one thread per draw: the blocks' partials in block order
__global__ void bl_predictive_density_draws_finish_kernel(const BlPredDensityParams p)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= p.n1 - p.n0) return;
    double a = 0.0;
    for (int b = 0; b < p.n_blocks; b++) a += p.draw_part[(size_t)m * p.n_blocks + b];
    p.per_draw[m] = a;
}

__global__ __launch_bounds__(BL_PD_THREADS) void bl_predictive_density_points_kernel(const BlPredDensityParams p)
{
    const size_t cells = (size_t)p.J * p.T * p.N;
    const size_t c = (size_t)blockIdx.x * BL_PD_THREADS + threadIdx.x; // = (j T + t) N + i, the observations' own order
    if (c >= cells) return;                                            // (no barrier in this kernel)
    const int q0 = bl_pd_strip_begin(p.n_draws, p.strips, blockIdx.y), q1 = bl_pd_strip_begin(p.n_draws, p.strips, blockIdx.y + 1);
    const int y = p.obs[c];
    if (y == 255 || q0 == q1) return; // not a point, or an empty strip: the finish kernel reads neither
    const int i = (int)(c % p.N), jt = (int)(c / p.N), t = jt % p.T, j = jt / p.T, v = t * p.J + j;
    double m = -INFINITY, s = 0.0, mean = 0.0, m2 = 0.0;
    for (int n = q0; n < q1; n++) {
        const PdDraw d = pd_draw(p, n);
        const float psi = pd_psi(p, d, i);
        const int zn = p.marginal ? 0 : pd_z(p, n, t, i, psi);
        const double ll = pd_loglik(p, d, y, psi, pd_r(p, d, i, v), zn);
        // streaming log-sum-exp: s = sum exp(ll - m) under the running maximum m (the first draw: s = 0 * exp(-inf) + 1)
        if (ll > m) {
            s = s * exp(m - ll) + 1.0;
            m = ll;
        } else {
            s += exp(ll - m);
        }
        // Welford
        const double delta = ll - mean;
        mean += delta / (double)(n - q0 + 1);
        m2 += delta * (ll - mean);
    }
    double *out = p.strip_part + (size_t)blockIdx.y * 4 * cells + c;
    out[0] = m; out[cells] = s; out[2 * cells] = mean; out[3 * cells] = m2;
}

// one thread per cell: the strips' partials in strip order
__global__ void bl_predictive_density_points_finish_kernel(const BlPredDensityParams p)
{
    const size_t cells = (size_t)p.J * p.T * p.N;
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cells) return;
    double lse = 0.0, var = 0.0; // what a cell that is no point gets
    if (p.obs[c] != 255) {
        double m = -INFINITY, s = 0.0, mean = 0.0, m2 = 0.0, cnt = 0.0;
        for (int r = 0; r < p.strips; r++) {
            const double k = (double)(bl_pd_strip_begin(p.n_draws, p.strips, r + 1) - bl_pd_strip_begin(p.n_draws, p.strips, r));
            if (k == 0.0) continue;
            const double *in = p.strip_part + (size_t)r * 4 * cells + c;
            const double mb = in[0], sb = in[cells], meanb = in[2 * cells], m2b = in[3 * cells];
            const double top = fmax(m, mb);
            s = s * exp(m - top) + sb * exp(mb - top);
            m = top;
            // Chan, Golub and LeVeque's pairwise merge of (cnt, mean, m2) with (k, meanb, m2b)
            const double tot = cnt + k, delta = meanb - mean;
            mean += delta * (k / tot);
            m2 += m2b + delta * delta * (cnt * k / tot);
            cnt = tot;
        }
        lse = m + log(s) - log(cnt);
        var = cnt > 1.0 ? m2 / (cnt - 1.0) : 0.0;
    }
    if (p.point_lse) p.point_lse[c] = lse;
    if (p.point_var) p.point_var[c] = var;
}

extern "C" int bl_launch_predictive_density_draws(const BlPredDensityParams *p, int grid_y, hipStream_t st)
{
    hipLaunchKernelGGL(bl_predictive_density_draws_kernel, dim3(p->n_blocks, grid_y), dim3(BL_PD_THREADS), 0, st, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const int n = p->n1 - p->n0;
    hipLaunchKernelGGL(bl_predictive_density_draws_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, *p);
    return (int)hipGetLastError();
}

extern "C" int bl_launch_predictive_density_points(const BlPredDensityParams *p, hipStream_t st)
{
    const size_t cells = (size_t)p->J * p->T * p->N;
    const unsigned blocks = (unsigned)((cells + BL_PD_THREADS - 1) / BL_PD_THREADS);
    hipLaunchKernelGGL(bl_predictive_density_points_kernel, dim3(blocks, p->strips), dim3(BL_PD_THREADS), 0, st, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(bl_predictive_density_points_finish_kernel, dim3(blocks), dim3(BL_PD_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
