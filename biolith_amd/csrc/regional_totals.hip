// regional_totals.hip -- the kernels of bl_regional_totals: per posterior draw and region, the weighted total of the first deterministic
// site (psi; occu_rn, nmixture: abundance) and, per period, of the latent state bl_predict / bl_predict_counts / bl_predict_scores draw
// for the same seed (BUILDER-DEFINED, the reference's users reduce predict()'s arrays on the host; the definition is the comment of
// bl_regional_totals in include/biolith_hip.h, its NumPy restatement tests/totals_ref.py).
//
// One thread per slot of the host's padded layout (regional_totals.hpp), 256-thread blocks, the draws on grid.y with the strided loop of
// the predict kernels.  A thread gathers its site's covariates and weight through the slot's index once and keeps them in registers; a
// draw's coefficients are wave-uniform reads.  Nothing of size (draws, sites) exists: a site's value under draw n is the very calls into
// predict_math.hpp that bl_psi_kernel and the predict kernels make -- so its bits are theirs, the generator keyed by the ORIGINAL site
// index --, multiplied by the weight in float64 and reduced at once:
//   1  a wave serves one region: its 64 terms are summed by __shfl_down over 32, 16, .. 1 lanes, one fixed tree; an idle lane holds
//      -0.0, the identity of the float64 sum (x + -0.0 = x for every x, -0.0 included), so a region of one site returns its term's bits;
//      lane 0 writes the wave's partial
//   2  the finish kernel, one thread per (draw, output row, region), adds the region's partials in wave order.
// No atomics, no LDS: a region's row is a function of its own sites in site order, their weights and the draws -- not of the other
// regions, of the chunking of the draws or of the outputs asked for --, and two calls return the same bytes.
#include "regional_totals.hpp"

#include "predict_math.hpp"

namespace {

__device__ __forceinline__ double rt_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v; // (lane 0's)
}

} // namespace

__global__ __launch_bounds__(BL_RT_THREADS) void bl_regional_totals_kernel(const BlRegionalTotalsParams p)
{
    const int slot = blockIdx.x * BL_RT_THREADS + threadIdx.x;
    if (slot >= p.n_slots) return; // (n_slots is a multiple of 64: whole waves leave)
    const int wave = slot >> 6, lane = threadIdx.x & 63;
    const int site = p.slot_site[slot];
    const bool live = site >= 0;
    const int i = live ? site : 0; // an idle lane computes site 0's value and contributes -0.0: every lane takes every shuffle
    const int ns = p.ns, N = p.N, T = p.T, Ks = p.Ks, model = p.model, rows = p.site_rows + p.latent_rows;
    const BlDrawCoords c = p.c;
    const double w = live && p.slot_w ? p.slot_w[slot] : 1.0;
    float x[BL_MAX_COVS];
    for (int k = 0; k < Ks; k++) x[k] = p.rows[(size_t)k * ns + i];
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *th = p.draws + (size_t)n * p.D;
        double *part = p.part + (size_t)(n - p.n0) * rows * p.n_waves + wave;
        const float eta = pm_site_eta(x, 1, th, Ks, c, i);
        if (p.site_rows) {
            // bl_psi_kernel's statement: occu psi = sigmoid(eta); occu_rn, nmixture: abundance = exp(eta)
            const float v = (model == 1 || model == 4) ? __expf(eta) : pm_sigmoid(eta);
            const double sum = rt_wave_sum(live ? w * (double)v : -0.0);
            if (lane == 0) part[0] = sum;
        }
        if (!p.latent_rows) continue;
        // bl_predict_scores_kernel forms psi from the covariates' predictor alone; the other two from eta
        const float psi = p.scores ? pm_sigmoid(pm_linear(x, 1, th, Ks)) : pm_sigmoid(eta);
        for (int t = 0; t < T; t++) {
            BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, i);
            const int zn = (model == 1 || model == 4) ? pm_draw_abundance(rng, eta, p.K) : pm_draw_z(rng, psi);
            const double sum = rt_wave_sum(live ? w * (double)zn : -0.0);
            if (lane == 0) part[(size_t)(p.site_rows + t) * p.n_waves] = sum;
        }
    }
}

// total[dn][row][g] = the partials of region g's waves, added in wave order; a region without a site: 0
__global__ __launch_bounds__(BL_RT_THREADS) void bl_regional_totals_finish_kernel(const BlRegionalTotalsParams p)
{
    const int rows = p.site_rows + p.latent_rows, G = p.n_regions;
    const size_t q = (size_t)blockIdx.x * BL_RT_THREADS + threadIdx.x;
    if (q >= (size_t)(p.n1 - p.n0) * rows * G) return;
    const int g = (int)(q % G), r = (int)(q / G % rows);
    const size_t dn = q / G / rows;
    const int w0 = p.wave_first[g], w1 = p.wave_first[g + 1];
    const double *part = p.part + (dn * rows + r) * p.n_waves;
    double sum = w0 < w1 ? part[w0] : 0.0;
    for (int wv = w0 + 1; wv < w1; wv++) sum += part[wv];
    if (r < p.site_rows) p.site_total[dn * G + g] = sum;
    else p.latent_total[(dn * p.T + (r - p.site_rows)) * G + g] = sum;
}

extern "C" int bl_launch_regional_totals(const BlRegionalTotalsParams *p, int grid_y, hipStream_t st)
{
    const int rows = p->site_rows + p->latent_rows;
    if (p->n_slots > 0) { // (every site in no region: the totals are the finish kernel's zeros)
        hipLaunchKernelGGL(bl_regional_totals_kernel, dim3((p->n_slots + BL_RT_THREADS - 1) / BL_RT_THREADS, grid_y), dim3(BL_RT_THREADS),
                           0, st, *p);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    const size_t cells = (size_t)(p->n1 - p->n0) * rows * p->n_regions;
    hipLaunchKernelGGL(bl_regional_totals_finish_kernel, dim3((unsigned)((cells + BL_RT_THREADS - 1) / BL_RT_THREADS)), dim3(BL_RT_THREADS),
                       0, st, *p);
    return (int)hipGetLastError();
}
