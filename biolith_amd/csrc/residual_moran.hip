// residual_moran.hip -- the kernels of bl_residual_moran: per posterior draw and period, Moran's I of the occupancy and the site-level
// detection residuals of Wright, Irvine and Higgs (2019) over a sparse neighbour graph, each next to the same statistic of a replicate
// drawn from the model, and the residuals' means over the draws per site (BUILDER-DEFINED: the reference ships the residuals,
// evaluation/residuals.py, and leaves the statistic to its users; the definition is the comment of bl_residual_moran in
// include/biolith_hip.h, its NumPy restatement tests/moran_ref.py).
//
// A cell's four values (rm_cell) are other entries' values, restated by calling what they call:
//   z        bl_site_posterior's: site_cell.hpp's conditional q, the first uniform of the cell's generator for `seed` against it
//   psi, p   bl_deterministic's: predict_math.hpp
//   z', y'   bl_predict's for `seed_rep`: the cell's generator consumed in bl_predict_kernel's order (predictive_check.hip)
//   seen, y  the handle's sign-folded record: c = 0 masked, c > 0 a detection
// Nothing of size (draws, visits, sites) exists; what does exist per (draw of a chunk, period, site) is the 32-byte record of the four
// values the gather reads (residual_moran.hpp).
//
// Moran side, four kernels a chunk, 256-thread blocks over the sites, the draws on grid.y with the strided loop of the predict kernels:
//   1 values  one thread per site: the record, and per field the wave's sum, count, max and min of the masked values
//   2 means   one thread per (draw, period, field): the waves' partials in wave order -> M, mu; mu = NaN where M < 2 or max == min
//   3 gather  one thread per site walks its CSR row in order: s = sum_e w_e m_j c_j, W_i = sum_e w_e m_j; the wave's sums of
//             m_i c_i s, m_i c_i^2 and m_i W_i.  A neighbour's record is ONE 32-byte sector whatever the field: the irregular read of
//             this file costs one transaction an edge, and the graph's own arrays are read in row order
//   4 finish  one thread per (draw, period, field): the waves' partials in wave order -> I = (M / W) num / den
// Every sum over sites is regional_totals.hip's: the wave's __shfl_down tree over 32, 16, .. 1 lanes, a lane outside the mask or past
// the last site holding -0.0, the identity of the float64 sum; then the waves in order.  Products and sums are a statement each:
// -ffp-contract=on fuses nothing across statements.  No atomics, no LDS: a draw's values are a function of the draw, the handle and the
// graph -- not of the chunking, of the launch or of the outputs asked for --, and two calls return the same bytes.
//
// Site side (bl_residual_moran_site_kernel): one thread per (period, site) over ALL the draws in ascending order, float64
// accumulators in registers (species_richness.hip's site side); the replicate is not formed.
#include "residual_moran.hpp"

#include "predict_math.hpp"
#include "site_cell.hpp"

namespace {

constexpr int F = BL_RM_FIELDS;

__device__ __forceinline__ double rm_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v; // (lane 0's)
}
__device__ __forceinline__ double rm_wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o));
    return v;
}
__device__ __forceinline__ double rm_wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o));
    return v;
}
__device__ __forceinline__ double rm_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// what a draw fixes for a site: the conditional's scalars, predict's psi and false-positive rates
struct RmSite {
    SiteCellPrior prior;
    float psi, f_c, f_u;
};
__device__ __forceinline__ RmSite rm_site(const BlResidualMoranParams &p, const float *__restrict__ th, int i)
{
    RmSite s;
    s.prior = sc_prior<true>(p.rows, p.ns, i, p.Ks, th, p.c);
    s.psi = pm_sigmoid(pm_site_eta(p.rows + i, p.ns, th, p.Ks, p.c, i));
    const float fpr = p.c.fp_mode ? pm_sigmoid(th[p.c.o_fp]) : 0.0f;
    s.f_c = p.c.fp_mode == BL_FP_CONSTANT ? fpr : 0.0f;
    s.f_u = p.c.fp_mode == BL_FP_UNOCCUPIED ? fpr : 0.0f;
    return s;
}

// The four values of cell (draw n, period t, site i); NaN = outside the field's mask.  REP = false: fields 1 and 3 are not formed.
template <bool REP>
__device__ __forceinline__ void rm_cell(const BlResidualMoranParams &p, const float *__restrict__ th, const RmSite &s, int n, int t, int i,
                                        double (&v)[F])
{
    const int ns = p.ns, T = p.T, J = p.J;
    float l, q;
    sc_cell(p.rows, ns, i, T, t, p.a, th, p.c, s.prior, l, q);
    BlPredRng rng = bl_cell_rng(p.seed, n, T, t, p.N, i);
    const int z = rng.uniform() < q ? 1 : 0; // bl_site_posterior_kernel's statement
    const double psi = (double)s.psi;
    v[0] = (double)z - psi;
    BlPredRng rep = bl_cell_rng(p.seed_rep, n, T, t, p.N, i);
    int zr = 0;
    v[1] = rm_nan();
    if constexpr (REP) {
        zr = pm_draw_z(rep, s.psi);
        v[1] = (double)zr - psi;
    }
    const float *__restrict__ al = th + p.Ks + 1;
    int seen = 0;
    double so = 0.0, sr = 0.0;
    for (int j = 0; j < J; j++) {
        const int vis = t * J + j;
        const float r = pm_sigmoid(pm_visit_nu(p.wraw, ns, th, al, p.Ko, p.c, T, J, vis, i));
        int yr = 0;
        if constexpr (REP) { // bl_predict_kernel's statements: every visit takes its uniform, seen or not
            float pd = (float)zr * r;
            if (p.c.fp_mode) pd = pm_false_positives(pd, s.f_c, s.f_u, zr);
            const float u = rep.uniform();
            yr = u < pd ? 1 : 0;
        }
        const float cc = p.rows[(size_t)(p.a.r0 + vis * p.a.vw) * ns + i];
        if (cc == 0.0f) continue; // masked
        seen++;
        const double pj = (double)r;
        const double to = (cc > 0.0f ? 1.0 : 0.0) - pj;
        so += to;
        if constexpr (REP) {
            const double tr = (double)yr - pj;
            sr += tr;
        }
    }
    v[2] = z == 1 && seen > 0 ? so / (double)seen : rm_nan();
    v[3] = REP && zr == 1 && seen > 0 ? sr / (double)seen : rm_nan();
}

} // namespace

__global__ __launch_bounds__(BL_RM_THREADS) void bl_residual_moran_values_kernel(const BlResidualMoranParams p)
{
    const int i0 = blockIdx.x * BL_RM_THREADS + threadIdx.x;
    const int wave = i0 >> 6, lane = threadIdx.x & 63;
    if (wave >= p.n_waves) return; // (whole waves leave)
    const bool live = i0 < p.N;
    const int i = live ? i0 : 0; // a lane past the last site computes site 0's values and contributes identities: it takes every shuffle
    const int T = p.T;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        const RmSite s = rm_site(p, th, i);
        for (int t = 0; t < T; t++) {
            const size_t cell = (size_t)(n - p.n0) * T + t;
            double v[F];
            rm_cell<true>(p, th, s, n, t, i, v);
            if (live) {
                double2 *__restrict__ rec = reinterpret_cast<double2 *>(p.val + (cell * p.N + i) * F);
                rec[0] = make_double2(v[0], v[1]);
                rec[1] = make_double2(v[2], v[3]);
            }
            double *__restrict__ part = p.part1 + (cell * p.n_waves + wave) * (F * 4);
#pragma unroll
            for (int f = 0; f < F; f++) {
                const bool m = live && v[f] == v[f];
                const double sum = rm_wave_sum(m ? v[f] : -0.0);
                const double cnt = rm_wave_sum(m ? 1.0 : 0.0); // (integers: exact in any order)
                const double mx = rm_wave_max(m ? v[f] : -HUGE_VAL);
                const double mn = rm_wave_min(m ? v[f] : HUGE_VAL);
                if (lane == 0) { part[f * 4] = sum; part[f * 4 + 1] = cnt; part[f * 4 + 2] = mx; part[f * 4 + 3] = mn; }
            }
        }
    }
}

// stat[cell][f] = (M, mu): the waves' partials in wave order; mu = NaN where the field has no I (M < 2, or max == min)
__global__ __launch_bounds__(64) void bl_residual_moran_means_kernel(const BlResidualMoranParams p)
{
    const size_t q = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= (size_t)(p.n1 - p.n0) * p.T * F) return;
    const size_t cell = q / F;
    const int f = (int)(q % F);
    const double *__restrict__ part = p.part1 + cell * p.n_waves * (F * 4) + f * 4;
    double sum = part[0], cnt = part[1], mx = part[2], mn = part[3];
#pragma unroll 8
    for (int w = 1; w < p.n_waves; w++) {
        const double *__restrict__ pw = part + (size_t)w * (F * 4);
        sum += pw[0];
        cnt += pw[1];
        mx = fmax(mx, pw[2]);
        mn = fmin(mn, pw[3]);
    }
    const double mu = sum / cnt;
    p.stat[q * 2] = cnt;
    p.stat[q * 2 + 1] = cnt < 2.0 || mx == mn ? rm_nan() : mu;
}

__global__ __launch_bounds__(BL_RM_THREADS) void bl_residual_moran_gather_kernel(const BlResidualMoranParams p)
{
    const int i0 = blockIdx.x * BL_RM_THREADS + threadIdx.x;
    const int wave = i0 >> 6, lane = threadIdx.x & 63;
    if (wave >= p.n_waves) return;
    const bool live = i0 < p.N;
    const int i = live ? i0 : 0;
    const int T = p.T, N = p.N;
    const int e0 = live ? p.nbr_ptr[i] : 0, e1 = live ? p.nbr_ptr[i + 1] : 0; // (a lane past the last site walks no row)
    const int *__restrict__ idx = p.nbr_idx;
    const double *__restrict__ nw = p.nbr_w;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        for (int t = 0; t < T; t++) {
            const size_t cell = (size_t)(n - p.n0) * T + t;
            const double2 *__restrict__ val = reinterpret_cast<const double2 *>(p.val + cell * N * F);
            const double *__restrict__ st = p.stat + cell * (F * 2);
            double mu[F], v[F], s[F], W[F];
#pragma unroll
            for (int f = 0; f < F; f++) { mu[f] = st[f * 2 + 1]; s[f] = 0.0; W[f] = 0.0; }
            {
                const double2 a = val[(size_t)i * 2], b = val[(size_t)i * 2 + 1];
                v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
            }
            for (int e = e0; e < e1; e++) {
                const int j = idx[e];
                const double w = nw ? nw[e] : 1.0;
                const double2 a = val[(size_t)j * 2], b = val[(size_t)j * 2 + 1]; // the neighbour's record: one 32-byte sector
                const double vj[F] = {a.x, a.y, b.x, b.y};
#pragma unroll
                for (int f = 0; f < F; f++) {
                    if (vj[f] == vj[f]) { // m_j
                        const double cj = vj[f] - mu[f];
                        const double term = w * cj;
                        s[f] += term;
                        W[f] += w;
                    }
                }
            }
            double *__restrict__ part = p.part3 + (cell * p.n_waves + wave) * (F * 3);
#pragma unroll
            for (int f = 0; f < F; f++) {
                const bool m = live && v[f] == v[f];
                const double ci = v[f] - mu[f];
                const double num_i = ci * s[f];
                const double den_i = ci * ci;
                const double num = rm_wave_sum(m ? num_i : -0.0);
                const double den = rm_wave_sum(m ? den_i : -0.0);
                const double Wf = rm_wave_sum(m ? W[f] : -0.0);
                if (lane == 0) { part[f * 3] = num; part[f * 3 + 1] = den; part[f * 3 + 2] = Wf; }
            }
        }
    }
}

// I = (M / W) num / den of every (draw, period, field): the waves' partials in wave order
__global__ __launch_bounds__(64) void bl_residual_moran_finish_kernel(const BlResidualMoranParams p)
{
    const size_t q = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= (size_t)(p.n1 - p.n0) * p.T * F) return;
    const size_t cell = q / F;
    const int f = (int)(q % F);
    const double M = p.stat[q * 2], mu = p.stat[q * 2 + 1];
    if (f >= 2 && p.det_sites) p.det_sites[cell * 2 + (f - 2)] = (int)M;
    double *__restrict__ out = f < 2 ? p.moran_occ : p.moran_det;
    if (!out) return;
    const double *__restrict__ part = p.part3 + cell * p.n_waves * (F * 3) + f * 3;
    double num = part[0], den = part[1], W = part[2];
#pragma unroll 8
    for (int w = 1; w < p.n_waves; w++) {
        const double *__restrict__ pw = part + (size_t)w * (F * 3);
        num += pw[0];
        den += pw[1];
        W += pw[2];
    }
    const double I = (M / W) * num / den;
    out[cell * 2 + (f & 1)] = mu != mu || W == 0.0 ? rm_nan() : I;
}

__global__ __launch_bounds__(BL_RM_THREADS) void bl_residual_moran_site_kernel(const BlResidualMoranParams p)
{
    const size_t q = (size_t)blockIdx.x * BL_RM_THREADS + threadIdx.x;
    if (q >= (size_t)p.T * p.N) return; // (no lane waits for another)
    const int t = (int)(q / p.N), i = (int)(q % p.N);
    double osum = 0.0, dsum = 0.0;
    int occupied = 0;
    for (int n = 0; n < p.n_draws; n++) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        const RmSite s = rm_site(p, th, i);
        double v[F];
        rm_cell<false>(p, th, s, n, t, i, v);
        osum += v[0];
        if (v[2] == v[2]) { occupied++; dsum += v[2]; }
    }
    if (p.occ_mean) p.occ_mean[q] = osum / (double)p.n_draws;
    if (p.det_mean) p.det_mean[q] = occupied ? dsum / (double)occupied : rm_nan();
    if (p.n_occupied) p.n_occupied[q] = occupied;
}

extern "C" int bl_launch_residual_moran(const BlResidualMoranParams *p, int grid_y, hipStream_t st)
{
    const dim3 sites((p->N + BL_RM_THREADS - 1) / BL_RM_THREADS, grid_y);
    const size_t fields = (size_t)(p->n1 - p->n0) * p->T * F;
    const dim3 per_field((unsigned)((fields + 63) / 64));
    hipLaunchKernelGGL(bl_residual_moran_values_kernel, sites, dim3(BL_RM_THREADS), 0, st, *p);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(bl_residual_moran_means_kernel, per_field, dim3(64), 0, st, *p);
    if ((rc = (int)hipGetLastError())) return rc;
    if (p->moran_occ || p->moran_det) { // (det_sites alone: M is the means kernel's)
        hipLaunchKernelGGL(bl_residual_moran_gather_kernel, sites, dim3(BL_RM_THREADS), 0, st, *p);
        if ((rc = (int)hipGetLastError())) return rc;
    }
    hipLaunchKernelGGL(bl_residual_moran_finish_kernel, per_field, dim3(64), 0, st, *p);
    return (int)hipGetLastError();
}

extern "C" int bl_launch_residual_moran_site(const BlResidualMoranParams *p, hipStream_t st)
{
    const size_t cells = (size_t)p->T * p->N;
    hipLaunchKernelGGL(bl_residual_moran_site_kernel, dim3((unsigned)((cells + BL_RM_THREADS - 1) / BL_RM_THREADS)), dim3(BL_RM_THREADS), 0,
                       st, *p);
    return (int)hipGetLastError();
}
