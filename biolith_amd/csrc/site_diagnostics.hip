// site_diagnostics.hip -- the kernels of bl_site_diagnostics: per cell of a deterministic site, over the posterior draws of all chains,
// the effective sample size (Geyer's initial monotone sequence on the chain-averaged autocovariances) and the split R-hat of the site's
// float32 values, with bl_site_summary's mean and sd (BUILDER-DEFINED, the reference's users run numpyro.diagnostics.summary over
// predict()'s arrays on the host; the definition is the comment of bl_site_diagnostics in include/biolith_hip.h, its NumPy restatement
// tests/diagnostics_ref.py).
//
// One thread per cell, 256-thread blocks, the site fastest in a wave, as site_summary.hip: the cell's covariates are read once and stay in
// registers, a draw's coefficients are wave-uniform reads, and the value under a draw is formed anew wherever a sum wants it -- the very
// calls into predict_math.hpp that bl_psi_kernel and bl_pdet_kernel make, so its bits are bl_deterministic's.  Nothing of size (draws,
// cells) exists.  Every sum is float64 in draw order, chain after chain:
//   1  per chain the sum -> its mean, and the sums of its first and last n / 2 values -> the half chains' means; the sum over all draws
//      -> the mean.  The three means of a chain go to the thread's own slots of the workspace (they are wanted again per chain below, and
//      the chain count is not a compile-time size).
//   2  per chain the squared deviations from the three means -> W, plus and their split counterparts -> r_hat; from the overall mean ->
//      sd, in bl_site_summary's statements.
//   3  the autocovariances, by direct lagged sums, BL_SD_LAGS lags a pass (only where n_eff is wanted).  The pass of lags k0 .. k0 + L - 1
//      walks a chain once with two streams of centred values, d_t and d_{t - k0} (one stream for k0 = 0); the trailing L values of the
//      second stand in a ring, so every step is L FMAs a[l] += d_t ring[l] on independent accumulators.  The walk is unrolled L times:
//      ring and accumulators keep static register indices.
//      The ring starts at zero, which are the terms t - k < 0 of the definition that do not exist: they add +0.
//      After the pass the lane folds its L / 2 pairs into the running minimum.  Once a pair is <= 0 the minimum is 0 and every later term
//      of tau is +0: the lane's tau is settled.  A NaN tau is settled as well (0 / 0 of a cell whose values are all equal).  The wave takes
//      passes while any lane is not settled -- wave-uniform control flow --; a settled lane's value is not touched again, so the wave's pass
//      count changes nobody's result.
// Why lag blocks and not a tile of stored values: the value is some twenty instructions, against L = 32 FMAs a step; a stored tile would
// save those at the price of a workspace of (draws, tile) floats, a tiling that results must not depend on, and a read per step whose
// latency nothing hides at the one wave per SIMD this launch shape has -- as nothing hides the coefficients' reads here.  DESIGN.md has
// the numbers.
// No atomics, no LDS: a cell's outputs are a function of its covariates, its effects and the draws, not of N, the block it falls in or
// the outputs asked for, and two calls return the same bits.
#include "site_diagnostics.hpp"

#include "predict_math.hpp"

namespace {

constexpr int L = BL_SD_LAGS;
static_assert(L % 2 == 0, "a pass ends on a whole pair");

// the float32 value of the cell under draw n: site_summary.hip's ss_value, statement for statement
template <bool VISIT, int KC>
__device__ __forceinline__ float sd_value(const BlSiteDiagnosticsParams &p, const float *__restrict__ x, int i, int v, int n)
{
    const float *th = p.draws + (size_t)n * p.D;
    if (VISIT) {
        const float nu = pm_visit_nu_staged(x, th, th + p.Ks + 1, KC >= 0 ? KC : p.Ko, p.c, p.T, p.J, v, i);
        return p.model == 3 ? __expf(nu) : pm_sigmoid(nu); // occu_cop: rate_detection
    }
    const float eta = pm_site_eta(x, 1, th, KC >= 0 ? KC : p.Ks, p.c, i);
    return (p.model == 1 || p.model == 4) ? __expf(eta) : pm_sigmoid(eta); // occu_rn, nmixture: abundance
}

template <bool VISIT, int KC>
__device__ __forceinline__ void sd_cell(const BlSiteDiagnosticsParams &p)
{
    const size_t cells = VISIT ? (size_t)p.J * p.T * p.N : (size_t)p.N;
    const size_t gid = (size_t)blockIdx.x * BL_SD_THREADS + threadIdx.x, threads = (size_t)gridDim.x * BL_SD_THREADS;
    size_t cell = gid; // = (j T + t) N + i
    const bool live = cell < cells;
    if (!live) cell = cells - 1; // the tail block's idle threads redo the last cell and write nothing: every lane takes every pass
    const int i = (int)(cell % p.N), jt = (int)(cell / p.N), v = VISIT ? (jt % p.T) * p.J + jt / p.T : 0;
    const int C = p.n_chains, n = p.n, h = n / 2;
    double *__restrict__ means = p.means + gid; // [C][3][threads]: this thread's slots, its own even where it redoes a cell

    float x[BL_MAX_COVS];
    const int nk = KC >= 0 ? KC : VISIT ? p.Ko : p.Ks;
    if (VISIT) {
        for (int k = 0; k < nk; k++) x[k] = p.wraw[((size_t)v * nk + k) * p.ns + i];
    } else {
        for (int k = 0; k < nk; k++) x[k] = p.rows[(size_t)k * p.ns + i];
    }

    // ---- 1
    double sum = 0.0, sum_m = 0.0, sum_hm = 0.0;
    for (int c = 0; c < C; c++) {
        double s = 0.0, s1 = 0.0, s2 = 0.0;
        for (int t = 0; t < n; t++) {
            const float val = sd_value<VISIT, KC>(p, x, i, v, c * n + t);
            sum += (double)val;
            s += (double)val;
            s1 += t < h ? (double)val : 0.0; // (the values are >= +0: adding +0 changes no bit)
            s2 += t >= n - h ? (double)val : 0.0;
        }
        const double m = s / (double)n, h1 = s1 / (double)h, h2 = s2 / (double)h;
        means[(size_t)(3 * c) * threads] = m;
        means[(size_t)(3 * c + 1) * threads] = h1;
        means[(size_t)(3 * c + 2) * threads] = h2;
        sum_m += m;
        sum_hm += h1;
        sum_hm += h2;
    }
    const int n_draws = C * n;
    const double mean = sum / (double)n_draws;
    const double mean_m = sum_m / (double)C, mean_hm = sum_hm / (double)(2 * C);
    if (live && p.mean) p.mean[cell] = mean;

    // ---- 2
    double m2 = 0.0, w_sum = 0.0, b_sum = 0.0, wh_sum = 0.0, bh_sum = 0.0;
    for (int c = 0; c < C; c++) {
        const double mc = means[(size_t)(3 * c) * threads], mh1 = means[(size_t)(3 * c + 1) * threads], mh2 = means[(size_t)(3 * c + 2) * threads];
        double q = 0.0, q1 = 0.0, q2 = 0.0;
        for (int t = 0; t < n; t++) {
            const float val = sd_value<VISIT, KC>(p, x, i, v, c * n + t);
            const double d = (double)val - mean;
            m2 += d * d;
            const double e = (double)val - mc, e1 = (double)val - mh1, e2 = (double)val - mh2;
            q += e * e;
            q1 += t < h ? e1 * e1 : 0.0;
            q2 += t >= n - h ? e2 * e2 : 0.0;
        }
        w_sum += q / (double)(n - 1);
        wh_sum += q1 / (double)(h - 1); // (0 / 0 where a half holds one draw)
        wh_sum += q2 / (double)(h - 1);
        b_sum += (mc - mean_m) * (mc - mean_m);
        bh_sum += (mh1 - mean_hm) * (mh1 - mean_hm);
        bh_sum += (mh2 - mean_hm) * (mh2 - mean_hm);
    }
    if (live && p.sd) p.sd[cell] = sqrt(m2 / (double)(n_draws - 1));
    double W = w_sum / (double)C;
    double plus = W * (double)(n - 1) / (double)n;
    if (C > 1) plus += b_sum / (double)(C - 1);
    else W = plus;
    if (live && p.r_hat) {
        const double wh = wh_sum / (double)(2 * C);
        const double plus_h = wh * (double)(h - 1) / (double)h + bh_sum / (double)(2 * C - 1);
        p.r_hat[cell] = sqrt(plus_h / wh);
    }

    // ---- 3
    if (!p.n_eff) return; // (wave-uniform)
    const int n_pairs = n / 2;
    double tau_sum = 0.0, run = __builtin_inf();
    bool done = false;
    for (int k0 = 0; k0 < 2 * n_pairs; k0 += L) {
        if (!__any(!done)) break;
        double acc[L];
#pragma unroll
        for (int l = 0; l < L; l++) acc[l] = 0.0;
        for (int c = 0; c < C; c++) {
            const double mc = means[(size_t)(3 * c) * threads];
            const int first = c * n;
            double ring[L];
#pragma unroll
            for (int l = 0; l < L; l++) ring[l] = 0.0;
            for (int t = k0; t < n; t += L) {
#pragma unroll
                for (int j = 0; j < L; j++) {
                    if (t + j < n) { // (wave-uniform)
                        const double b = (double)sd_value<VISIT, KC>(p, x, i, v, first + t + j - k0) - mc;
                        const double a = k0 ? (double)sd_value<VISIT, KC>(p, x, i, v, first + t + j) - mc : b;
                        ring[j] = b; // d_{t + j - k0}; slot (j - l) mod L holds d_{t + j - k0 - l}, written l steps ago
#pragma unroll
                        for (int l = 0; l < L; l++) acc[l] += a * ring[(j - l + L) % L];
                    }
                }
            }
        }
        // the pass's pairs, in order
#pragma unroll
        for (int q = 0; q < L / 2; q++) {
            const int pair = k0 / 2 + q;
            if (pair < n_pairs && !done) {
                const double g0 = acc[2 * q] / (double)C / (double)n, g1 = acc[2 * q + 1] / (double)C / (double)n;
                const double rho0 = pair == 0 ? 1.0 : 1.0 - (W - g0) / plus, rho1 = 1.0 - (W - g1) / plus;
                const double P = rho0 + rho1;
                if (pair == 0) {
                    tau_sum = P; // (not clipped)
                    done = P != P;
                } else {
                    const double clipped = P > 0.0 ? P : (P != P ? P : 0.0);
                    run = (clipped < run || clipped != clipped) ? clipped : run;
                    tau_sum += run;
                    done = !(run > 0.0);
                }
            }
        }
    }
    if (live) p.n_eff[cell] = (double)n_draws / (-1.0 + 2.0 * tau_sum);
}

} // namespace

template <int KC>
__global__ __launch_bounds__(BL_SD_THREADS) void bl_site_diagnostics_psi_kernel(const BlSiteDiagnosticsParams p)
{
    sd_cell<false, KC>(p);
}
template <int KC>
__global__ __launch_bounds__(BL_SD_THREADS) void bl_site_diagnostics_prob_kernel(const BlSiteDiagnosticsParams p)
{
    sd_cell<true, KC>(p);
}

template <bool VISIT>
static dim3 sd_grid(const BlSiteDiagnosticsParams *p)
{
    const size_t cells = VISIT ? (size_t)p->J * p->T * p->N : (size_t)p->N;
    return dim3((unsigned)((cells + BL_SD_THREADS - 1) / BL_SD_THREADS));
}
size_t bl_site_diagnostics_workspace(const BlSiteDiagnosticsParams *p, bool visit)
{
    return (size_t)(visit ? sd_grid<true>(p) : sd_grid<false>(p)).x * BL_SD_THREADS * 3 * (size_t)p->n_chains;
}

template <bool VISIT, int KC>
static void sd_go(const BlSiteDiagnosticsParams *p, hipStream_t st)
{
    if constexpr (VISIT) {
        const auto kernel = bl_site_diagnostics_prob_kernel<KC>;
        hipLaunchKernelGGL(kernel, sd_grid<VISIT>(p), dim3(BL_SD_THREADS), 0, st, *p);
    } else {
        const auto kernel = bl_site_diagnostics_psi_kernel<KC>;
        hipLaunchKernelGGL(kernel, sd_grid<VISIT>(p), dim3(BL_SD_THREADS), 0, st, *p);
    }
}
// the instantiation that knows the side's covariate count (0 .. 4; the general one above that)
template <bool VISIT>
static int sd_launch(const BlSiteDiagnosticsParams *p, hipStream_t st)
{
    switch (VISIT ? p->Ko : p->Ks) {
    case 0: sd_go<VISIT, 0>(p, st); break;
    case 1: sd_go<VISIT, 1>(p, st); break;
    case 2: sd_go<VISIT, 2>(p, st); break;
    case 3: sd_go<VISIT, 3>(p, st); break;
    case 4: sd_go<VISIT, 4>(p, st); break;
    default: sd_go<VISIT, -1>(p, st); break;
    }
    return (int)hipGetLastError();
}
extern "C" int bl_launch_site_diagnostics_psi(const BlSiteDiagnosticsParams *p, hipStream_t st) { return sd_launch<false>(p, st); }
extern "C" int bl_launch_site_diagnostics_prob(const BlSiteDiagnosticsParams *p, hipStream_t st) { return sd_launch<true>(p, st); }
