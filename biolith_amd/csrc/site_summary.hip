// site_summary.hip -- the kernels of bl_site_summary: per cell of a deterministic site, over all the posterior draws, the mean, the
// standard deviation and order statistics of the site's float32 values (BUILDER-DEFINED, the reference's users reduce predict()'s arrays
// on the host; the definition is the comment of bl_site_summary in include/biolith_hip.h, its NumPy restatement tests/summary_ref.py).
//
// One thread per cell, 256-thread blocks, the site fastest in a wave: a cell is a site (the first site, constant over the periods) or
// (j, t, site) in bl_deterministic's order (the second).  The cell's covariates are read once and stay in registers; a draw's
// coefficients are wave-uniform reads -- one read per draw where the instantiation knows the side's covariate count (0 .. 4; the general
// one serves the rest).  Nothing of size (draws, cells) exists: the value under draw n is a handful of FMAs and one
// __expf -- the very calls into predict_math.hpp that bl_psi_kernel and bl_pdet_kernel make, so its bits are bl_deterministic's -- and it
// is formed anew in every pass:
//   1  the sum in float64 in draw order -> the mean; the smallest and the largest value
//   2  sum (v - mean)^2 in float64 in draw order -> sd = sqrt(M2 / (n - 1)), NaN for one draw           (only where sd is wanted)
//   3  the order statistics, by bisection on the bit pattern (site_summary.hpp: the values are >= +0, so it orders them): the value
//      of rank r is the largest K with #{v < K} <= r.  A pass over the draws settles one bit of every rank's K, a counter per rank,
//      all counters in registers.  The bits above the highest bit in which the wave's smallest and largest values differ are common
//      to all of them and take no pass: a probability's values cost about 25 passes, a cell whose draws are all equal none.
// Every pass count is the wave's, so control flow is wave-uniform; a cell's results do not depend on it: bits a cell's values share
// come out of the bisection as they went in.  No atomics, no LDS, no workspace: a cell's outputs are a function of its covariates, its
// effects and the draws, not of N, the block it falls in or the outputs asked for, and two calls return the same bits.
#include "site_summary.hpp"

#include "predict_math.hpp"

namespace {

// the float32 value of the cell under draw n: bl_psi_kernel's / bl_pdet_kernel's statements on the staged covariates.  KC: the covariate
// count of the cell's side where the instantiation knows it (the dot product unrolls and a draw's coefficients come in one read),
// -1 = the handle's
template <bool VISIT, int KC>
__device__ __forceinline__ float ss_value(const BlSiteSummaryParams &p, const float *__restrict__ x, int i, int v, int n)
{
    const float *th = p.draws + (size_t)n * p.D;
    if (VISIT) {
        const float nu = pm_visit_nu_staged(x, th, th + p.Ks + 1, KC >= 0 ? KC : p.Ko, p.c, p.T, p.J, v, i);
        return p.model == 3 ? __expf(nu) : pm_sigmoid(nu); // occu_cop: rate_detection
    }
    const float eta = pm_site_eta(x, 1, th, KC >= 0 ? KC : p.Ks, p.c, i);
    return (p.model == 1 || p.model == 4) ? __expf(eta) : pm_sigmoid(eta); // occu_rn, nmixture: abundance
}

// NR: the counters the instantiation carries, >= p.n_ranks (0: no order statistic)
template <bool VISIT, int NR, int KC>
__device__ __forceinline__ void ss_cell(const BlSiteSummaryParams &p)
{
    const size_t cells = VISIT ? (size_t)p.J * p.T * p.N : (size_t)p.N;
    size_t cell = (size_t)blockIdx.x * BL_SS_THREADS + threadIdx.x; // = (j T + t) N + i
    const bool live = cell < cells;
    if (!live) cell = cells - 1; // the tail block's idle threads redo the last cell and write nothing: every lane takes every pass
    const int i = (int)(cell % p.N), jt = (int)(cell / p.N), v = VISIT ? (jt % p.T) * p.J + jt / p.T : 0;
    const int n_draws = p.n_draws;

    float x[BL_MAX_COVS];
    const int nk = KC >= 0 ? KC : VISIT ? p.Ko : p.Ks;
    if (VISIT) {
        for (int k = 0; k < nk; k++) x[k] = p.wraw[((size_t)v * nk + k) * p.ns + i];
    } else {
        for (int k = 0; k < nk; k++) x[k] = p.rows[(size_t)k * p.ns + i];
    }

    // ---- 1
    double sum = 0.0;
    unsigned lo = 0xffffffffu, hi = 0u;
    for (int n = 0; n < n_draws; n++) {
        const float val = ss_value<VISIT, KC>(p, x, i, v, n);
        const unsigned key = __float_as_uint(val);
        sum += (double)val;
        lo = key < lo ? key : lo;
        hi = key > hi ? key : hi;
    }
    const double mean = sum / (double)n_draws;
    if (live && p.mean) p.mean[cell] = mean;

    // ---- 2
    if (p.sd) {
        double m2 = 0.0;
        for (int n = 0; n < n_draws; n++) {
            const double d = (double)ss_value<VISIT, KC>(p, x, i, v, n) - mean;
            m2 += d * d;
        }
        if (live) p.sd[cell] = sqrt(m2 / (double)(n_draws - 1)); // (0 / 0 for one draw)
    }

    // ---- 3
    if constexpr (NR > 0) {
        if (!p.order) return; // (wave-uniform)
        unsigned diff = lo ^ hi;
        for (int o = 32; o > 0; o >>= 1) diff |= (unsigned)__shfl_xor((int)diff, o);
        diff = __builtin_amdgcn_readfirstlane(diff);                  // (every lane holds it; now the compiler knows)
        const unsigned below = diff ? 0xffffffffu >> __clz(diff) : 0u; // the bits that take a pass
        unsigned K[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) K[r] = lo & ~below;
        for (unsigned bit = below ^ (below >> 1); bit; bit >>= 1) {
            int cnt[NR];
#pragma unroll
            for (int r = 0; r < NR; r++) cnt[r] = 0;
            for (int n = 0; n < n_draws; n++) {
                const unsigned key = __float_as_uint(ss_value<VISIT, KC>(p, x, i, v, n));
#pragma unroll
                for (int r = 0; r < NR; r++) cnt[r] += key < (K[r] | bit) ? 1 : 0;
            }
#pragma unroll
            for (int r = 0; r < NR; r++)
                if (cnt[r] <= p.ranks[r]) K[r] |= bit;
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < NR; r++)
                if (r < p.n_ranks) p.order[(size_t)r * cells + cell] = __uint_as_float(K[r]);
        }
    }
}

} // namespace

template <int NR, int KC>
__global__ __launch_bounds__(BL_SS_THREADS) void bl_site_summary_psi_kernel(const BlSiteSummaryParams p)
{
    ss_cell<false, NR, KC>(p);
}
template <int NR, int KC>
__global__ __launch_bounds__(BL_SS_THREADS) void bl_site_summary_prob_kernel(const BlSiteSummaryParams p)
{
    ss_cell<true, NR, KC>(p);
}

template <bool VISIT, int NR, int KC>
static void ss_go(const BlSiteSummaryParams *p, dim3 grid, hipStream_t st)
{
    if constexpr (VISIT) {
        const auto kernel = bl_site_summary_prob_kernel<NR, KC>;
        hipLaunchKernelGGL(kernel, grid, dim3(BL_SS_THREADS), 0, st, *p);
    } else {
        const auto kernel = bl_site_summary_psi_kernel<NR, KC>;
        hipLaunchKernelGGL(kernel, grid, dim3(BL_SS_THREADS), 0, st, *p);
    }
}
// the instantiation that knows the side's covariate count (0 .. 4; the general one above that)
template <bool VISIT, int NR>
static void ss_go(const BlSiteSummaryParams *p, dim3 grid, hipStream_t st)
{
    switch (VISIT ? p->Ko : p->Ks) {
    case 0: return ss_go<VISIT, NR, 0>(p, grid, st);
    case 1: return ss_go<VISIT, NR, 1>(p, grid, st);
    case 2: return ss_go<VISIT, NR, 2>(p, grid, st);
    case 3: return ss_go<VISIT, NR, 3>(p, grid, st);
    case 4: return ss_go<VISIT, NR, 4>(p, grid, st);
    default: return ss_go<VISIT, NR, -1>(p, grid, st);
    }
}
// ... with the fewest counters that hold the call's ranks
template <bool VISIT>
static int ss_launch(const BlSiteSummaryParams *p, hipStream_t st)
{
    const size_t cells = VISIT ? (size_t)p->J * p->T * p->N : (size_t)p->N;
    const dim3 grid((unsigned)((cells + BL_SS_THREADS - 1) / BL_SS_THREADS));
    const int nr = p->order ? p->n_ranks : 0;
    if (nr == 0) ss_go<VISIT, 0>(p, grid, st);
    else if (nr <= 4) ss_go<VISIT, 4>(p, grid, st);
    else if (nr <= 8) ss_go<VISIT, 8>(p, grid, st);
    else ss_go<VISIT, BL_SUMMARY_MAX_RANKS>(p, grid, st);
    return (int)hipGetLastError();
}
extern "C" int bl_launch_site_summary_psi(const BlSiteSummaryParams *p, hipStream_t st) { return ss_launch<false>(p, st); }
extern "C" int bl_launch_site_summary_prob(const BlSiteSummaryParams *p, hipStream_t st) { return ss_launch<true>(p, st); }
