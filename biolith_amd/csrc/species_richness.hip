// species_richness.hip -- the kernels of bl_species_richness: the posterior of the number of species a site holds, over the S species
// that were sampled under one chain (BUILDER-DEFINED, the reference has no counterpart; the definition is the comment of
// bl_species_richness in include/biolith_hip.h, its NumPy restatement tests/richness_ref.py).
//
// Given draw n, the species' presences at site i are independent Bernoulli(psi_s), psi_s the float32 bl_deterministic gives for species
// s's coefficient block -- the very calls into predict_math.hpp that bl_psi_kernel makes, so its bits are bl_deterministic's --, and the
// number present is Poisson-binomial.  Its pmf is the float64 recursion over the species in ascending order, from pi = [1, 0, .. 0]:
//   p = (double)psi_s, q = 1.0 - p;   pi[r] <- pi[r] q + pi[r - 1] p  (r = s + 1 .. 1),   pi[0] <- pi[0] q
// two products and one sum, each rounded (a statement each: -ffp-contract=on fuses nothing across statements).  Entries above s + 1 are
// +0 before and after species s, so the step stops there.  E = sum_s p, float64 in ascending s.
//
// The recursion lives in registers: pi is indexed by the unrolled loops' own counters only, never by a run-time value, so it is
// instantiated per CAPACITY CLASS of S (8, 16, 32 species: 9, 17, 33 doubles); a class skips the species beyond S by a wave-uniform
// branch per species -- skipping is the p = 0 step, which leaves every entry's bits as they are.  Nothing of size (draws, sites) exists.
//
// Area side (bl_species_richness_area_kernel): one thread per slot of the host's padded layout, 256-thread blocks, the draws on grid.y
// with the strided loop of the predict kernels; covariates and weight are staged once, a draw's S coefficient blocks are wave-uniform
// reads.  Row r's term is w pi[r], a float64 product, reduced in regional_totals.hip's order: a wave serves one region, a row's 64 terms
// are summed by the tree over lanes 32, 16, .. 1 apart, an idle lane holds -0.0, the identity of the float64 sum.  The S + 1 rows are
// taken BL_SR_ROW_BLOCK = 4 at a time as trajectory_totals.hip's transposed reduce-scatter (sr_block_sum): 7 shuffles and additions a
// block where four plain trees take 24; every addition is one the plain tree makes for that row, with the same two operands, so the
// bits are the plain tree's (blocks of 1, 4 and 8 measured, the same bytes: profiles/NOTES.md).  The workspace is wave-major; the
// finish kernel, one thread per (region, draw, row), adds a region's partials in wave order, its loads issued 32 waves ahead.
//
// Site side (bl_species_richness_site_kernel): one thread per site over ALL the draws in ascending order, an accumulator per entry of
// the pmf and one for E, in registers; the sd of E takes a second pass that forms E anew (site_summary.hip's two passes).  Where the pmf
// is not wanted the kernel without the recursion runs; E's statements are the same in both.
//
// No atomics, no LDS: a region's rows are a function of its own sites in site order, their weights and the draws, a site's outputs of
// its covariates, its effects and the draws -- not of the other regions or sites, of the chunking of the draws, of the launch or of the
// outputs asked for --, and two calls return the same bytes.
#include "species_richness.hpp"

#include "predict_math.hpp"

namespace {

constexpr int B = BL_SR_ROW_BLOCK; // the rows of a block of the reduction
static_assert(B >= 1 && B <= 64 && (B & (B - 1)) == 0, "the block of rows halves with the lanes' distance");

// The tree over lanes 32, 16, .. 1 apart for the B rows of a lane's block at once, as a transposed reduce-scatter (response_curves.hip:
// rc_block_sum): at the step 32 apart the lower lane of a pair keeps the first half of the block's rows and the upper lane the second
// half, each sends the half it gives up, and so on with the halves of the halves, until a lane holds one row, which the remaining steps
// finish.  Returns, in every lane, the sum of row sr_lane_row(lane) of the block over the wave's 64 lanes; v is used up.
__device__ __forceinline__ double sr_block_sum(double (&v)[B], int lane)
{
    int o = 32;
#pragma unroll
    for (int half = B / 2; half >= 1; half >>= 1, o >>= 1) {
        const bool upper = lane & o;
#pragma unroll
        for (int j = 0; j < half; j++) {
            const double send = upper ? v[j] : v[j + half], keep = upper ? v[j + half] : v[j];
            v[j] = keep + __shfl_xor(send, o);
        }
    }
    double s = v[0];
    for (; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}
// which row of its block a lane's sr_block_sum is (B = 4: lanes 0-15: 0, 16-31: 1, 32-47: 2, 48-63: 3), and whether the lane is the
// one that writes it (the first of the lanes that hold the row)
__device__ __forceinline__ int sr_lane_row(int lane)
{
    int g = 0, o = 32;
#pragma unroll
    for (int half = B / 2; half >= 1; half >>= 1, o >>= 1)
        if (lane & o) g += half;
    return g;
}
__device__ __forceinline__ bool sr_lane_writes(int lane) { return (lane & (64 / B - 1)) == 0; }

// a site's covariates, staged once (beyond Ks: unread)
__device__ __forceinline__ void sr_stage(const BlSpeciesRichnessParams &p, int i, float (&x)[BL_MAX_COVS])
{
#pragma unroll
    for (int k = 0; k < BL_MAX_COVS; k++) x[k] = k < p.Ks ? p.rows[(size_t)k * p.ns + i] : 0.0f;
}
// psi of species s at site i under draw n: bl_psi_kernel's statements on species s's block
__device__ __forceinline__ float sr_psi(const BlSpeciesRichnessParams &p, const float (&x)[BL_MAX_COVS], int i, int n, int s)
{
    const float *__restrict__ th = p.draws + ((size_t)n * p.S + s) * p.D;
    return pm_sigmoid(pm_site_eta(x, 1, th, p.Ks, p.c, i));
}
// E = sum_s (double)psi_s in ascending s, alone
__device__ __forceinline__ double sr_expected(const BlSpeciesRichnessParams &p, const float (&x)[BL_MAX_COVS], int i, int n)
{
    double E = 0.0;
    for (int s = 0; s < p.S; s++) E += (double)sr_psi(p, x, i, n, s);
    return E;
}
// the pmf of the number of species present at site i under draw n into pi; returns E (sr_expected's additions)
template <int CAP>
__device__ __forceinline__ double sr_pmf(const BlSpeciesRichnessParams &p, const float (&x)[BL_MAX_COVS], int i, int n, double (&pi)[CAP + 1])
{
    const int S = p.S;
    pi[0] = 1.0;
#pragma unroll
    for (int r = 1; r <= CAP; r++) pi[r] = 0.0;
    double E = 0.0;
#pragma unroll
    for (int s = 0; s < CAP; s++) {
        if (s < S) { // (wave-uniform)
            const double ps = (double)sr_psi(p, x, i, n, s), q = 1.0 - ps;
            E += ps;
#pragma unroll
            for (int r = s + 1; r >= 1; r--) {
                const double stay = pi[r] * q;
                const double come = pi[r - 1] * ps;
                pi[r] = stay + come;
            }
            pi[0] = pi[0] * q; // (+ 0 p: the product's bits)
        }
    }
    return E;
}

} // namespace

template <int CAP>
__global__ __launch_bounds__(BL_SR_THREADS) void bl_species_richness_area_kernel(const BlSpeciesRichnessParams p)
{
    const int slot = blockIdx.x * BL_SR_THREADS + threadIdx.x;
    if (slot >= p.n_slots) return; // (n_slots is a multiple of 64: whole waves leave)
    const int wave = slot >> 6, lane = threadIdx.x & 63;
    const int site = p.slot_site[slot];
    const bool live = site >= 0;
    const int i = live ? site : 0; // an idle lane computes site 0's values and contributes -0.0: every lane takes every shuffle
    const int rows = p.S + 1;
    const size_t cells = (size_t)(p.n1 - p.n0) * rows; // the output rows of the chunk
    const double w = live && p.slot_w ? p.slot_w[slot] : 1.0;
    float x[BL_MAX_COVS];
    sr_stage(p, i, x);
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        double *__restrict__ part = p.part + (size_t)wave * cells + (size_t)(n - p.n0) * rows; // [wave][draw of the chunk][row]
        double pi[CAP + 1];
        sr_pmf<CAP>(p, x, i, n, pi);
#pragma unroll
        for (int g0 = 0; g0 <= CAP; g0 += B) {
            if (g0 < rows) { // (wave-uniform)
                double v[B];
#pragma unroll
                for (int j = 0; j < B; j++) v[j] = live && g0 + j <= CAP ? w * pi[g0 + j < CAP ? g0 + j : CAP] : -0.0;
                const double sum = sr_block_sum(v, lane);
                const int row = g0 + sr_lane_row(lane);
                if (sr_lane_writes(lane) && row < rows) part[row] = sum;
            }
        }
    }
}

// area_total[dn][r][g] = the partials of region g's waves, added in wave order; a region without a site: 0.  One thread per (region,
// draw, row), the region slowest: the workspace is wave-major, so the threads of a wave read neighbouring doubles, and the loads are
// issued 32 waves ahead of the additions, which wait for nothing but one another.  One wave a block: a chunk has few thousand threads,
// which so spread over the compute units.
__global__ __launch_bounds__(BL_SR_FINISH_THREADS) void bl_species_richness_finish_kernel(const BlSpeciesRichnessParams p)
{
    const int G = p.n_regions;
    const size_t cells = (size_t)(p.n1 - p.n0) * (p.S + 1);
    const size_t c = (size_t)blockIdx.x * BL_SR_FINISH_THREADS + threadIdx.x;
    if (c >= cells * G) return;
    const int g = (int)(c / cells);
    const size_t q = c % cells; // = dn (S + 1) + r
    const int w0 = p.wave_first[g], w1 = p.wave_first[g + 1];
    constexpr int AHEAD = 32;
    const double *__restrict__ part = p.part + q;
    double sum = w0 < w1 ? part[(size_t)w0 * cells] : 0.0;
    int wv = w0 + 1;
    for (; wv + AHEAD <= w1; wv += AHEAD) {
        double v[AHEAD];
#pragma unroll
        for (int j = 0; j < AHEAD; j++) v[j] = part[(size_t)(wv + j) * cells];
#pragma unroll
        for (int j = 0; j < AHEAD; j++) sum += v[j];
    }
    for (; wv < w1; wv++) sum += part[(size_t)wv * cells];
    p.area_total[q * G + g] = sum;
}

// PMF: the pmf is wanted, CAP its capacity class; else E alone (CAP unused)
template <int CAP, bool PMF>
__global__ __launch_bounds__(BL_SR_THREADS) void bl_species_richness_site_kernel(const BlSpeciesRichnessParams p)
{
    const int i = blockIdx.x * BL_SR_THREADS + threadIdx.x;
    if (i >= p.N) return; // (no lane waits for another)
    const int n_draws = p.n_draws;
    float x[BL_MAX_COVS];
    sr_stage(p, i, x);

    // ---- 1: the sums over the draws, in draw order
    double esum = 0.0;
    if constexpr (PMF) {
        const int S = p.S;
        double acc[CAP + 1];
#pragma unroll
        for (int r = 0; r <= CAP; r++) acc[r] = 0.0;
        for (int n = 0; n < n_draws; n++) {
            double pi[CAP + 1];
            esum += sr_pmf<CAP>(p, x, i, n, pi);
#pragma unroll
            for (int r = 0; r <= CAP; r++) acc[r] += pi[r];
        }
        double *__restrict__ out = p.pmf + (size_t)i * (S + 1);
#pragma unroll
        for (int r = 0; r <= CAP; r++)
            if (r <= S) out[r] = acc[r] / (double)n_draws;
    } else {
        for (int n = 0; n < n_draws; n++) esum += sr_expected(p, x, i, n);
    }
    const double mean = esum / (double)n_draws;
    if (p.mean) p.mean[i] = mean;

    // ---- 2
    if (p.sd) {
        double m2 = 0.0;
        for (int n = 0; n < n_draws; n++) {
            const double d = sr_expected(p, x, i, n) - mean;
            m2 += d * d;
        }
        p.sd[i] = sqrt(m2 / (double)(n_draws - 1)); // (0 / 0 for one draw)
    }
}

template <int CAP>
static void sr_go_area(const BlSpeciesRichnessParams *p, dim3 grid, hipStream_t st)
{
    const auto kernel = bl_species_richness_area_kernel<CAP>;
    hipLaunchKernelGGL(kernel, grid, dim3(BL_SR_THREADS), 0, st, *p);
}
template <int CAP, bool PMF>
static void sr_go_site(const BlSpeciesRichnessParams *p, dim3 grid, hipStream_t st)
{
    const auto kernel = bl_species_richness_site_kernel<CAP, PMF>;
    hipLaunchKernelGGL(kernel, grid, dim3(BL_SR_THREADS), 0, st, *p);
}

extern "C" int bl_launch_species_richness_area(const BlSpeciesRichnessParams *p, int grid_y, hipStream_t st)
{
    if (p->n_slots > 0) { // (every site in no region: the totals are the finish kernel's zeros)
        const dim3 grid((p->n_slots + BL_SR_THREADS - 1) / BL_SR_THREADS, grid_y);
        if (p->S <= 8 && BL_SR_MIN_CLASS <= 8) sr_go_area<8>(p, grid, st);
        else if (p->S <= 16 && BL_SR_MIN_CLASS <= 16) sr_go_area<16>(p, grid, st);
        else sr_go_area<BL_RICHNESS_MAX_SPECIES>(p, grid, st);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    const size_t cells = (size_t)(p->n1 - p->n0) * (p->S + 1) * p->n_regions;
    hipLaunchKernelGGL(bl_species_richness_finish_kernel, dim3((unsigned)((cells + BL_SR_FINISH_THREADS - 1) / BL_SR_FINISH_THREADS)),
                       dim3(BL_SR_FINISH_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}

extern "C" int bl_launch_species_richness_site(const BlSpeciesRichnessParams *p, hipStream_t st)
{
    const dim3 grid((p->N + BL_SR_THREADS - 1) / BL_SR_THREADS);
    if (!p->pmf) sr_go_site<0, false>(p, grid, st);
    else if (p->S <= 8 && BL_SR_MIN_CLASS <= 8) sr_go_site<8, true>(p, grid, st);
    else if (p->S <= 16 && BL_SR_MIN_CLASS <= 16) sr_go_site<16, true>(p, grid, st);
    else sr_go_site<BL_RICHNESS_MAX_SPECIES, true>(p, grid, st);
    return (int)hipGetLastError();
}
