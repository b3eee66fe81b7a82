// response_curves.hip -- the kernels of bl_response_curves: per posterior draw and grid value, the weighted total over the sites of the
// first deterministic site (psi; occu_rn, nmixture: abundance) or of the second summed over the visits (prob_detection; occu_cop:
// rate_detection), with ONE covariate set to the grid value at every site / visit and everything else left as it is -- the average
// response curve, partial dependence (BUILDER-DEFINED, the reference's users copy the data per grid value and reduce predict()'s arrays
// on the host; the definition is the comment of bl_response_curves in include/biolith_hip.h, the order's NumPy restatement
// tests/curves_ref.py).
//
// One thread per site, 256-thread blocks, the draws on grid.y with the strided loop of the predict kernels.  Nothing of size (draws,
// values, sites) exists: a site's value under draw n and grid value g is predict_math.hpp's fmaf chain with the grid value in covariate
// k's place -- the same fmaf calls in the same order as pm_linear, so its bits are those bl_psi_kernel / bl_pdet_kernel give on the
// modified covariates --, then the effects and the transcendental by the very calls those kernels make.  The chain's terms before k do
// not hold the grid value: they are formed once per draw (site side) or once per visit and block of values (obs side).  The covariate
// arrays are never indexed with the runtime k: the unrolled loops select by comparing their own index with it, all in registers.
//   site side  a site's covariates are staged once and kept over all draws and values
//   obs side   a visit's covariates are loaded once per block of BL_RC_VALUE_BLOCK values, whose float64 sums over the visits, in
//              ascending visit order from the first term on, are a register-only block of accumulators; the visit order does not
//              depend on the block
// Every term is multiplied by the weight in float64 and reduced at once, in bl_regional_totals' order for a single region:
//   1  a wave serves one run of 64 sites: a value's 64 terms are summed by the tree over lanes 32, 16, .. 1 apart; an idle lane holds
//      -0.0, the identity of the float64 sum; one lane writes the run's partial.  The obs kernel takes the tree a value at a time
//      (rc_wave_sum).  The site kernel, whose terms are cheap next to it, holds the terms of a block of BL_RC_VALUE_BLOCK values in a
//      lane and takes the tree as a TRANSPOSED reduce-scatter over them (rc_block_sum): at the step 32 apart the lower lane of a pair
//      keeps the first half of the block's values and the upper lane the second half, each sends the half it gives up, and so on with
//      the halves of the halves -- half as many shuffles and additions a step --, until a lane holds one value, which the remaining
//      steps finish.  Every addition is one the plain tree makes for that value, with the same two operands (a float64 sum does not
//      depend on which of the two comes first), so the bits are the plain tree's.  (Measured both ways on both sides: profiles/NOTES.md.)
//   2  the finish kernel, one thread per (draw, value), adds the runs' partials in run order; the workspace is run-major, so its reads
//      are coalesced, and they are issued 32 runs ahead of the additions, which wait for nothing but one another.
// No atomics, no LDS: a value's column is a function of the sites, the weights, the draws and that value alone -- not of the other
// values, their number, the chunking of the draws or the launch --, and two calls return the same bytes.
#include "response_curves.hpp"

#include "predict_math.hpp"

namespace {

constexpr int B = BL_RC_VALUE_BLOCK;
static_assert(B >= 1 && B <= 64 && (B & (B - 1)) == 0, "the block of values halves with the lanes' distance");

// the tree over lanes 32, 16, .. 1 apart for one value: lane 0's return is the wave's sum
__device__ __forceinline__ double rc_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
// The same tree for the B values of a lane's block at once, as a transposed reduce-scatter.  Returns, in every lane, the sum of value
// rc_lane_value(lane) of the block over the wave's 64 lanes; v is used up.
__device__ __forceinline__ double rc_block_sum(double (&v)[B], int lane)
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
// which value of its block a lane's rc_block_sum is, and whether the lane is the one that writes it
__device__ __forceinline__ int rc_lane_value(int lane)
{
    int g = 0, o = 32;
#pragma unroll
    for (int half = B / 2; half >= 1; half >>= 1, o >>= 1)
        if (lane & o) g += half;
    return g;
}
__device__ __forceinline__ bool rc_lane_writes(int lane) { return (lane & (64 / B - 1)) == 0; }

// pm_linear's chain over x with covariate k left to the caller: the terms before k, from the intercept on ...
__device__ __forceinline__ float rc_chain_before(const float (&x)[BL_MAX_COVS], const float *__restrict__ b, int k)
{
    float s = b[0];
#pragma unroll
    for (int j = 0; j < BL_MAX_COVS; j++)
        if (j < k) s = fmaf(x[j], b[j + 1], s);
    return s;
}
// ... and, behind them, the grid value in k's place and the terms after it
__device__ __forceinline__ float rc_chain_from(float s, float value, const float (&x)[BL_MAX_COVS], const float *__restrict__ b, int k, int K)
{
    s = fmaf(value, b[k + 1], s);
#pragma unroll
    for (int j = 1; j < BL_MAX_COVS; j++)
        if (j > k && j < K) s = fmaf(x[j], b[j + 1], s);
    return s;
}

} // namespace

__global__ __launch_bounds__(BL_RC_THREADS) void bl_response_curves_site_kernel(const BlResponseCurvesParams p)
{
    const int slot = blockIdx.x * BL_RC_THREADS + threadIdx.x;
    if (slot >= p.n_runs * 64) return; // (whole waves leave)
    const int run = slot >> 6, lane = threadIdx.x & 63;
    const bool live = slot < p.N;
    const int i = live ? slot : 0; // an idle lane computes site 0's value and contributes -0.0: every lane takes every shuffle
    const int ns = p.ns, Ks = p.Ks, k = p.k, V = p.n_values, model = p.model;
    const BlDrawCoords c = p.c;
    const double w = live && p.weight ? p.weight[i] : 1.0;
    float x[BL_MAX_COVS];
#pragma unroll
    for (int j = 0; j < BL_MAX_COVS; j++) x[j] = j < Ks ? p.rows[(size_t)j * ns + i] : 0.0f;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *th = p.draws + (size_t)n * p.D;
        double *part = p.part + ((size_t)run * (p.n1 - p.n0) + (n - p.n0)) * V;
        const float before = rc_chain_before(x, th, k);
        for (int g0 = 0; g0 < V; g0 += B) {
            double term[B];
#pragma unroll
            for (int b = 0; b < B; b++) {
                // pm_site_eta's statements, then bl_psi_kernel's: occu psi = sigmoid(eta); occu_rn, nmixture: abundance = exp(eta)
                float eta = rc_chain_from(before, p.values[min(g0 + b, V - 1)], x, th, k, Ks); // (past the last value: never written)
                if (c.o_u >= 0) eta += th[c.o_u + i];
                const float v = (model == 1 || model == 4) ? __expf(eta) : pm_sigmoid(eta);
                term[b] = live ? w * (double)v : -0.0;
            }
            const double sum = rc_block_sum(term, lane);
            const int g = g0 + rc_lane_value(lane);
            if (rc_lane_writes(lane) && g < V) part[g] = sum;
        }
    }
}

__global__ __launch_bounds__(BL_RC_THREADS) void bl_response_curves_obs_kernel(const BlResponseCurvesParams p)
{
    const int slot = blockIdx.x * BL_RC_THREADS + threadIdx.x;
    if (slot >= p.n_runs * 64) return;
    const int run = slot >> 6, lane = threadIdx.x & 63;
    const bool live = slot < p.N;
    const int i = live ? slot : 0;
    const int ns = p.ns, T = p.T, J = p.J, Ko = p.Ko, k = p.k, V = p.n_values, model = p.model;
    const BlDrawCoords c = p.c;
    const double w = live && p.weight ? p.weight[i] : 1.0;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *th = p.draws + (size_t)n * p.D, *al = th + p.Ks + 1;
        double *part = p.part + ((size_t)run * (p.n1 - p.n0) + (n - p.n0)) * V;
        for (int g0 = 0; g0 < V; g0 += B) {
            float value[B];
            double s[B];
#pragma unroll
            for (int b = 0; b < B; b++) value[b] = p.values[min(g0 + b, V - 1)]; // (past the last value: computed, never written)
            for (int v = 0; v < T * J; v++) {
                float x[BL_MAX_COVS];
#pragma unroll
                for (int j = 0; j < BL_MAX_COVS; j++) x[j] = j < Ko ? p.wraw[((size_t)v * Ko + j) * ns + i] : 0.0f;
                const float before = rc_chain_before(x, al, k);
#pragma unroll
                for (int b = 0; b < B; b++) {
                    // pm_visit_nu's statements, then bl_pdet_kernel's: prob_detection = sigmoid(nu); occu_cop: rate_detection = exp(nu)
                    const float nu = pm_visit_effects(rc_chain_from(before, value[b], x, al, k, Ko), th, c, T, J, v, i);
                    const float u = model == 3 ? __expf(nu) : pm_sigmoid(nu);
                    s[b] = v == 0 ? (double)u : s[b] + (double)u; // the sum starts from the first term
                }
            }
#pragma unroll
            for (int b = 0; b < B; b++) {
                if (g0 + b >= V) break; // (wave-uniform)
                const double sum = rc_wave_sum(live ? w * s[b] : -0.0);
                if (lane == 0) part[g0 + b] = sum;
            }
        }
    }
}

// total[dn][g] = the runs' partials of (draw dn, value g), added in run order
// (one wave a block: a chunk of 10^6 sites' 32 values has some 2000 threads, which so spread over 34 compute units, not 9)
__global__ __launch_bounds__(BL_RC_FINISH_THREADS) void bl_response_curves_finish_kernel(const BlResponseCurvesParams p)
{
    const size_t cells = (size_t)(p.n1 - p.n0) * p.n_values;
    const size_t q = (size_t)blockIdx.x * BL_RC_FINISH_THREADS + threadIdx.x;
    if (q >= cells) return;
    constexpr int AHEAD = 32;
    double sum = p.part[q];
    int r = 1;
    for (; r + AHEAD <= p.n_runs; r += AHEAD) {
        double v[AHEAD];
#pragma unroll
        for (int j = 0; j < AHEAD; j++) v[j] = p.part[(size_t)(r + j) * cells + q];
#pragma unroll
        for (int j = 0; j < AHEAD; j++) sum += v[j];
    }
    for (; r < p.n_runs; r++) sum += p.part[(size_t)r * cells + q];
    p.total[q] = sum;
}

extern "C" int bl_launch_response_curves(const BlResponseCurvesParams *p, int grid_y, hipStream_t st)
{
    const dim3 grid((p->n_runs * 64 + BL_RC_THREADS - 1) / BL_RC_THREADS, grid_y);
    if (p->side) hipLaunchKernelGGL(bl_response_curves_obs_kernel, grid, dim3(BL_RC_THREADS), 0, st, *p);
    else hipLaunchKernelGGL(bl_response_curves_site_kernel, grid, dim3(BL_RC_THREADS), 0, st, *p);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    const size_t cells = (size_t)(p->n1 - p->n0) * p->n_values;
    hipLaunchKernelGGL(bl_response_curves_finish_kernel, dim3((unsigned)((cells + BL_RC_FINISH_THREADS - 1) / BL_RC_FINISH_THREADS)),
                       dim3(BL_RC_FINISH_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
