// trajectory_totals.hip -- the kernels of bl_trajectory_totals: per posterior draw of an occu_dyn handle and region, the weighted totals
// over the region's sites of the occupancy trajectory without the observations -- the expected occupancy per season, the area colonised
// and lost between seasons, the equilibrium -- and of one ancestral path per draw (BUILDER-DEFINED, like the model; the definition is
// the comment of bl_trajectory_totals in include/biolith_hip.h, its NumPy restatement tests/trajectory_ref.py).
//
// One thread per slot of the host's padded layout (trajectory_totals.hpp), 256-thread blocks, the draws on grid.y with the strided loop
// of the predict kernels.  A thread gathers its site's covariates and weight through the slot's index once and keeps them in registers,
// promoted to float64; a draw's coefficients are wave-uniform reads.  Nothing of size (draws, sites) exists.
//
// Arithmetic, float64 throughout (the predict family is float32: there is no device predict for occu_dyn whose bits could be promised,
// and the outputs are sums of up to 10^6 terms and ratios near 1):
//   eta      = fma(x_K, b_K, .. fma(x_1, b_1, b_0)), in covariate order, the intercept first, for psi, gamma and eps
//   sigma    e = exp(-|eta|), r = 1 / (1 + e), s = e r:  (sigma(eta), sigma(-eta)) = eta > 0 ? (r, s) : (s, r)  -- both sides of a rate come
//            from the sigmoid, no complement is formed as 1 - x (the rule of path_posterior.hip)
//   t = 0    pi = psi, q = sigma(-eta_psi)
//   step     col = q gamma, ext = pi eps;   pi' = fma(pi, 1 - eps, col),   q' = fma(q, 1 - gamma, ext)      -- two POSITIVE sums
//   eq       gamma / (gamma + eps)
//   path     cell (n, t, i) takes one uniform u of bl_cell_rng(seed, n, T, t, N, i), i the ORIGINAL site index:
//            z_0 = (double)u < psi,   z_t+1 = (double)u < (z_t ? 1 - eps : gamma)
// T is a run-time value: a step's terms are formed, multiplied by the weight and reduced across the wave at once, nothing is kept per
// period, so no array with a run-time index exists and nothing goes to scratch.  The covariates' loops run over the capacity
// BL_TT_MAX_KS with the count as a guard, so they unroll and the staged covariates stay in registers.
//
// The sum is regional_totals.hip's: a wave serves one region, a row's 64 terms are summed by the tree over lanes 32, 16, .. 1 apart; an
// idle lane holds -0.0, the identity of the float64 sum, so a region of one site returns its term's bits; one lane writes the wave's
// partial and the finish kernel, one thread per (region, draw, output row), adds the region's partials in wave order.  A period has up
// to six rows and their reductions are nearly all of the kernel's time, so the tree is taken for a BLOCK of four rows at once, as
// response_curves.hip's transposed reduce-scatter (tt_block_sum): a period's expected rows (occupancy, colonised, extinct and, at the
// first period, the equilibrium) are one block, its realised rows (z, z_colonised, z_extinct) another -- 7 shuffles and additions a
// block where four plain trees take 24.  Every addition is one the plain tree makes for that row, with the same two operands, so the
// bits are the plain tree's (measured both ways: profiles/NOTES.md).  A block whose rows are all unwanted is skipped; an unwanted row of
// a block that runs is reduced and not written.  No atomics, no LDS: a region's row is a function of its own sites in site order, their
// weights and the draws -- not of the other regions, of the chunking of the draws or of the outputs asked for --, and two calls return
// the same bytes.
#include "trajectory_totals.hpp"

#include "pred_rng.hpp"

namespace {

constexpr int B = 4; // the rows of a block

// The tree over lanes 32, 16, .. 1 apart for the B rows of a lane's block at once, as a transposed reduce-scatter: at the step 32 apart
// the lower lane of a pair keeps the first half of the block's rows and the upper lane the second half, each sends the half it gives
// up, and so on with the halves of the halves, until a lane holds one row, which the remaining steps finish.  Returns, in every lane,
// the sum of row tt_lane_row(lane) of the block over the wave's 64 lanes; v is used up.
__device__ __forceinline__ double tt_block_sum(double (&v)[B], int lane)
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
// which row of its block a lane's tt_block_sum is (lanes 0-15: 0, 16-31: 1, 32-47: 2, 48-63: 3); the first lane of the 16 writes it
__device__ __forceinline__ int tt_lane_row(int lane) { return ((lane & 32) ? 2 : 0) + ((lane & 16) ? 1 : 0); }
__device__ __forceinline__ bool tt_lane_writes(int lane) { return (lane & 15) == 0; }

// reduces the block and writes its rows: row0 .. row3 are their places among the draw's output rows, -1 = not written
__device__ __forceinline__ void tt_reduce_block(double (&v)[B], int lane, int row0, int row1, int row2, int row3, double *__restrict__ part)
{
    const double sum = tt_block_sum(v, lane);
    const int j = tt_lane_row(lane), row = j == 0 ? row0 : j == 1 ? row1 : j == 2 ? row2 : row3;
    if (tt_lane_writes(lane) && row >= 0) part[row] = sum;
}

// f = sigma(x), g = sigma(-x), each from its own positive parts
__device__ __forceinline__ void tt_sig(double x, double &f, double &g)
{
    const double e = exp(-fabs(x)), r = 1.0 / (1.0 + e), s = e * r;
    f = x > 0.0 ? r : s;
    g = x > 0.0 ? s : r;
}

} // namespace

__global__ __launch_bounds__(BL_TT_THREADS) void bl_trajectory_totals_kernel(const BlTrajectoryTotalsParams p)
{
    const int slot = blockIdx.x * BL_TT_THREADS + threadIdx.x;
    if (slot >= p.n_slots) return; // (n_slots is a multiple of 64: whole waves leave)
    const int wave = slot >> 6, lane = threadIdx.x & 63;
    const int site = p.slot_site[slot];
    const bool live = site >= 0;
    const int i = live ? site : 0; // an idle lane computes site 0's values and contributes -0.0: every lane takes every shuffle
    const int ns = p.ns, N = p.N, T = p.T, Ks = p.Ks, rows = p.row_first[BL_TT_OUTPUTS];
    const size_t cells = (size_t)(p.n1 - p.n0) * rows; // the output rows of the chunk
    const int r_occ = p.row_first[BL_TT_OCC], r_col = p.row_first[BL_TT_COL], r_ext = p.row_first[BL_TT_EXT];
    const int r_eq = p.row_first[BL_TT_EQ], r_z = p.row_first[BL_TT_Z], r_zcol = p.row_first[BL_TT_ZCOL], r_zext = p.row_first[BL_TT_ZEXT];
    // (T = 1: the per-pair outputs have no rows)
    const bool w_occ = r_col > r_occ, w_col = r_ext > r_col, w_ext = r_eq > r_ext, w_eq = r_z > r_eq;
    const bool w_z = r_zcol > r_z, w_zcol = r_zext > r_zcol, w_zext = rows > r_zext;
    const bool steps = w_occ || w_col || w_ext, path = w_z || w_zcol || w_zext;
    const double w = live && p.slot_w ? p.slot_w[slot] : 1.0;
    double x[BL_TT_MAX_KS];
#pragma unroll
    for (int k = 0; k < BL_TT_MAX_KS; k++) x[k] = k < Ks ? (double)p.rows[(size_t)k * ns + i] : 0.0;
    for (int n = p.n0 + blockIdx.y; n < p.n1; n += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)n * p.D;
        double *__restrict__ part = p.part + (size_t)wave * cells + (size_t)(n - p.n0) * rows; // [wave][draw of the chunk][row]
        double e_psi = (double)th[0], e_gam = (double)th[Ks + 1], e_eps = (double)th[2 * (Ks + 1)];
#pragma unroll
        for (int k = 0; k < BL_TT_MAX_KS; k++)
            if (k < Ks) {
                e_psi = fma(x[k], (double)th[k + 1], e_psi);
                e_gam = fma(x[k], (double)th[Ks + 1 + k + 1], e_gam);
                e_eps = fma(x[k], (double)th[2 * (Ks + 1) + k + 1], e_eps);
            }
        double psi, npsi, gam, ngam, eps, neps;
        tt_sig(e_psi, psi, npsi);
        tt_sig(e_gam, gam, ngam);
        tt_sig(e_eps, eps, neps);
        const double eq = gam / (gam + eps);
        double pi = psi, q = npsi;
        bool zb = false;
        for (int t = 0; t < T; t++) {
            const bool pair = t + 1 < T;
            const double col = q * gam, ext = pi * eps;
            if (steps || (w_eq && t == 0)) { // the expected rows of the period: occupancy, colonised, extinct; the equilibrium rides with the first
                double v[B] = {live ? w * pi : -0.0, live ? w * col : -0.0, live ? w * ext : -0.0, live ? w * eq : -0.0};
                tt_reduce_block(v, lane, w_occ ? r_occ + t : -1, w_col && pair ? r_col + t : -1, w_ext && pair ? r_ext + t : -1,
                                w_eq && t == 0 ? r_eq : -1, part);
            }
            if (path) { // the realised rows: z, and the transition into this period
                BlPredRng rng = bl_cell_rng(p.seed, n, T, t, N, i);
                const bool zn = (double)rng.uniform() < (t == 0 ? psi : zb ? neps : gam);
                double v[B] = {live ? w * (zn ? 1.0 : 0.0) : -0.0, live ? w * (!zb && zn ? 1.0 : 0.0) : -0.0,
                               live ? w * (zb && !zn ? 1.0 : 0.0) : -0.0, -0.0};
                tt_reduce_block(v, lane, w_z ? r_z + t : -1, w_zcol && t > 0 ? r_zcol + t - 1 : -1, w_zext && t > 0 ? r_zext + t - 1 : -1, -1,
                                part);
                zb = zn;
            }
            const double pi1 = fma(pi, neps, col), q1 = fma(q, ngam, ext);
            pi = pi1; q = q1;
        }
    }
}

// out[k][dn][row of k][g] = the partials of region g's waves, added in wave order; a region without a site: 0.  One thread per (region,
// draw, output row), the region slowest: the workspace is wave-major, so the threads of a wave read neighbouring doubles, and the loads
// are issued 32 waves ahead of the additions, which wait for nothing but one another (a grid in one region has 15 625 partials a thread).
// One wave a block: a chunk has few thousand threads, which so spread over the compute units.
__global__ __launch_bounds__(BL_TT_FINISH_THREADS) void bl_trajectory_totals_finish_kernel(const BlTrajectoryTotalsParams p)
{
    const int rows = p.row_first[BL_TT_OUTPUTS], G = p.n_regions;
    const size_t cells = (size_t)(p.n1 - p.n0) * rows;
    const size_t c = (size_t)blockIdx.x * BL_TT_FINISH_THREADS + threadIdx.x;
    if (c >= cells * G) return;
    const int g = (int)(c / cells), r = (int)(c % cells % rows);
    const size_t q = c % cells, dn = q / rows;
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
    // the output the row belongs to: a chain of selects over the unrolled outputs, nothing is indexed by a run-time value
    double *dst = nullptr;
    int local = 0, len = 0;
#pragma unroll
    for (int k = 0; k < BL_TT_OUTPUTS; k++)
        if (r >= p.row_first[k] && r < p.row_first[k + 1]) { dst = p.out[k]; local = r - p.row_first[k]; len = p.row_first[k + 1] - p.row_first[k]; }
    dst[(dn * len + local) * G + g] = sum;
}

extern "C" int bl_launch_trajectory_totals(const BlTrajectoryTotalsParams *p, int grid_y, hipStream_t st)
{
    const int rows = p->row_first[BL_TT_OUTPUTS];
    if (p->n_slots > 0) { // (every site in no region: the totals are the finish kernel's zeros)
        hipLaunchKernelGGL(bl_trajectory_totals_kernel, dim3((p->n_slots + BL_TT_THREADS - 1) / BL_TT_THREADS, grid_y), dim3(BL_TT_THREADS),
                           0, st, *p);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    const size_t cells = (size_t)(p->n1 - p->n0) * rows * p->n_regions;
    hipLaunchKernelGGL(bl_trajectory_totals_finish_kernel, dim3((unsigned)((cells + BL_TT_FINISH_THREADS - 1) / BL_TT_FINISH_THREADS)),
                       dim3(BL_TT_FINISH_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
