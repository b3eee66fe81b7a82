// psis_loo.hip -- the kernels of bl_psis_loo: Pareto-smoothed importance-sampling leave-one-out of every cell of a (draws, cells)
// log-likelihood matrix (BUILDER-DEFINED, the reference has no LOO; the definition is the comment of bl_psis_loo in
// include/biolith_hip.h, its float64 NumPy restatement tests/psis_ref.py).  All arithmetic is float64 on the float32 input.
//
// bl_psis_transpose_kernel: [n][cells] -> [cells][n] through a 32 x 33 LDS tile, so that a cell's draws are contiguous.
//
// bl_psis_loo_kernel: one wave64 (= one workgroup) per cell, the cell's column resident in LDS as float32 (dynamic, 4 n bytes).
//   A  load: the column into LDS, its minimum and maximum, and whether every value is finite (if not: three NaN, nothing else)
//   B  the (M+1)-th smallest ll, exactly, by bisection on the order-preserving integer image of a float: 32 counting passes over the
//      LDS column (ballot + popcount, no atomics); it is the (M+1)-th largest log ratio lr = -ll - max(-ll)
//   C  one pass: the tail {lr > cut} compacted in draw order (ballot prefix), the largest lr outside it, sum exp(ll - max ll) for lppd
//   D  the tail (<= 272) sorted by rank counting, ties by position; x_i = exp(lr_i) - exp(cut)
//   E  the fit: candidate b_j on lane j - 1, each walking the tail in order; the weights, b, k and sigma from LDS in index order
//   F  the tail's smoothed lr; the log-sum-exp of all lr; elpd from the tail's terms and ONE term for the n - M' draws outside it
//      (for them lw + ll = min ll - logsumexp(lr), the same number)
// Every sum is either a serial loop in index order or a lane's strided partial followed by one fixed xor butterfly, so a cell's outputs
// are a function of its column alone -- not of its neighbours, the grid or the chunking -- and two calls return the same bits.  No
// floating-point atomic.  Nothing of the column is private: scratch stays 0 (tests/test_psis_resources.py).
#include "psis_loo.hpp"

#include <cfloat>

namespace {

constexpr double PSIS_LOG_DBL_MIN = -708.3964185322641; // log(DBL_MIN), written out as in tests/psis_ref.py

__device__ __forceinline__ double psis_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v; // every lane: the same sum, in one fixed order
}
__device__ __forceinline__ double psis_wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double psis_wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
// float -> unsigned, ascending with the float (finite values; -0 sorts just below +0, which is all the select needs)
__device__ __forceinline__ unsigned psis_key(float v)
{
    const unsigned b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float psis_unkey(unsigned k)
{
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}

} // namespace

__global__ __launch_bounds__(BL_PSIS_TILE * 8) void bl_psis_transpose_kernel(const BlPsisParams p)
{
    __shared__ float tile[BL_PSIS_TILE][BL_PSIS_TILE + 1];
    const int tx = threadIdx.x, ty = threadIdx.y; // 32 x 8
    const size_t c0 = (size_t)blockIdx.x * BL_PSIS_TILE;
    const int s0 = blockIdx.y * BL_PSIS_TILE;
    for (int r = ty; r < BL_PSIS_TILE; r += 8) {
        const int s = s0 + r;
        const size_t c = c0 + tx;
        if (s < p.n && c < (size_t)p.cells) tile[r][tx] = p.in[(size_t)s * p.cells + c];
    }
    __syncthreads();
    for (int r = ty; r < BL_PSIS_TILE; r += 8) {
        const size_t c = c0 + r;
        const int s = s0 + tx;
        if (s < p.n && c < (size_t)p.cells) p.cols[c * p.n + s] = tile[tx][r];
    }
}

__global__ __launch_bounds__(64) void bl_psis_loo_kernel(const BlPsisParams p)
{
    extern __shared__ float col[];                 // [n]
    __shared__ float t_raw[BL_PSIS_TAIL_MAX];      // the tail's ll in draw order
    __shared__ float t_ll[BL_PSIS_TAIL_MAX];       // ... by descending ll = ascending lr
    __shared__ double t_x[BL_PSIS_TAIL_MAX];       // exceedances, ascending
    __shared__ double t_v[BL_PSIS_TAIL_MAX];       // the fit's log1p terms, then the tail's final lr
    __shared__ double c_b[BL_PSIS_CAND_MAX], c_L[BL_PSIS_CAND_MAX], c_w[BL_PSIS_CAND_MAX];

    const int lane = threadIdx.x, n = p.n;
    const size_t cell = blockIdx.x;
    const float *src = p.cols + cell * n;
    double *out = p.out + cell;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- A: load
    double mn = INFINITY, mx = -INFINITY;
    bool bad = false;
    for (int s = lane; s < n; s += 64) {
        const float v = src[s];
        col[s] = v;
        bad |= !isfinite(v);
        mn = fmin(mn, (double)v);
        mx = fmax(mx, (double)v);
    }
    if (__any(bad)) { // (wave-uniform: the whole workgroup leaves)
        if (lane == 0) { out[0] = nan; out[p.cells] = nan; out[2 * (size_t)p.cells] = nan; }
        return;
    }
    mn = psis_wave_min(mn);
    mx = psis_wave_max(mx);
    const double negmax = -mn; // max(-ll)
    __syncthreads();

    // ---- B: the key of rank r (0-based, ascending) = the largest K with #{key < K} <= r
    const int r = p.tail < n - 1 ? p.tail : n - 1;
    unsigned K = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const unsigned cand = K | (1u << bit);
        int cnt = 0;
        for (int s0 = 0; s0 < n; s0 += 64) {
            const int s = s0 + lane;
            cnt += __popcll(__ballot(s < n && psis_key(col[s]) < cand));
        }
        if (cnt <= r) K = cand;
    }
    const double lr_sel = -(double)psis_unkey(K) - negmax;
    const double cut = fmax(lr_sel, PSIS_LOG_DBL_MIN);

    // ---- C: the tail in draw order, the largest lr outside it, lppd's sum
    int Mp = 0;
    double rest_max = -INFINITY, s_ll = 0.0;
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int s = s0 + lane;
        const bool live = s < n;
        const float v = live ? col[s] : 0.0f;
        const double lr = -(double)v - negmax;
        const bool in_tail = live && lr > cut;
        const unsigned long long mask = __ballot(in_tail);
        const int pos = Mp + __popcll(mask & ((1ull << lane) - 1ull));
        if (in_tail && pos < BL_PSIS_TAIL_MAX) t_raw[pos] = v; // (pos <= M - 1 by the definition of cut; the bound is a guard)
        Mp += __popcll(mask);
        if (live && !in_tail) rest_max = fmax(rest_max, lr);
        if (live) s_ll += exp((double)v - mx);
    }
    if (Mp > BL_PSIS_TAIL_MAX) Mp = BL_PSIS_TAIL_MAX;
    rest_max = psis_wave_max(rest_max);
    s_ll = psis_wave_sum(s_ll);
    __syncthreads();

    // ---- D: sort by rank counting (descending ll, ties in draw order), then the exceedances
    for (int i = lane; i < Mp; i += 64) {
        const float v = t_raw[i];
        int rank = 0;
        for (int j = 0; j < Mp; j++) {
            const float u = t_raw[j];
            rank += (u > v || (u == v && j < i)) ? 1 : 0;
        }
        t_ll[rank] = v;
    }
    __syncthreads();
    const double ecut = exp(cut);
    for (int i = lane; i < Mp; i += 64) t_x[i] = exp(-(double)t_ll[i] - negmax) - ecut;
    __syncthreads();

    // ---- E: the generalised-Pareto fit
    double k = INFINITY, sigma = 0.0;
    if (Mp > 4) {
        const double dM = (double)Mp;
        const int m = 30 + (int)floor(sqrt(dM));
        const double xq = t_x[(int)floor(dM / 4.0 + 0.5) - 1], xmax = t_x[Mp - 1];
        if (lane < m) {
            const double bj = (1.0 - sqrt((double)m / ((double)(lane + 1) - 0.5))) / (3.0 * xq) + 1.0 / xmax;
            double acc = 0.0;
            for (int i = 0; i < Mp; i++) acc += log1p(-bj * t_x[i]);
            const double kkj = acc / dM;
            c_b[lane] = bj;
            c_L[lane] = dM * (log(-bj / kkj) - kkj - 1.0);
        }
        __syncthreads();
        if (lane < m) {
            const double Lj = c_L[lane];
            double acc = 0.0;
            for (int l = 0; l < m; l++) acc += exp(c_L[l] - Lj);
            const double w = 1.0 / acc;
            c_w[lane] = (w < 10.0 * DBL_EPSILON) ? 0.0 : w;
        }
        __syncthreads();
        double wsum = 0.0;
        for (int l = 0; l < m; l++) wsum += c_w[l];
        double b = 0.0;
        for (int l = 0; l < m; l++) b += (c_w[l] / wsum) * c_b[l];
        for (int i = lane; i < Mp; i += 64) t_v[i] = log1p(-b * t_x[i]);
        __syncthreads();
        double acc = 0.0;
        for (int i = 0; i < Mp; i++) acc += t_v[i];
        const double kk = acc / dM;
        sigma = -kk / b;
        k = (dM * kk + 5.0) / (dM + 10.0);
        __syncthreads(); // (t_v is written again below)
    }

    // ---- F: the tail's final lr, logsumexp(lr), elpd
    const bool smooth = Mp > 4 && isfinite(k);
    double tail_max = -INFINITY;
    for (int i = lane; i < Mp; i += 64) {
        double v = -(double)t_ll[i] - negmax;
        if (smooth) {
            const double l1p = log1p(-((double)i + 0.5) / (double)Mp);
            const double q = fabs(k) < 1e-15 ? -l1p : expm1(-k * l1p) / k;
            v = log(sigma * q + ecut);
            v = v > 0.0 ? 0.0 : v;
        }
        t_v[i] = v;
        tail_max = fmax(tail_max, v);
    }
    tail_max = psis_wave_max(tail_max);
    __syncthreads();
    const double top = fmax(rest_max, tail_max);
    double s_lr = 0.0;
    for (int s = lane; s < n; s += 64) {
        const double lr = -(double)col[s] - negmax;
        if (!(lr > cut)) s_lr += exp(lr - top);
    }
    for (int i = lane; i < Mp; i += 64) s_lr += exp(t_v[i] - top);
    const double lse = top + log(psis_wave_sum(s_lr));
    // lw + ll: outside the tail (-ll - max(-ll)) - lse + ll = min ll - lse for every draw; in the tail (lr' - lse) + ll
    const int n_rest = n - Mp;
    const double rest = mn - lse;
    double e_top = n_rest > 0 ? rest : -INFINITY;
    for (int i = lane; i < Mp; i += 64) e_top = fmax(e_top, (t_v[i] - lse) + (double)t_ll[i]);
    e_top = psis_wave_max(e_top);
    double s_e = 0.0;
    for (int i = lane; i < Mp; i += 64) s_e += exp((t_v[i] - lse) + (double)t_ll[i] - e_top);
    s_e = psis_wave_sum(s_e);
    if (n_rest > 0) s_e += (double)n_rest * exp(rest - e_top);
    if (lane == 0) {
        out[0] = e_top + log(s_e);
        out[p.cells] = k;
        out[2 * (size_t)p.cells] = mx + log(s_ll) - log((double)n);
    }
}

extern "C" int bl_launch_psis_loo(const BlPsisParams *p, hipStream_t st)
{
    const dim3 tgrid((unsigned)((p->cells + BL_PSIS_TILE - 1) / BL_PSIS_TILE), (unsigned)((p->n + BL_PSIS_TILE - 1) / BL_PSIS_TILE));
    hipLaunchKernelGGL(bl_psis_transpose_kernel, tgrid, dim3(BL_PSIS_TILE, 8), 0, st, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(bl_psis_loo_kernel, dim3((unsigned)p->cells), dim3(64), (size_t)p->n * sizeof(float), st, *p);
    return (int)hipGetLastError();
}
