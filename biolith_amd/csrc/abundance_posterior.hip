// abundance_posterior.hip -- the kernel of bl_abundance_posterior: per posterior draw and (period, site), with l_n the log of the n-th
// addend of the model's own marginal likelihood over that cell's unmasked replicates,
//   log_lik = logsumexp_n l_n,  N_pmf(n) = exp(l_n - log_lik),  N_mean = sum n N_pmf(n),  occ_prob = 1 - N_pmf(0),  N_i ~ N_pmf.
// occu_rn  (rn_device.hpp; re_kernel.hpp kinds 4 / 5):  l_n = n eta - lgamma(n + 1) - log Z + sum_j log Bernoulli(y_j; f + (1 - f)(1 - q_j^n)),
//          Z = sum_(m <= K) e^(m eta) / m!, q_j = 1 - r_j, f the false-positive rate or 0, every probability clamped to [tiny, 1 - eps]
//          as numpyro clamps it: a non-detection costs max(n log q_j + log(1 - f), log eps), a detection log(clamp(f + (1 - f)(1 - q_j^n))).
// nmixture (occu_device.hpp: bl_eval_sites_nmix; re_kernel.hpp kind 3):  l_n = n eta - lgamma(n + 1) - lambda + sum_j log Binomial(y_j; n, p_j)
//          = a - lambda + n (eta + c) - lgamma(n + 1) + tab[t][n],  a = sum_j y_j nu_j,  c = -sum_j softplus(nu_j),  max_j y_j <= n <= K.
//
// One thread per site, the draws on grid.y: a row is read by 64 neighbouring sites at once, a draw's coefficients are wave-uniform.
// Nothing is kept per n, per visit or per covariate: two passes over n, each forming l_n anew from the rows (the data set is
// L2-resident), so no array with a run-time index exists and nothing goes to scratch.  While no non-detection has reached numpyro's
// floor the non-detections of occu_rn are rank one in n (n sum_j log q_j) and only the detections are visited per n.
//   pass 1  the running maximum and the sum relative to it (rescaled when the maximum moves): log_lik.  It stops at the first n >= lambda
//           whose Poisson part is more than 45 nats below the running maximum: that part falls from there on and every likelihood factor
//           is <= 1, so all later terms are below e^-45 of the largest.
//   pass 2  over the same n: the first moment, the mass at 0 and the draw by inversion of the running sum at u * (pass 1's sum).
// Numerics.  Everything that is formed once per cell is float64: the abundance predictor, the visits' predictors and their log q /
// softplus (the rank-one parts), n eta - lgamma(n + 1) (it cancels from hundreds to a few nats), the weights e^(l_n - max) and the sums
// over n, as bl_predict_kernel's are for the same pmf.  Where nothing was detected and lambda is small the pmf sits on 0, the scale of
// the cell's terms is lambda itself and N_mean = e^(eta + sum_j log q_j) has to be right to an ulp: float32 predictors miss that.
// What is formed per (n, visit) -- a detection's log(f + (1 - f)(1 - q^n)), a floored non-detection -- is float32.
#include "abundance_posterior.hpp"

#include "posterior_math.hpp"
#include "pred_rng.hpp"

namespace {

constexpr float AP_ONE_M_EPS = 0.99999988f;
constexpr double AP_CUT = 45.0;

// 1 - e^x for x <= 0 without cancellation: the series of expm1 down to x = -0.5 (|x|^10 / 10! < 3e-10 of x), 1 - e^x below
__device__ __forceinline__ float ap_one_minus_exp(float x)
{
    float s = fmaf(x, 1.0f / 9.0f, 1.0f);
    s = fmaf(x * (1.0f / 8.0f), s, 1.0f);
    s = fmaf(x * (1.0f / 7.0f), s, 1.0f);
    s = fmaf(x * (1.0f / 6.0f), s, 1.0f);
    s = fmaf(x * (1.0f / 5.0f), s, 1.0f);
    s = fmaf(x * (1.0f / 4.0f), s, 1.0f);
    s = fmaf(x * (1.0f / 3.0f), s, 1.0f);
    s = fmaf(x * 0.5f, s, 1.0f);
    return x > -0.5f ? -x * s : 1.0f - bl_exp(x);
}

// log(1 + e^x) in float64
__device__ __forceinline__ double ap_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

} // namespace

template <bool NMIX>
__global__ void bl_abundance_posterior_kernel(const BlAbundPostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const float *__restrict__ rows = p.rows;
    const int ns = p.ns, N = p.N, T = p.T, J = p.J, K = p.K, Ko = p.Ko;
    for (int d = p.n0 + blockIdx.y; d < p.n1; d += gridDim.y) {
        const float *__restrict__ th = p.draws + (size_t)d * p.D;
        const float *__restrict__ al = th + p.o_al;
        double etad = (double)th[0];
        for (int k = 0; k < p.Ks; k++) etad = fma((double)rows[(size_t)k * ns + i], (double)th[k + 1], etad);
        if (p.c.o_u >= 0) etad += (double)th[p.c.o_u + i];
        const float vi = p.c.o_v >= 0 ? th[p.c.o_v + i] : 0.0f;
        const float lam = bl_exp(fminf((float)etad, 80.0f)); // (the stopping rule's only: n >= lambda)
        // what every l_n carries besides n eta - lgamma(n + 1): -lambda (nmixture), -log Z (occu_rn; Z over 0 .. K)
        double shift;
        float fpr = 0.0f, gq = 1.0f, lgq = 0.0f; // occu_rn: the rate f, 1 - f, log(1 - f)
        double lgqd = 0.0;
        if constexpr (NMIX) {
            shift = -exp(etad);
        } else {
            double m0 = 0.0;
            for (int n = 1; n <= K; n++) m0 = fmax(m0, fma((double)n, etad, -(double)BL_LGAMMA1P[n]));
            double sz = 0.0;
            for (int n = 0; n <= K; n++) {
                const double pn = fma((double)n, etad, -(double)BL_LGAMMA1P[n]) - m0;
                if (pn > -AP_CUT) sz += exp(pn);
            }
            shift = -(m0 + log(sz));
            if (p.c.o_fp >= 0) {
                const float phi = th[p.c.o_fp];
                post_sig(phi, fpr, gq);
                lgqd = -ap_softplus((double)phi);
                lgq = (float)lgqd;
            }
        }
        for (int t = 0; t < T; t++) {
            // occu_rn, per (n, visit): a visit's predictor c nu in float32 (the rows are sign-folded; c = 0: masked)
            [[maybe_unused]] auto visit = [&](int j, float &c) -> float {
                const int v = t * J + j;
                const size_t r = (size_t)(p.r0 + v * p.vw) * ns + i;
                float re = vi;
                if (p.c.o_e >= 0) re += th[(size_t)p.c.o_e + (size_t)i * T * J + v];
                c = rows[r];
                float u = c * al[0];
                for (int k = 1; k <= Ko; k++) u = fmaf(rows[r + (size_t)k * ns], al[k], u);
                return fmaf(c, re, u);
            };
            // a visit's predictor nu in float64, for the pass over the visits that is made once per cell (m = 0 or c = 0: masked)
            auto visit_d = [&](int j, float &c) -> double {
                const int v = t * J + j;
                const size_t r = (size_t)(p.r0 + v * p.vw) * ns + i;
                double u = (double)al[0] + (double)vi;
                if (p.c.o_e >= 0) u += (double)th[(size_t)p.c.o_e + (size_t)i * T * J + v];
                c = rows[NMIX ? r + ns : r];
                const double sg = NMIX ? 1.0 : (double)c; // (c w_k) c = w_k
                for (int k = 0; k < Ko; k++) u = fma((double)rows[r + (size_t)((NMIX ? 2 : 1) + k) * ns] * sg, (double)al[k + 1], u);
                return u;
            };
            // ---- the visits once, in float64: what of them is rank one in n ----
            // nmixture: l_n = a + shift + n slope - lgamma(n + 1) + tab_n;  occu_rn: the non-detections' n cnon + a while none is floored
            double a = 0.0, slope = etad, cnon = 0.0;
            float nn = 0.0f, nd = 0.0f, lqmin = 0.0f; // occu_rn: unmasked non-detections / detections, the smallest log q of a non-detection
            int lo = 0;
            const float *__restrict__ tb = nullptr;
            if constexpr (NMIX) {
                for (int j = 0; j < J; j++) {
                    float mk;
                    const double nu = visit_d(j, mk);
                    if (mk == 0.0f) continue;
                    const float ym = rows[(size_t)(p.r0 + (t * J + j) * p.vw) * ns + i];
                    a = fma((double)ym, nu, a);
                    slope -= ap_softplus(nu); // log(1 - p) = -softplus(nu)
                }
                lo = min(max((int)rows[(size_t)(p.r_ymax + t) * ns + i], 0), K); // the cell's largest count
                tb = p.tab + (size_t)t * (K + 1) * ns + i;
            } else {
                for (int j = 0; j < J; j++) {
                    float c;
                    const double nu = visit_d(j, c);
                    if (c > 0.0f) nd += 1.0f;
                    if (c >= 0.0f) continue;
                    const double lq = -ap_softplus(nu); // log q = log(1 - r)
                    cnon += lq;
                    nn += 1.0f;
                    lqmin = fminf(lqmin, (float)lq);
                }
                a = (double)nn * lgqd;
            }
            // l_n, and its Poisson part (an upper bound of l_n: every likelihood factor is <= 1)
            auto term = [&](int n, double &pois) -> double {
                pois = fma((double)n, etad, -(double)BL_LGAMMA1P[n]) + shift;
                if constexpr (NMIX) {
                    return fma((double)n, slope, -(double)BL_LGAMMA1P[n]) + (a + shift) + (double)tb[(size_t)n * ns];
                } else {
                    double s = pois;
                    const float nf = (float)n;
                    const bool open = fmaf(nf, lqmin, lgq) > POST_LOG_EPS; // no non-detection is at numpyro's floor: rank one in n
                    if (open) s += fma((double)n, cnon, a);
                    if (nd > 0.0f || !open)
                        for (int j = 0; j < J; j++) {
                            float c;
                            const float u = visit(j, c);
                            if (c == 0.0f || (c < 0.0f && open)) continue;
                            const float l1 = post_log1p(bl_exp(-fabsf(u)));
                            if (c < 0.0f) {
                                s += (double)fmaxf(fmaf(nf, fminf(u, 0.0f) - l1, lgq), POST_LOG_EPS);
                            } else { // P(y = 1 | n) = f + (1 - f)(1 - q^n), q^n = e^(n log q), log q = log sigma(-u)
                                const float pd = ap_one_minus_exp(nf * (fminf(-u, 0.0f) - l1));
                                s += (double)bl_log(fmaxf(fminf(fmaf(gq, pd, fpr), AP_ONE_M_EPS), POST_TINY));
                            }
                        }
                    return s;
                }
            };
            // ---- pass 1: the maximum, the sum relative to it, the last n that matters ----
            double mx = 0.0, S = 0.0;
            int hi = K;
            for (int n = lo; n <= K; n++) {
                double pois;
                const double ln = term(n, pois);
                if (n == lo || ln > mx) {
                    S = (n == lo ? 0.0 : S * exp(fmax(mx - ln, -700.0))) + 1.0;
                    mx = ln;
                } else if (ln - mx > -AP_CUT)
                    S += exp(ln - mx);
                if ((float)n >= lam && pois < mx - AP_CUT) { hi = n; break; }
            }
            float l = (float)(mx + log(S));
            if (!NMIX && nn + nd == 0.0f) l = 0.0f; // nothing observed: the likelihood is 1 (nmixture: log P(N <= K), as the model has it)
            const size_t o = ((size_t)(d - p.n0) * T + t) * N + i;
            if (p.log_lik) p.log_lik[o] = l;
            if (!p.n_mean && !p.occ_prob && !p.n_draw) continue;
            // ---- pass 2: the first moment, the mass at 0, the draw by inversion ----
            BlPredRng rng = bl_cell_rng(p.seed, d, T, t, N, i);
            const double target = (double)rng.uniform() * S;
            double S1 = 0.0, cum = 0.0, w0 = 0.0;
            int draw = -1, last = lo;
            for (int n = lo; n <= hi; n++) {
                double pois;
                const double dl = term(n, pois) - mx;
                const double w = dl > -AP_CUT ? exp(dl) : 0.0;
                S1 = fma((double)n, w, S1);
                cum += w;
                if (n == 0) w0 = w;
                if (draw < 0 && target < cum) draw = n;
                last = w > 0.0 ? n : last;
            }
            if (draw < 0) draw = last; // (the running sum fell short of u * S by rounding: the last n with mass)
            if (p.n_mean) p.n_mean[o] = (float)(S1 / cum);
            if (p.occ_prob) p.occ_prob[o] = (float)((cum - w0) / cum);
            if (p.n_draw) p.n_draw[o] = draw;
        }
    }
}

extern "C" int bl_launch_abundance_posterior(const BlAbundPostParams *p, int grid_y, hipStream_t st)
{
    dim3 grid, block;
    post_geometry(p->N, grid_y, grid, block);
    if (p->nmix) hipLaunchKernelGGL(bl_abundance_posterior_kernel<true>, grid, block, 0, st, *p);
    else hipLaunchKernelGGL(bl_abundance_posterior_kernel<false>, grid, block, 0, st, *p);
    return (int)hipGetLastError();
}
