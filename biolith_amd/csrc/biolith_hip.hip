// biolith_hip.hip -- host side of the C-ABI in include/biolith_hip.h (+ the small non-templated kernels).
//
// Everything numpyro did behind `mcmc.run` (biolith/utils/fit.py:128-130) for the occu model is
// reached through these entry points.  No CPU fallback exists: without a HIP device every compute
// entry point returns BL_ERR_NO_DEVICE.
#include "../../include/biolith_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "logp_kernel.hpp"
#include "re_kernel.hpp"
#include "nuts_kernel.hpp"
#include "predict.hpp"
#include "site_posterior.hpp"
#include "abundance_posterior.hpp"
#include "path_posterior.hpp"
#include "score_posterior.hpp"
#include "count_posterior.hpp"
#include "comb_predict.hpp"
#include "predictive_check.hpp"
#include "predictive_check_counts.hpp"
#include "predictive_density.hpp"
#include "psis_loo.hpp"
#include "site_summary.hpp"
#include "site_diagnostics.hpp"
#include "regional_totals.hpp"
#include "response_curves.hpp"
#include "trajectory_totals.hpp"
#include "species_richness.hpp"
#include "residual_moran.hpp"

// ------------------------------------------------------------------ errors ----
static thread_local std::string g_err;
static thread_local char g_kernel_name[160]; // the sampler instantiation the last launch of this thread picked (kernels_inst.hip: bl_launch)
static int bl_fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define BL_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess)                                                                         \
            return bl_fail(BL_ERR_NO_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),   \
                           __FILE__, __LINE__);                                                        \
    } while (0)

// Scratch device allocations of one call: freed on every return path.
struct DevScratch {
    std::vector<void *> ptrs;
    ~DevScratch() { for (void *q : ptrs) hipFree(q); }
    hipError_t alloc(void **out, size_t bytes)
    {
        const hipError_t e = hipMalloc(out, bytes ? bytes : 1);
        if (e == hipSuccess) ptrs.push_back(*out);
        return e;
    }
};

// ------------------------------------------- kernel instantiation dispatch ----
#if defined(BL_STAMPS) || defined(BL_ONLY33) /* diagnostic / experimental builds: one instantiation */
#define BL_KK_LIST(X) X(3, 3)
#else
#define BL_K_LIST(X, a) X(a, 1) X(a, 2) X(a, 3) X(a, 4) X(a, 8) X(a, 16)
#define BL_KK_LIST(X) BL_K_LIST(X, 1) BL_K_LIST(X, 2) BL_K_LIST(X, 3) BL_K_LIST(X, 4) BL_K_LIST(X, 8) BL_K_LIST(X, 16)
#endif
#define BL_DECL(ks, ko)                                                                                        \
    extern "C" int bl_launch_nuts_##ks##_##ko(const BlNutsParams *, int, int, int, int, hipStream_t);          \
    extern "C" int bl_launch_logp_##ks##_##ko(const BlLogpParams *, int, int, int, int, hipStream_t);
BL_KK_LIST(BL_DECL)

typedef int (*nuts_launch_fn)(const BlNutsParams *, int, int, int, int, hipStream_t);
typedef int (*logp_launch_fn)(const BlLogpParams *, int, int, int, int, hipStream_t);
struct KernelEntry {
    int ks, ko;
    nuts_launch_fn nuts;
    logp_launch_fn logp;
};
#define BL_ENTRY(ks, ko) {ks, ko, bl_launch_nuts_##ks##_##ko, bl_launch_logp_##ks##_##ko},
static const KernelEntry g_kernels[] = {BL_KK_LIST(BL_ENTRY)};

static int pad_covs(int k)
{
    if (k <= 1) return 1;
    if (k <= 4) return k;
    if (k <= 8) return 8;
    return 16;
}
static const KernelEntry *find_kernels(int KS, int KO)
{
    for (const auto &e : g_kernels)
        if (e.ks == KS && e.ko == KO) return &e;
    return nullptr;
}

// ------------------------------------------------------------- host RNG ----
// xoshiro128++ 1.0 with jump(); stream (chain, s) = base advanced by chain*64+s jumps.
static inline uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
static uint32_t xo_next(uint32_t s[4])
{
    const uint32_t result = rotl32(s[0] + s[3], 7) + s[0];
    const uint32_t t = s[1] << 9;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
    s[2] ^= t;
    s[3] = rotl32(s[3], 11);
    return result;
}
static void xo_jump(uint32_t s[4])
{
    static const uint32_t JUMP[4] = {0x8764000bu, 0xf542d2d3u, 0x6fa035c3u, 0x77f2db5bu};
    uint32_t t[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++)
        for (int b = 0; b < 32; b++) {
            if (JUMP[i] & (1u << b)) { t[0] ^= s[0]; t[1] ^= s[1]; t[2] ^= s[2]; t[3] ^= s[3]; }
            xo_next(s);
        }
    memcpy(s, t, sizeof t);
}
static uint64_t splitmix64(uint64_t &x)
{
    uint64_t z = (x += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static void rng_streams(uint64_t seed, int chain, int nstreams, uint32_t *out)
{
    uint64_t sm = seed;
    const uint64_t a = splitmix64(sm), b = splitmix64(sm);
    uint32_t s[4] = {(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
    if (!(s[0] | s[1] | s[2] | s[3])) s[0] = 1;
    for (long k = 0; k < (long)chain * BL_RNG_STREAMS_PER_CHAIN; k++) xo_jump(s);
    for (int k = 0; k < nstreams; k++) {
        memcpy(out + 4 * k, s, sizeof s);
        xo_jump(s);
    }
}

// Streams of `nchains` consecutive chains at `stride` streams per chain (stream (c, s) = base advanced by c * stride + s
// jumps, like rng_streams with its stride of 64): out[(c - first_chain) * stride + s].
static void rng_streams_strided(uint64_t seed, int first_chain, int stride, int nchains, uint32_t *out)
{
    uint64_t sm = seed;
    const uint64_t a = splitmix64(sm), b = splitmix64(sm);
    uint32_t s[4] = {(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
    if (!(s[0] | s[1] | s[2] | s[3])) s[0] = 1;
    for (long long k = 0; k < (long long)first_chain * stride; k++) xo_jump(s);
    for (long long k = 0; k < (long long)nchains * stride; k++) {
        memcpy(out + 4 * k, s, sizeof s);
        xo_jump(s);
    }
}

static int adaptation_schedule(int num_steps, int32_t *starts, int32_t *ends, int cap)
{
    // numpyro.infer.hmc_util.build_adaptation_schedule
    int n = 0;
    auto push = [&](int s, int e) { if (n < cap) { starts[n] = s; ends[n] = e; } n++; };
    if (num_steps <= 0) return 0;
    if (num_steps < 20) { push(0, num_steps - 1); return n; }
    int start_buffer = 75, end_buffer = 50, init_window = 25;
    if (start_buffer + end_buffer + init_window > num_steps) {
        start_buffer = (int)(0.15 * num_steps);
        end_buffer = (int)(0.1 * num_steps);
        init_window = num_steps - start_buffer - end_buffer;
    }
    push(0, start_buffer - 1);
    const int end_window_start = num_steps - end_buffer;
    int next_size = init_window, next_start = start_buffer;
    while (next_start < end_window_start) {
        int cur_start = next_start, cur_size = next_size;
        if (3 * cur_size <= end_window_start - cur_start) next_size = 2 * cur_size;
        else cur_size = end_window_start - cur_start;
        next_start = cur_start + cur_size;
        push(cur_start, next_start - 1);
    }
    push(end_window_start, num_steps - 1);
    return n;
}

// ----------------------------------------------------------------- handle ----
struct bl_dataset {
    int device = 0;
    int model = 0;          // 0 occu, 1 occu_rn, 2 occu with false positives, 3 occu_cop, 4 nmixture, 6 occu with random effects
    BlReModel re{};         // model 6 (re_kernel.hpp); D is then the full coordinate count
    BlCombModel comb{};     // model 6 kind 8 (occu_comb): its blocks' shapes and rate priors
    float *d_restate = nullptr; // model 6: sampler state [C][k][RE_SLOTS][dl_max]
    size_t restate_bytes = 0;
    float *d_tab = nullptr; // nmixture: B[t][n][site] = sum_j m log C(n, y_j), -inf below the largest count
    int ko_layout = 0;      // KO the record layout helpers are called with (KO, or KO + 1 for occu_cop's wider visits)
    int max_abundance = 0;  // occu_rn only
    int fp_mode = 0;        // model 2: BL_FP_CONSTANT / BL_FP_UNOCCUPIED
    double fp_a = 2.0, fp_b = 5.0;  // model 2: Beta prior of the false-positive rate
    bl_dims dims{};
    int Ks = 0, Ko = 0, KS = 0, KO = 0, D = 0;
    int nsp = 1;            // species sampled jointly by this handle (models 0 and 2)
    int n_stride = 0, n_rows = 0;
    float *d_rows = nullptr;
    BlDevData dd{};
    const KernelEntry *kern = nullptr;
    bl_normal_prior pb{}, pa{};
    int fam_b = 0, fam_a = 0; // BL_PRIOR_NORMAL / BL_PRIOR_LAPLACE (bl_dataset_set_prior_family)
    // raw nan_to_num'd obs covariates, site-fastest [V][Ko][n_stride], for prob_detection (lazy upload)
    std::vector<float> h_wraw;
    float *d_wraw = nullptr;
    // occu_comb: the same for the ARU block, [T Jaru][Karu][n_stride], for bl_predict_comb / bl_deterministic_comb (lazy upload; h_wraw
    // holds the point counts', Kpc wide)
    std::vector<float> h_araw;
    float *d_araw = nullptr;
    // occu_cop: raw session durations, site-fastest [V][n_stride], for the predictive counts (lazy upload)
    std::vector<float> h_dur;
    float *d_dur = nullptr;
    // occu_cop: per cell, the sum over its unmasked visits of y log(dur) - lgamma(y + 1), site-fastest [T][n_stride], for
    // bl_count_posterior (lazy upload)
    std::vector<float> h_ccell;
    float *d_ccell = nullptr;
    // ---- last NUTS launch ----
    bool in_flight = false, have_run = false;
    int C = 0, S = 0, W = 0, k = 0, nloc = 0, lds_ld = 0, lds_bytes = 0, staged = 0, nvp = 0, ncw = 0, lane_grp = 0;
    char kernel_name[160] = {0}; // the sampler instantiation of the last launch, as rocprofv3 names it
    char env_overrides[512] = {0}; // BIOLITH_HIP_* knobs that were set when the last launch read the environment (bl_env_snapshot)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void *d_run = nullptr;  // one slab for all run buffers
    size_t run_bytes = 0;
    float *d_draws = nullptr, *d_acc = nullptr, *d_pot = nullptr, *d_eps = nullptr, *d_minv = nullptr, *d_init = nullptr;
    unsigned char *d_div = nullptr;
    int *d_steps = nullptr, *d_status = nullptr;
    long long *d_nleap = nullptr, *d_dbg = nullptr;
    int *d_loc = nullptr;
    uint32_t *d_rng = nullptr;
    float *d_scores = nullptr; // occu_cs: scores, site-fastest [T J][n_stride]; occu_comb: its own rows (re_kernel.hpp: bl_comb_site_pass)
    unsigned long long *d_xchg = nullptr;
    size_t xchg_bytes = 0;
    int *h_abort = nullptr, *d_abort = nullptr;
};


// ------------------------------------------------------------------------------------------ environment knobs ----
// Every environment variable the launch path looks at, in ONE table (INTEGRATION.md lists them with their meaning).  None is needed in
// production: they force a geometry or a kernel form for tests, A/B runs and measurement.  They are read in ONE place --
// bl_env_snapshot(), at the top of the public entries that can reach one (dataset creation, bl_logp_grad, bl_nuts_launch) -- so a launch
// sees one consistent set, and bl_env_overrides() / bl_nuts_env_overrides() report the ones that were set (bench.py prints them: a
// stray variable must not change a geometry silently).  A snapshot per entry rather than per process: the parity tests switch forms
// between two launches of one process (tests/test_gpu_kernel_forms.py, test_gpu_re.py).
#define BL_ENV_TABLE(X) X(DYN_G) X(GRP_VISITS) X(OCCU_G) X(OCCU_GT) X(SINGLE) X(CWAVES) X(NO_WIDE) X(RN_K) X(WIDE_K) X(NMIX_LDS) X(RE_EFF) \
    X(RE_NO_SPLIT) X(RE_LDS_ROWS) X(RE_LDS_TIER) X(RE_WGS) X(NO_LOCAL) X(PITCH) X(GRP_KERNEL) X(SPIN_US) X(POLL_SLEEP) X(FIRST_DELAY) X(GENERAL)
enum bl_env_knob {
#define X(n) BL_ENV_##n,
    BL_ENV_TABLE(X)
#undef X
    BL_ENV_COUNT
};
static const char *const BL_ENV_NAMES[BL_ENV_COUNT] = {
#define X(n) "BIOLITH_HIP_" #n,
    BL_ENV_TABLE(X)
#undef X
};
struct bl_env_config {
    bool set[BL_ENV_COUNT] = {};
    char val[BL_ENV_COUNT][32] = {};
};
static bl_env_config g_env;
static void bl_env_snapshot()
{
    for (int i = 0; i < BL_ENV_COUNT; i++) {
        const char *e = getenv(BL_ENV_NAMES[i]);
        g_env.set[i] = e != nullptr;
        snprintf(g_env.val[i], sizeof g_env.val[i], "%s", e ? e : "");
    }
}
// the knob's value at the last snapshot, or NULL when it was not set
static const char *bl_env(bl_env_knob k) { return g_env.set[k] ? g_env.val[k] : nullptr; }
static std::string bl_env_active()
{
    std::string out;
    for (int i = 0; i < BL_ENV_COUNT; i++)
        if (g_env.set[i]) out += (out.empty() ? "" : ",") + std::string(BL_ENV_NAMES[i]) + "=" + g_env.val[i];
    return out;
}
extern "C" int bl_env_force_general(void) { const char *e = bl_env(BL_ENV_GENERAL); return e && e[0] == '1'; } // (kernels_inst.hip)
extern "C" int bl_env_overrides(char *buf, int n)
{
    if (!buf || n <= 0) return bl_fail(BL_ERR_INVALID, "NULL argument");
    bl_env_snapshot();
    snprintf(buf, (size_t)n, "%s", bl_env_active().c_str());
    return BL_OK;
}

static int set_device(const bl_dataset *ds)
{
    BL_HIP(hipSetDevice(ds->device));
    return BL_OK;
}

extern "C" int bl_abi_version(void) { return BL_ABI_VERSION; }
extern "C" const char *bl_last_error(void) { return g_err.c_str(); }

extern "C" int bl_device_count(int *count)
{
    if (!count) return bl_fail(BL_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return bl_fail(BL_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return BL_OK;
}

// ------------------------------------------------------------------ the per-draw entries ----
// bl_predict, bl_predict_scores, bl_predict_counts, bl_predict_comb, bl_deterministic_comb, bl_predictive_check, bl_site_posterior, bl_abundance_posterior, bl_path_posterior, bl_score_posterior and
// bl_count_posterior run one kernel over (site, posterior draw).  What they share is stated once: the name of a handle's model, the checks in front, the rows that go up on
// first use, and the driver that takes the draws through the kernel in chunks.

// The handle's model as the Python layer names it -- the one spelling every refusal uses.
static const char *model_name(const bl_dataset *ds)
{
    static const char *const plain[] = {"occu", "occu_rn", "occu_fp (occu with false positives)", "occu_cop", "nmixture"};
    static const char *const re_kind[] = {"occu_re (occu with random effects)", "occu_cs", "occu_re (occu with random effects)", "nmixture",
                                          "occu_rn", "occu_rn", "occu_cop", "occu_cop", "occu_comb"};
    if (ds->nsp > 1) return "a joint-species handle (it samples; use one handle per species)";
    if (ds->model >= 0 && ds->model <= 4) return plain[ds->model];
    if (ds->model == 6 && ds->re.kind >= 0 && ds->re.kind <= 8) return re_kind[ds->re.kind];
    return ds->model == 8 ? "occu_dyn" : "this model";
}
// model 6 with one of these re.kind values
static bool re_kind_in(const bl_dataset *ds, std::initializer_list<int> kinds)
{
    return ds->model == 6 && std::find(kinds.begin(), kinds.end(), ds->re.kind) != kinds.end();
}

// The plain model whose branch of a predictive kernel the handle runs: a random-effects handle runs its kind's.
static int branch_model(const bl_dataset *ds)
{
    static const int of_kind[] = {0, 0, 2, 4, 1, 1, 3, 3, 0};
    return ds->model == 6 && ds->re.kind >= 0 && ds->re.kind <= 8 ? of_kind[ds->re.kind] : ds->model;
}
// A handle's draw layout as the post-fit kernels are told it: o_fp is the false-positive coordinate if the handle has one (behind the
// coefficients with random effects, else the last one) and fp_mode its mode, else -1 and 0; the effects' offsets, -1 = absent.
static BlDrawCoords draw_coords(const bl_dataset *ds)
{
    const bool re = ds->model == 6;
    BlDrawCoords c;
    c.fp_mode = re ? ds->re.fp_mode : ds->fp_mode;
    c.o_fp = c.fp_mode ? (re ? ds->re.o_fp : ds->D - 1) : -1;
    c.o_u = re ? ds->re.o_u : -1; c.o_v = re ? ds->re.o_v : -1; c.o_e = re ? ds->re.o_e : -1;
    return c;
}

// What every per-draw entry checks before it touches the device.  `serves`: does the entry serve this handle; `built`: what it does serve.
static int per_draw_front(const char *entry, const bl_dataset *ds, int n_draws, const float *draws, bool any_output,
                          bool (*serves)(const bl_dataset *), const char *built)
{
    if (!ds || !draws || n_draws <= 0 || !any_output) return bl_fail(BL_ERR_INVALID, "%s: bad argument", entry);
    if (!serves(ds)) return bl_fail(BL_ERR_UNSUPPORTED, "%s: not built for %s (%s)", entry, model_name(ds), built);
    if (ds->in_flight) return bl_fail(BL_ERR_BUSY, "a NUTS launch is in flight on this handle");
    return set_device(ds);
}

// Rows that only a post-fit kernel reads (the raw observation covariates, occu_cop's durations and per-cell constants) go up on first
// use and stay.
static int upload_once(float **dev, const std::vector<float> &host)
{
    if (*dev) return BL_OK;
    BL_HIP(hipMalloc((void **)dev, host.size() * 4));
    BL_HIP(hipMemcpy(*dev, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    return BL_OK;
}

// One output of a per-draw entry, `bytes` per draw.  *dev receives the device buffer of a chunk of draws, or NULL where the output is
// not wanted (host == NULL and not `always`) or empty; the kernel indexes it from the chunk's first draw.
struct DrawOut {
    void *host;
    size_t bytes;
    void **dev;
    bool always; // allocated also when the caller does not want it back (a kernel's workspace)
};

// Runs launch(d_draws, n0, n1, grid_y) over the draws [n0, n1) in chunks of at most 256 MB / chunk_bytes draws (chunk_bytes: the entry's
// largest output of one draw), grid_y = min(n1 - n0, 1024) rows of draws, and copies every wanted output back to host + n0 * bytes.
// A draw is `width` floats, 0 = the handle's D (bl_species_richness stacks its species' blocks: n_species D).
template <size_t K, class Launch>
static int run_over_draws(const bl_dataset *ds, int n_draws, const float *draws, size_t chunk_bytes, const DrawOut (&outs)[K],
                          Launch launch, size_t width = 0)
{
    DevScratch scratch;
    float *d_draws = nullptr;
    if (!width) width = (size_t)ds->D;
    BL_HIP(scratch.alloc((void **)&d_draws, (size_t)n_draws * width * 4));
    BL_HIP(hipMemcpy(d_draws, draws, (size_t)n_draws * width * 4, hipMemcpyHostToDevice));
    const size_t fit = ((size_t)256 << 20) / std::max<size_t>(1, chunk_bytes); // draws whose largest output fills 256 MB
    const int chunk = (int)std::min<size_t>((size_t)n_draws, std::max<size_t>(1, fit));
    for (const DrawOut &o : outs) {
        *o.dev = nullptr;
        if ((o.host || o.always) && o.bytes) BL_HIP(scratch.alloc(o.dev, (size_t)chunk * o.bytes));
    }
    for (int n0 = 0; n0 < n_draws; n0 += chunk) {
        const int n1 = std::min(n0 + chunk, n_draws);
        BL_HIP(launch(d_draws, n0, n1, std::min(n1 - n0, 1024)));
        for (const DrawOut &o : outs)
            if (o.host && *o.dev)
                BL_HIP(hipMemcpy((char *)o.host + (size_t)n0 * o.bytes, *o.dev, (size_t)(n1 - n0) * o.bytes, hipMemcpyDeviceToHost));
    }
    return BL_OK;
}
// The usual launch: the chunk's draws and bounds into the entry's kernel parameters, then its launcher.
template <size_t K, class Params>
static int run_over_draws(const bl_dataset *ds, int n_draws, const float *draws, size_t chunk_bytes, const DrawOut (&outs)[K], Params &p,
                          int (*launcher)(const Params *, int, hipStream_t))
{
    return run_over_draws(ds, n_draws, draws, chunk_bytes, outs, [&](const float *d_draws, int n0, int n1, int grid_y) {
        p.draws = d_draws; p.n0 = n0; p.n1 = n1;
        return (hipError_t)launcher(&p, grid_y, nullptr);
    });
}

// ------------------------------------------------------------------ posterior predictive ----
// Kernels: predict.hip (bl_predict, bl_predict_counts, bl_predict_scores, bl_deterministic).  What they read of the handle, once the raw
// rows they need are up:
static BlPredictParams predict_params(const bl_dataset *ds, uint64_t seed)
{
    BlPredictParams p{};
    p.rows = ds->d_rows; p.wraw = ds->d_wraw; p.dur = ds->d_dur; p.ns = ds->n_stride;
    p.N = ds->dims.n_sites; p.T = ds->dims.n_periods; p.J = ds->dims.n_replicates; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = ds->D;
    p.model = branch_model(ds); p.K = ds->max_abundance; p.c = draw_coords(ds); p.seed = (unsigned long long)seed;
    return p;
}

extern "C" int bl_predict(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, uint8_t *latent, uint8_t *y)
{
    int rc = per_draw_front("bl_predict", ds, n_draws, draws, latent || y,
                            [](const bl_dataset *d) {
                                return d->nsp == 1 && ((d->model >= 0 && d->model <= 2) || re_kind_in(d, {0, 2, 4, 5}));
                            },
                            "occu, occu_fp, occu_re and occu_rn; the count models use bl_predict_counts, occu_cs bl_predict_scores");
    if (rc || (rc = upload_once(&ds->d_wraw, ds->h_wraw))) return rc;
    BlPredictParams p = predict_params(ds, seed);
    const size_t cells = (size_t)p.T * p.N; // per draw
    const DrawOut outs[] = {{latent, cells, (void **)&p.latent, false}, {y, cells * p.J, (void **)&p.y, false}};
    return run_over_draws(ds, n_draws, draws, cells * (y ? (size_t)p.J : 1), outs, p, bl_launch_predict);
}

// ---- conditional occupancy: P(z | data), the site-period log-likelihood and a draw of z, per posterior draw ----
// (BUILDER-DEFINED: the reference's predict withholds the observations.)  Kernel: site_posterior.hip.  The sign-folded visit rows the
// density kernels read already carry y and the mask, so nothing is uploaded; a draw's layout is bl_predict's.
extern "C" int bl_site_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob, uint8_t *z)
{
    int rc = per_draw_front("bl_site_posterior", ds, n_draws, draws, log_lik || z_prob || z,
                            [](const bl_dataset *d) { return d->nsp == 1 && (d->model == 0 || d->model == 2 || re_kind_in(d, {0, 2, 8})); },
                            "occu, with or without false positives / random effects, and occu_comb");
    if (rc) return rc;
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, D = ds->D;
    BlSitePostParams p{};
    p.ns = ds->n_stride; p.N = N; p.T = T; p.Ks = ds->Ks; p.D = D; p.seed = (unsigned long long)seed;
    p.c = draw_coords(ds);
    if (ds->model == 6 && ds->re.kind == 8) { // occu_comb: its own rows (bl_dataset_create_comb)
        const BlReModel &m = ds->re;
        const BlCombModel &cm = ds->comb;
        p.rows = m.rows; p.comb = 1;
        p.a = BlSitePostBlock{m.rv0, cm.Jpc, cm.Kpc, cm.Kpc + 1, m.Ks + 1};
        p.b = BlSitePostBlock{m.rv0 + cm.r_aru, cm.Jaru, cm.Karu, cm.Karu + 1, m.Ks + cm.Kpc + 2};
        p.r_per = m.rv0 + cm.r_per; p.o_x = m.G0;
    } else {
        const int Ko = ds->model == 6 ? ds->re.Ko : ds->Ko;
        p.rows = ds->d_rows;
        p.a = BlSitePostBlock{ds->KS, ds->dims.n_replicates, Ko, ds->KO + 1, ds->Ks + 1};
        p.b = BlSitePostBlock{0, 0, 0, 1, 0};
    }
    const size_t cells = (size_t)T * N; // per draw; the larger outputs are 4 bytes a cell
    const DrawOut outs[] = {{log_lik, cells * 4, (void **)&p.log_lik, false},
                            {z_prob, cells * 4, (void **)&p.z_prob, false},
                            {z, cells, (void **)&p.z, false}};
    return run_over_draws(ds, n_draws, draws, cells * 4, outs, p, bl_launch_site_posterior);
}

// ---- conditional abundance: P(N | data), the site-period log-likelihood and a draw of N, per posterior draw ----
// (BUILDER-DEFINED: the reference's predict withholds the observations.)  Kernel: abundance_posterior.hip.  It reads the rows the
// samplers read -- occu_rn's sign-folded visits, nmixture's (m y, m, w..) visits, largest-count rows and table of log-binomial sums --
// so nothing is uploaded; a draw's layout is bl_predict's / bl_predict_counts'.
extern "C" int bl_abundance_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *n_mean,
                                      float *occ_prob, int32_t *n_draw)
{
    int rc = per_draw_front("bl_abundance_posterior", ds, n_draws, draws, log_lik || n_mean || occ_prob || n_draw,
                            [](const bl_dataset *d) { return d->nsp == 1 && (d->model == 1 || d->model == 4 || re_kind_in(d, {3, 4, 5})); },
                            "occu_rn, with or without a false-positive rate / random effects, and nmixture, with or without random effects");
    if (rc) return rc;
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, J = ds->dims.n_replicates, D = ds->D;
    BlAbundPostParams p{};
    p.rows = ds->d_rows; p.ns = ds->n_stride; p.N = N; p.T = T; p.J = J; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = D;
    p.r0 = ds->KS; p.vw = ds->KO + 2; p.o_al = ds->Ks + 1; p.seed = (unsigned long long)seed;
    p.c = draw_coords(ds);
    p.nmix = (ds->model == 4 || (ds->model == 6 && ds->re.kind == 3)) ? 1 : 0;
    p.K = ds->model == 6 ? ds->re.max_abundance : ds->max_abundance;
    p.tab = p.nmix ? ds->d_tab : nullptr;
    p.r_ymax = ds->KS + T * J * p.vw;
    if (p.K < 1 || p.K >= BL_RN_NB || (p.nmix && !p.tab)) return bl_fail(BL_ERR_INVALID, "bl_abundance_posterior: the handle carries no abundance table");
    const size_t cells = (size_t)T * N; // per draw; every output is 4 bytes a cell
    const DrawOut outs[] = {{log_lik, cells * 4, (void **)&p.log_lik, false},
                            {n_mean, cells * 4, (void **)&p.n_mean, false},
                            {occ_prob, cells * 4, (void **)&p.occ_prob, false},
                            {n_draw, cells * 4, (void **)&p.n_draw, false}};
    return run_over_draws(ds, n_draws, draws, cells * 4, outs, p, bl_launch_abundance_posterior);
}

// ---- conditional dynamics: the smoothed P(z_t | all seasons' data), the transitions' pairwise terms, the site log-likelihood and a
// joint draw of the path, per posterior draw ----
// (BUILDER-DEFINED, like the model.)  Kernel: path_posterior.hip.  It reads the sign-folded visit rows of the occu_dyn handle, so nothing
// is uploaded; a draw's layout is the sampler's, [b_psi | b_col | b_ext | alpha].  The device z_prob buffer doubles as the kernel's
// workspace (the filtered log-odds), so it is allocated whether or not the caller wants z_prob back.
extern "C" int bl_path_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob,
                                 float *col_prob, float *ext_prob, uint8_t *z)
{
    int rc = per_draw_front("bl_path_posterior", ds, n_draws, draws, log_lik || z_prob || col_prob || ext_prob || z,
                            [](const bl_dataset *d) { return d->model == 8; },
                            "occu_dyn only; the static models' conditionals are bl_site_posterior / bl_abundance_posterior");
    if (rc) return rc;
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, D = ds->D;
    BlPathPostParams p{};
    p.rows = ds->d_rows; p.ns = ds->n_stride; p.N = N; p.T = T; p.J = ds->dims.n_replicates; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = D;
    p.r0 = ds->KS; p.vw = ds->KO + 1; p.seed = (unsigned long long)seed;
    const size_t cells = (size_t)T * N, pairs = (size_t)(T - 1) * N; // per draw; the largest output is 4 bytes a cell
    const DrawOut outs[] = {{log_lik, (size_t)N * 4, (void **)&p.log_lik, false},
                            {z_prob, cells * 4, (void **)&p.z_prob, true},        // (the kernel's workspace)
                            {col_prob, pairs * 4, (void **)&p.col_prob, false},   // (T = 1: empty, skipped)
                            {ext_prob, pairs * 4, (void **)&p.ext_prob, false},
                            {z, cells, (void **)&p.z, false}};
    return run_over_draws(ds, n_draws, draws, cells * 4, outs, p, bl_launch_path_posterior);
}

// ---- conditional scores: P(z | data) and P(f_j | data) of the continuous-score model, the cell log-likelihood and a joint draw of
// (z, f), per posterior draw ----
// (BUILDER-DEFINED: the reference's predict withholds the scores.)  Kernel: score_posterior.hip.  It reads the handle's rows (site
// covariates, the visits' masks), its score rows and the raw observation covariates bl_predict_scores already uses, which go up on
// first use; a draw's layout is the sampler's.  The chunk of draws is sized by f_prob, the largest output, when a visit-level output is wanted.
extern "C" int bl_score_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob, uint8_t *z,
                                  float *f_prob, uint8_t *f)
{
    int rc = per_draw_front("bl_score_posterior", ds, n_draws, draws, log_lik || z_prob || z || f_prob || f,
                            [](const bl_dataset *d) { return re_kind_in(d, {1}); },
                            "occu_cs only; the other models' conditionals are bl_site_posterior / bl_abundance_posterior / bl_path_posterior");
    if (rc || (rc = upload_once(&ds->d_wraw, ds->h_wraw))) return rc;
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, J = ds->dims.n_replicates;
    BlScorePostParams p{};
    p.rows = ds->d_rows; p.wraw = ds->d_wraw; p.scores = ds->re.scores;
    p.ns = ds->n_stride; p.N = N; p.T = T; p.J = J; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = ds->D;
    p.r0 = ds->KS; p.vw = ds->KO + 1; p.seed = (unsigned long long)seed;
    const size_t cells = (size_t)T * N, visits = (size_t)J * cells; // per draw
    const DrawOut outs[] = {{log_lik, cells * 4, (void **)&p.log_lik, false},
                            {z_prob, cells * 4, (void **)&p.z_prob, false},
                            {z, cells, (void **)&p.z, false},
                            {f_prob, visits * 4, (void **)&p.f_prob, false},
                            {f, visits, (void **)&p.f, false}};
    return run_over_draws(ds, n_draws, draws, (f_prob || f ? visits : cells) * 4, outs, p, bl_launch_score_posterior);
}

// ---- conditional counts: P(z | data) of the count-detection model, the cell log-likelihood, and how many of a visit's counted
// detections were real -- their mean and a joint draw of (z, true counts) -- per posterior draw ----
// (BUILDER-DEFINED: the reference's predict withholds the counts.)  Kernel: count_posterior.hip.  It reads the rows the occu_cop samplers
// read (site covariates, the visits' (y_m, d_m, w..), Ysum / Dsum) and one row of its own, the cells' parameter-free constants, which goes
// up on first use; a draw's layout is the sampler's.  The chunk of draws is sized by true_mean, the largest output, when a visit-level
// output is wanted.
extern "C" int bl_count_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob, uint8_t *z,
                                  float *true_mean, int32_t *true_count)
{
    int rc = per_draw_front("bl_count_posterior", ds, n_draws, draws, log_lik || z_prob || z || true_mean || true_count,
                            [](const bl_dataset *d) { return d->nsp == 1 && (d->model == 3 || re_kind_in(d, {6, 7})); },
                            "occu_cop only, with or without a false-positive rate / random effects; the other models' conditionals are "
                            "bl_site_posterior / bl_abundance_posterior / bl_path_posterior / bl_score_posterior");
    if (rc || (rc = upload_once(&ds->d_ccell, ds->h_ccell))) return rc;
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, J = ds->dims.n_replicates;
    BlCountPostParams p{};
    p.rows = ds->d_rows; p.ccell = ds->d_ccell;
    p.ns = ds->n_stride; p.N = N; p.T = T; p.J = J; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = ds->D;
    p.r0 = ds->KS; p.vw = ds->KO + 2; p.r_sum = ds->KS + T * J * p.vw; p.seed = (unsigned long long)seed;
    p.c = draw_coords(ds);
    const size_t cells = (size_t)T * N, visits = (size_t)J * cells; // per draw
    const DrawOut outs[] = {{log_lik, cells * 4, (void **)&p.log_lik, false},
                            {z_prob, cells * 4, (void **)&p.z_prob, false},
                            {z, cells, (void **)&p.z, false},
                            {true_mean, visits * 4, (void **)&p.true_mean, false},
                            {true_count, visits * 4, (void **)&p.true_count, false}};
    return run_over_draws(ds, n_draws, draws, (true_mean || true_count ? visits : cells) * 4, outs, p, bl_launch_count_posterior);
}

// ---- predictive scores of the continuous-score model (occu_cs.py:196-232 with obs=None) ----
extern "C" int bl_predict_scores(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, uint8_t *latent, uint8_t *f, float *s)
{
    int rc = per_draw_front("bl_predict_scores", ds, n_draws, draws, latent || f || s,
                            [](const bl_dataset *d) { return re_kind_in(d, {1}); }, "an occu_cs dataset is required");
    if (rc || (rc = upload_once(&ds->d_wraw, ds->h_wraw))) return rc;
    BlPredictParams p = predict_params(ds, seed);
    const size_t cells = (size_t)p.T * p.N, visits = cells * p.J; // per draw
    const DrawOut outs[] = {{latent, cells, (void **)&p.latent, false}, {f, visits, (void **)&p.f, false}, {s, visits * 4, (void **)&p.s, false}};
    return run_over_draws(ds, n_draws, draws, visits * 4, outs, p, bl_launch_predict_scores);
}

// ---- occu_comb: the posterior predictive of its three observed sites, and its deterministic sites ----
// (bl_predict_comb is BUILDER-DEFINED: the reference's predict cannot withhold the scores from this model.)  Kernels: comb_predict.hip.
// They read the site covariates from the head of the handle's rows and the two detection blocks' raw covariates, which go up on first
// use (the density rows are folded by the observation); a draw's layout is the sampler's.  With no point counts the handle holds a
// one-replicate stand-in: the block is empty here (cm.Jpc = 0).
static bool serves_comb(const bl_dataset *d) { return re_kind_in(d, {8}); }
static int comb_predict_params(bl_dataset *ds, BlCombPredParams &p)
{
    int rc = upload_once(&ds->d_wraw, ds->h_wraw);
    if (rc || (rc = upload_once(&ds->d_araw, ds->h_araw))) return rc;
    const BlReModel &m = ds->re;
    const BlCombModel &cm = ds->comb;
    p.rows = m.rows; p.ns = m.n_stride; p.N = m.n_sites; p.T = m.T; p.Ks = m.Ks; p.D = ds->D;
    p.pc = BlCombPredBlock{cm.Jpc, cm.Kpc, m.Ks + 1, ds->d_wraw};
    p.aru = BlCombPredBlock{cm.Jaru, cm.Karu, m.Ks + cm.Kpc + 2, ds->d_araw};
    p.Js = cm.Jsc; p.o_x = m.G0;
    return BL_OK;
}

extern "C" int bl_predict_comb(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, uint8_t *z, uint8_t *y_pc, uint8_t *y_aru,
                               float *scores)
{
    int rc = per_draw_front("bl_predict_comb", ds, n_draws, draws, z || y_pc || y_aru || scores, serves_comb,
                            "occu_comb only; the other models use bl_predict / bl_predict_counts / bl_predict_scores");
    BlCombPredParams p{};
    if (rc || (rc = comb_predict_params(ds, p))) return rc;
    p.seed = (unsigned long long)seed;
    const size_t cells = (size_t)p.T * p.N; // per draw
    const DrawOut outs[] = {{z, cells, (void **)&p.z, false},
                            {y_pc, cells * p.pc.J, (void **)&p.y_pc, false},   // (an empty block: skipped)
                            {y_aru, cells * p.aru.J, (void **)&p.y_aru, false},
                            {scores, cells * p.Js * 4, (void **)&p.scores, false}};
    size_t largest = cells;
    for (const DrawOut &o : outs) if (o.host) largest = std::max(largest, o.bytes);
    return run_over_draws(ds, n_draws, draws, largest, outs, p, bl_launch_comb_predict);
}

extern "C" int bl_deterministic_comb(bl_dataset *ds, int n_draws, const float *draws, float *psi, float *pc_prob, float *aru_prob)
{
    int rc = per_draw_front("bl_deterministic_comb", ds, n_draws, draws, psi || pc_prob || aru_prob, serves_comb,
                            "occu_comb only; the other models use bl_deterministic");
    BlCombPredParams p{};
    if (rc || (rc = comb_predict_params(ds, p))) return rc;
    const size_t cells = (size_t)p.T * p.N; // per draw
    const DrawOut outs[] = {{psi, cells * 4, (void **)&p.psi, false},
                            {pc_prob, cells * p.pc.J * 4, (void **)&p.pc_prob, false},
                            {aru_prob, cells * p.aru.J * 4, (void **)&p.aru_prob, false}};
    size_t largest = cells * 4;
    for (const DrawOut &o : outs) if (o.host) largest = std::max(largest, o.bytes);
    return run_over_draws(ds, n_draws, draws, largest, outs, p, bl_launch_comb_deterministic);
}

// ---- the posterior predictive check, fused: two discrepancies of the observed and of the replicate data per posterior draw ----
// (biolith/evaluation/posterior_predictive_check.py:17-160 on predict()'s y and psi * prob_detection.)  Kernels: predictive_check.hip.
// They regenerate bl_predict's replicate and bl_deterministic's psi and p, so they read what those read: the head of the handle's rows and
// the raw observation covariates.  The observations come from the caller (the handle's rows fold the covariate masks into theirs; the
// check masks by the observation alone); their count per revisit does not depend on the draw and is formed here.  The blocks' partials are
// workspace of the draws' chunk; the results are 32 bytes a draw.
// what bl_predictive_check and bl_predictive_density serve
static bool serves_occu(const bl_dataset *d) { return d->nsp == 1 && (d->model == 0 || d->model == 2 || re_kind_in(d, {0, 2})); }
static const char *const SERVES_OCCU = "occu, with or without false positives / random effects: the handles of bl_predict without occu_rn";
extern "C" int bl_predictive_check(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, const uint8_t *obs, double *by_site,
                                   double *by_revisit)
{
    int rc = per_draw_front("bl_predictive_check", ds, n_draws, draws, obs && (by_site || by_revisit), serves_occu, SERVES_OCCU);
    if (rc || (rc = upload_once(&ds->d_wraw, ds->h_wraw))) return rc;
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, J = ds->dims.n_replicates, TJ = T * J;
    std::vector<int> obs_visit((size_t)TJ, 0);
    for (int j = 0; j < J; j++)
        for (int t = 0; t < T; t++) {
            const uint8_t *row = obs + ((size_t)j * T + t) * N;
            int c = 0;
            for (int i = 0; i < N; i++) {
                if (row[i] > 1 && row[i] != 255) return bl_fail(BL_ERR_INVALID, "bl_predictive_check: obs holds %d (0, 1, or 255 = not observed)", (int)row[i]);
                c += row[i] == 1;
            }
            obs_visit[(size_t)t * J + j] = c;
        }
    BlPredCheckParams p{};
    p.rows = ds->d_rows; p.wraw = ds->d_wraw; p.ns = ds->n_stride; p.N = N; p.T = T; p.J = J; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = ds->D;
    p.seed = (unsigned long long)seed; p.c = draw_coords(ds);
    p.n_blocks = (N + BL_PC_THREADS - 1) / BL_PC_THREADS;
    DevScratch scratch;
    unsigned char *d_obs = nullptr;
    int *d_obs_visit = nullptr;
    BL_HIP(scratch.alloc((void **)&d_obs, (size_t)TJ * N));
    BL_HIP(hipMemcpy(d_obs, obs, (size_t)TJ * N, hipMemcpyHostToDevice));
    BL_HIP(scratch.alloc((void **)&d_obs_visit, (size_t)TJ * 4));
    BL_HIP(hipMemcpy(d_obs_visit, obs_visit.data(), (size_t)TJ * 4, hipMemcpyHostToDevice));
    p.obs = d_obs; p.obs_visit = d_obs_visit;
    const size_t nb = (size_t)p.n_blocks;
    const DrawOut outs[] = {{by_site, 32, (void **)&p.by_site, false},
                            {by_revisit, 32, (void **)&p.by_revisit, false},
                            {nullptr, by_site ? nb * 32 : 0, (void **)&p.site_part, true},
                            {nullptr, by_revisit ? nb * TJ * 8 : 0, (void **)&p.visit_exp, true},
                            {nullptr, by_revisit ? nb * TJ * 4 : 0, (void **)&p.visit_rep, true}};
    return run_over_draws(ds, n_draws, draws, std::max<size_t>(32, nb * std::max(32, TJ * 8)), outs, p, bl_launch_predictive_check);
}

// ---- the same check for the abundance and count models: occu_rn, nmixture, occu_cop ----
// (BUILDER-DEFINED: the reference's check is occu's.)  Kernels: predictive_check_counts.hip.  They regenerate bl_predict's (occu_rn) /
// bl_predict_counts' (nmixture, occu_cop) replicate and bl_deterministic's sites, so they read what those read: the head of the handle's
// rows, the raw observation covariates and occu_cop's raw durations.  The observed counts come from the caller; their total per revisit
// does not depend on the draw and is formed here.  The blocks' partials are workspace of the draws' chunk; the results are 32 bytes a draw.
extern "C" int bl_predictive_check_counts(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, const int32_t *obs,
                                          double *by_site, double *by_revisit)
{
    int rc = per_draw_front("bl_predictive_check_counts", ds, n_draws, draws, obs && (by_site || by_revisit),
                            [](const bl_dataset *d) {
                                return d->nsp == 1 && (d->model == 1 || d->model == 3 || d->model == 4 || re_kind_in(d, {3, 4, 5, 6, 7}));
                            },
                            "occu_rn, nmixture and occu_cop, with or without a false-positive rate / random effects; occu uses bl_predictive_check");
    if (rc || (rc = upload_once(&ds->d_wraw, ds->h_wraw))) return rc;
    const int model = branch_model(ds);
    if (model == 3 && (rc = upload_once(&ds->d_dur, ds->h_dur))) return rc; // occu_cop's session durations
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, J = ds->dims.n_replicates, TJ = T * J;
    std::vector<double> obs_visit((size_t)TJ, 0.0);
    for (int j = 0; j < J; j++)
        for (int t = 0; t < T; t++) {
            const int32_t *row = obs + ((size_t)j * T + t) * N;
            int64_t c = 0;
            for (int i = 0; i < N; i++) {
                if (row[i] < -1) return bl_fail(BL_ERR_INVALID, "bl_predictive_check_counts: obs holds %d (a count, or -1 = not observed)", (int)row[i]);
                if (row[i] > 1 && model == 1)
                    return bl_fail(BL_ERR_INVALID, "bl_predictive_check_counts: obs holds %d (occu_rn: 0, 1, or -1 = not observed)", (int)row[i]);
                c += row[i] > 0 ? row[i] : 0;
            }
            obs_visit[(size_t)t * J + j] = (double)c;
        }
    BlPredCheckCountsParams p{};
    p.rows = ds->d_rows; p.wraw = ds->d_wraw; p.dur = ds->d_dur; p.ns = ds->n_stride; p.N = N; p.T = T; p.J = J; p.Ks = ds->Ks; p.Ko = ds->Ko;
    p.D = ds->D; p.model = model; p.K = ds->max_abundance; p.seed = (unsigned long long)seed; p.c = draw_coords(ds);
    p.n_blocks = (N + BL_PCC_THREADS - 1) / BL_PCC_THREADS;
    DevScratch scratch;
    int *d_obs = nullptr;
    double *d_obs_visit = nullptr;
    BL_HIP(scratch.alloc((void **)&d_obs, (size_t)TJ * N * 4));
    BL_HIP(hipMemcpy(d_obs, obs, (size_t)TJ * N * 4, hipMemcpyHostToDevice));
    BL_HIP(scratch.alloc((void **)&d_obs_visit, (size_t)TJ * 8));
    BL_HIP(hipMemcpy(d_obs_visit, obs_visit.data(), (size_t)TJ * 8, hipMemcpyHostToDevice));
    p.obs = d_obs; p.obs_visit = d_obs_visit;
    const size_t nb = (size_t)p.n_blocks;
    const DrawOut outs[] = {{by_site, 32, (void **)&p.by_site, false},
                            {by_revisit, 32, (void **)&p.by_revisit, false},
                            {nullptr, by_site ? nb * 32 : 0, (void **)&p.site_part, true},
                            {nullptr, by_revisit ? nb * TJ * 8 : 0, (void **)&p.visit_exp, true},
                            {nullptr, by_revisit ? nb * TJ * 8 : 0, (void **)&p.visit_rep, true}};
    return run_over_draws(ds, n_draws, draws, std::max<size_t>(32, nb * std::max(32, TJ * 8)), outs, p, bl_launch_predictive_check_counts);
}

// ---- the information criteria's two reductions of the pointwise log-likelihood, fused ----
// (biolith/evaluation/log_likelihood.py:10-96 under lppd.py, waic.py and deviance.py.)  Kernels: predictive_density.hip.  They read what
// bl_predictive_check reads and the caller's observation bytes, in which 255 now carries every mask.  The per-draw sums go through the
// draws in chunks whose block partials stay within 256 MB; the per-point statistics are one launch over all the draws (its strip
// partials do not grow with them), so no chunking can split them: it goes out with the first chunk, when all the draws are up.
extern "C" int bl_predictive_density(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, const uint8_t *obs, int marginal,
                                     double *per_draw, double *point_lse, double *point_var)
{
    int rc = per_draw_front("bl_predictive_density", ds, n_draws, draws, obs && (per_draw || point_lse || point_var), serves_occu,
                            SERVES_OCCU);
    if (rc || (rc = upload_once(&ds->d_wraw, ds->h_wraw))) return rc;
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, J = ds->dims.n_replicates;
    const size_t cells = (size_t)T * J * N;
    for (size_t c = 0; c < cells; c++)
        if (obs[c] > 1 && obs[c] != 255)
            return bl_fail(BL_ERR_INVALID, "bl_predictive_density: obs holds %d (0, 1, or 255 = not a point)", (int)obs[c]);
    BlPredDensityParams p{};
    p.rows = ds->d_rows; p.wraw = ds->d_wraw; p.ns = ds->n_stride; p.N = N; p.T = T; p.J = J; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = ds->D;
    p.seed = (unsigned long long)seed;
    p.marginal = marginal ? 1 : 0;
    p.n_draws = n_draws; p.c = draw_coords(ds);
    p.n_blocks = (N + BL_PD_THREADS - 1) / BL_PD_THREADS;
    DevScratch scratch;
    unsigned char *d_obs = nullptr;
    BL_HIP(scratch.alloc((void **)&d_obs, cells));
    BL_HIP(hipMemcpy(d_obs, obs, cells, hipMemcpyHostToDevice));
    p.obs = d_obs;
    const bool points = point_lse || point_var;
    if (points) {
        // strips of draws on grid.y: as many as let cells * strips fill the device, whatever the draw count
        p.strips = (int)std::min<size_t>(BL_PD_MAX_STRIPS, std::max<size_t>(1, (BL_PD_FILL + cells - 1) / cells));
        BL_HIP(scratch.alloc((void **)&p.strip_part, (size_t)p.strips * 4 * cells * 8));
        if (point_lse) BL_HIP(scratch.alloc((void **)&p.point_lse, cells * 8));
        if (point_var) BL_HIP(scratch.alloc((void **)&p.point_var, cells * 8));
    }
    const size_t part = per_draw ? (size_t)p.n_blocks * 8 : 0; // (no per-draw sums: one chunk, for the points' launch)
    const DrawOut outs[] = {{per_draw, 8, (void **)&p.per_draw, false}, {nullptr, part, (void **)&p.draw_part, true}};
    rc = run_over_draws(ds, n_draws, draws, part, outs, [&](const float *d_draws, int n0, int n1, int grid_y) {
        p.draws = d_draws; p.n0 = n0; p.n1 = n1;
        int e = per_draw ? bl_launch_predictive_density_draws(&p, grid_y, nullptr) : 0;
        if (!e && points && n0 == 0) {
            e = bl_launch_predictive_density_points(&p, nullptr);
            if (!e) e = (int)hipStreamSynchronize(nullptr); // it reads all the draws: done before run_over_draws lets go of them
        }
        return (hipError_t)e;
    });
    if (rc) return rc;
    if (point_lse) BL_HIP(hipMemcpy(point_lse, p.point_lse, cells * 8, hipMemcpyDeviceToHost));
    if (point_var) BL_HIP(hipMemcpy(point_var, p.point_var, cells * 8, hipMemcpyDeviceToHost));
    return BL_OK;
}

// ---- PSIS-LOO of a (draws, cells) log-likelihood matrix ----
// (No counterpart in the reference.)  Kernels: psis_loo.hip.  The entry knows no model and takes no handle: the matrix is what any
// conditional posterior returned.  Cells go up in ranges -- a strided copy each -- whose workspace (the range as uploaded, its transpose
// and three doubles per cell) stays within 256 MB; a cell's outputs do not depend on the range it travels in.
extern "C" int bl_psis_loo(int device, int n_draws, int64_t cells, const float *log_lik, int64_t cells_per_launch, double *elpd,
                           double *pareto_k, double *lppd)
{
    if (!log_lik) return bl_fail(BL_ERR_INVALID, "bl_psis_loo: log_lik is NULL");
    if (!elpd && !pareto_k && !lppd) return bl_fail(BL_ERR_INVALID, "bl_psis_loo: every output is NULL");
    if (n_draws < 2) return bl_fail(BL_ERR_INVALID, "bl_psis_loo: n_draws=%d (at least 2 draws)", n_draws);
    if (cells < 0 || cells_per_launch < 0 || device < 0)
        return bl_fail(BL_ERR_INVALID, "bl_psis_loo: cells=%lld, cells_per_launch=%lld, device=%d", (long long)cells,
                       (long long)cells_per_launch, device);
    if (n_draws > BL_PSIS_MAX_DRAWS)
        return bl_fail(BL_ERR_UNSUPPORTED, "bl_psis_loo: n_draws=%d above BL_PSIS_MAX_DRAWS=%d", n_draws, BL_PSIS_MAX_DRAWS);
    if (cells == 0) return BL_OK;
    BlPsisParams p{};
    p.n = n_draws;
    p.tail = (int)std::ceil(std::min(n_draws / 5.0, 3.0 * std::sqrt((double)n_draws)));
    if (p.tail > BL_PSIS_TAIL_MAX) return bl_fail(BL_ERR_UNSUPPORTED, "bl_psis_loo: tail of %d draws above %d", p.tail, BL_PSIS_TAIL_MAX);
    const size_t per_cell = (size_t)n_draws * 8 + 24;
    int64_t chunk = std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / per_cell));
    if (cells_per_launch > 0) chunk = std::min(chunk, cells_per_launch);
    chunk = std::min(chunk, cells);
    BL_HIP(hipSetDevice(device));
    DevScratch scratch;
    float *d_in = nullptr;
    BL_HIP(scratch.alloc((void **)&d_in, (size_t)chunk * n_draws * 4));
    BL_HIP(scratch.alloc((void **)&p.cols, (size_t)chunk * n_draws * 4));
    BL_HIP(scratch.alloc((void **)&p.out, (size_t)chunk * 3 * 8));
    p.in = d_in;
    double *const outs[3] = {elpd, pareto_k, lppd};
    for (int64_t c0 = 0; c0 < cells; c0 += chunk) {
        const int64_t cc = std::min(chunk, cells - c0);
        p.cells = (int)cc;
        if (cc == cells) // (one range: the matrix as it lies)
            BL_HIP(hipMemcpy(d_in, log_lik, (size_t)cells * n_draws * 4, hipMemcpyHostToDevice));
        else
            BL_HIP(hipMemcpy2D(d_in, (size_t)cc * 4, log_lik + c0, (size_t)cells * 4, (size_t)cc * 4, (size_t)n_draws, hipMemcpyHostToDevice));
        BL_HIP((hipError_t)bl_launch_psis_loo(&p, nullptr));
        for (int o = 0; o < 3; o++)
            if (outs[o]) BL_HIP(hipMemcpy(outs[o] + c0, p.out + (size_t)o * cc, (size_t)cc * 8, hipMemcpyDeviceToHost));
    }
    return BL_OK;
}

// ---- predictive counts of the count models (occu_cop, nmixture) ----
extern "C" int bl_predict_counts(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, int32_t *latent, int32_t *y)
{
    int rc = per_draw_front("bl_predict_counts", ds, n_draws, draws, latent || y,
                            [](const bl_dataset *d) { return d->model == 3 || d->model == 4 || re_kind_in(d, {3, 6, 7}); },
                            "the count models occu_cop and nmixture; use bl_predict");
    if (rc || (rc = upload_once(&ds->d_wraw, ds->h_wraw))) return rc;
    if (branch_model(ds) == 3 && (rc = upload_once(&ds->d_dur, ds->h_dur))) return rc; // occu_cop's session durations
    BlPredictParams p = predict_params(ds, seed);
    const size_t cells = (size_t)p.T * p.N * 4; // per draw
    const DrawOut outs[] = {{latent, cells, (void **)&p.count_latent, false}, {y, cells * p.J, (void **)&p.count_y, false}};
    return run_over_draws(ds, n_draws, draws, cells * (y ? (size_t)p.J : 1), outs, p, bl_launch_predict_counts);
}

extern "C" int bl_rng_streams(uint64_t seed, int chain, int nstreams, uint32_t *out)
{
    if (!out || chain < 0 || nstreams < 0) return bl_fail(BL_ERR_INVALID, "bl_rng_streams: bad argument");
    rng_streams(seed, chain, nstreams, out);
    return BL_OK;
}

extern "C" int bl_adaptation_schedule(int num_warmup, int32_t *starts, int32_t *ends, int capacity)
{
    if (!starts || !ends || capacity <= 0) return -1;
    return adaptation_schedule(num_warmup, starts, ends, capacity);
}

struct ModelOpts {
    int model = 0, max_abundance = 0, fp_mode = 0;
    double fp_a = 2.0, fp_b = 5.0;           // model 2: Beta(a, b); model 3: Exponential(rate = fp_a)
    const float *session_duration = nullptr; // model 3: [N][T][J]
    bool vector_kernels = false;             // the rows feed re_kernel.hpp (random effects): no 64-lane limit on species x coefficients
};
static int dataset_create_impl(const ModelOpts &mo, const bl_dims *dims, const float *site_covs, const float *obs_covs,
                               const float *obs, const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha,
                               int device, bl_dataset **out);

extern "C" int bl_dataset_create(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                 const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device,
                                 bl_dataset **out)
{
    return dataset_create_impl(ModelOpts{}, dims, site_covs, obs_covs, obs, prior_beta, prior_alpha, device, out);
}

extern "C" int bl_dataset_create_rn(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                    int max_abundance, const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha,
                                    int device, bl_dataset **out)
{
    if (max_abundance < 1 || max_abundance >= BL_RN_NB)
        return bl_fail(BL_ERR_UNSUPPORTED, "max_abundance=%d outside 1..%d", max_abundance, BL_RN_NB - 1);
    ModelOpts mo; mo.model = 1; mo.max_abundance = max_abundance;
    return dataset_create_impl(mo, dims, site_covs, obs_covs, obs, prior_beta, prior_alpha, device, out);
}

extern "C" int bl_dataset_create_dyn(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                     const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    if (dims && dims->n_site_covs > BL_DYN_MAX_KS)
        return bl_fail(BL_ERR_UNSUPPORTED, "dynamic occupancy: at most %d site covariates (three coefficient blocks), got %d", BL_DYN_MAX_KS, dims->n_site_covs);
    ModelOpts mo; mo.model = 8; // (6 names the random-effects / occu_cs handles)
    return dataset_create_impl(mo, dims, site_covs, obs_covs, obs, prior_beta, prior_alpha, device, out);
}

extern "C" int bl_dataset_create_fp(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                    int fp_mode, const bl_beta_prior *prior_fp, const bl_normal_prior *prior_beta,
                                    const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    if (fp_mode != BL_FP_CONSTANT && fp_mode != BL_FP_UNOCCUPIED)
        return bl_fail(BL_ERR_INVALID, "fp_mode must be BL_FP_CONSTANT or BL_FP_UNOCCUPIED");
    ModelOpts mo; mo.model = 2; mo.fp_mode = fp_mode;
    if (prior_fp) { mo.fp_a = prior_fp->a; mo.fp_b = prior_fp->b; }
    if (!(mo.fp_a > 0.0) || !(mo.fp_b > 0.0) || !std::isfinite(mo.fp_a) || !std::isfinite(mo.fp_b))
        return bl_fail(BL_ERR_INVALID, "Beta prior needs finite a, b > 0");
    return dataset_create_impl(mo, dims, site_covs, obs_covs, obs, prior_beta, prior_alpha, device, out);
}

extern "C" int bl_dataset_create_nmix(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                      int max_abundance, const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha,
                                      int device, bl_dataset **out)
{
    if (max_abundance < 1 || max_abundance >= BL_RN_NB)
        return bl_fail(BL_ERR_UNSUPPORTED, "max_abundance=%d outside 1..%d", max_abundance, BL_RN_NB - 1);
    ModelOpts mo; mo.model = 4; mo.max_abundance = max_abundance;
    return dataset_create_impl(mo, dims, site_covs, obs_covs, obs, prior_beta, prior_alpha, device, out);
}

extern "C" int bl_dataset_create_cop(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                     const float *session_duration, int fp_mode, double prior_fp_rate,
                                     const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device,
                                     bl_dataset **out)
{
    if (fp_mode != 0 && fp_mode != BL_FP_CONSTANT && fp_mode != BL_FP_UNOCCUPIED)
        return bl_fail(BL_ERR_INVALID, "fp_mode must be 0, BL_FP_CONSTANT or BL_FP_UNOCCUPIED");
    if (!session_duration) return bl_fail(BL_ERR_INVALID, "session_duration is NULL");
    ModelOpts mo; mo.model = 3; mo.fp_mode = fp_mode; mo.session_duration = session_duration;
    mo.fp_a = fp_mode ? prior_fp_rate : 1.0;
    if (!(mo.fp_a > 0.0) || !std::isfinite(mo.fp_a)) return bl_fail(BL_ERR_INVALID, "Exponential prior needs a finite rate > 0");
    return dataset_create_impl(mo, dims, site_covs, obs_covs, obs, prior_beta, prior_alpha, device, out);
}

static int dataset_create_impl(const ModelOpts &mo, const bl_dims *dims, const float *site_covs, const float *obs_covs,
                               const float *obs, const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha,
                               int device, bl_dataset **out)
{
    const int model = mo.model, max_abundance = mo.max_abundance;
    if (!dims || !out) return bl_fail(BL_ERR_INVALID, "dims/out is NULL");
    bl_env_snapshot();
    *out = nullptr;
    const int S = dims->n_species, N = dims->n_sites, T = dims->n_periods, J = dims->n_replicates;
    const int Ks = dims->n_site_covs, Ko = dims->n_obs_covs;
    // shape checks mirror the asserts at biolith/models/occu.py:103-133
    if (N <= 0 || T <= 0 || J <= 0 || Ks < 0 || Ko < 0) return bl_fail(BL_ERR_INVALID, "non-positive dimension");
    // Several species in ONE handle = one chain over all species' coefficients (the species plate of occu.py:182-186 under one
    // NUTS, with a false-positive rate shared across species, occu.py:146-157): the LDS-staged occu / false-positive forms only.
    if (S < 1) return bl_fail(BL_ERR_INVALID, "n_species=%d", S);
    if (model == 8 && S != 1) return bl_fail(BL_ERR_UNSUPPORTED, "dynamic occupancy: one species per dataset");
    if (S > 1 && model != 0 && model != 2)
        return bl_fail(BL_ERR_UNSUPPORTED, "n_species=%d: joint sampling of several species is built for occu with or without false positives; "
                       "this model takes one species per dataset", S);
    if (Ks > BL_MAX_COVS || Ko > BL_MAX_COVS)
        return bl_fail(BL_ERR_UNSUPPORTED, "more than %d covariates per side (Ks=%d, Ko=%d)", BL_MAX_COVS, Ks, Ko);
    if ((Ks > 0 && !site_covs) || (Ko > 0 && !obs_covs) || !obs) return bl_fail(BL_ERR_INVALID, "NULL data pointer");
    const bl_normal_prior pb = prior_beta ? *prior_beta : bl_normal_prior{0.0, 1.0};
    const bl_normal_prior pa = prior_alpha ? *prior_alpha : bl_normal_prior{0.0, 1.0};
    if (!(pb.scale > 0.0) || !(pa.scale > 0.0) || !std::isfinite(pb.loc) || !std::isfinite(pa.loc))
        return bl_fail(BL_ERR_INVALID, "Normal prior needs finite loc and scale > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return bl_fail(BL_ERR_NO_DEVICE, "no HIP device visible: the occupancy engine has no CPU fallback");
    if (device < 0 || device >= ndev) return bl_fail(BL_ERR_INVALID, "device %d out of range (%d visible)", device, ndev);

    bl_dataset *ds = new bl_dataset();
    const int has_extra = (model == 2 || (model == 3 && mo.fp_mode != 0)) ? 1 : 0; // trailing false-positive coordinate
    ds->device = device; ds->dims = *dims; ds->Ks = Ks; ds->Ko = Ko; ds->D = S * (Ks + Ko + 2) + has_extra;
    if (model == 8) ds->D = 3 * (Ks + 1) + Ko + 1; // dynamic occupancy: [b_psi | b_gamma | b_eps | alpha]
    ds->nsp = S;
    ds->model = model; ds->max_abundance = max_abundance;
    ds->fp_mode = mo.fp_mode; ds->fp_a = mo.fp_a; ds->fp_b = mo.fp_b;
    ds->KS = pad_covs(Ks); ds->KO = pad_covs(Ko);
    ds->kern = find_kernels(ds->KS, ds->KO);
    ds->pb = pb; ds->pa = pa;
    if (!ds->kern) { delete ds; return bl_fail(BL_ERR_UNSUPPORTED, "no kernel for capacity (%d,%d)", pad_covs(Ks), pad_covs(Ko)); }
    const int V = T * J, KS = ds->KS, KO = ds->KO;
    if (S > 1 && !mo.vector_kernels && (S * BL_SP_COEF(KS, KO) + 2 > 64 || S * BL_SP_PART(KS, KO) * BL_CWAVES_MAX > BL_PART_FLOATS || ds->D + 4 > 64)) {
        delete ds;
        return bl_fail(BL_ERR_UNSUPPORTED, "n_species=%d x (Ks=%d, Ko=%d): too many coordinates for one joint chain (sample the species one by one)", S, Ks, Ko);
    }
    // floats per visit: (c, c w_1 .. c w_KO), or (y, dur | m, w..) for the count models; occu_rn keeps one more, zero here, that its
    // kernel rewrites at every evaluation (rn_device.hpp)
    const int vw = KO + 1 + ((model == 1 || model == 3 || model == 4) ? 1 : 0);
    ds->ko_layout = vw - 1;
    const int n_stride = (N + 63) / 64 * 64;
    const int sp_rows = V * vw + 2 * T;          // rows of one species' block (visits, ka, kb); the site covariates come once
    const int n_rows = KS + S * sp_rows;
    ds->n_stride = n_stride; ds->n_rows = n_rows;

    // ---- pack: mask (occu.py:136-142, modeling.py:15-17), NaN->0, sign folding, site-fastest rows ----
    std::vector<float> rows((size_t)n_rows * n_stride, 0.0f);
    ds->h_wraw.assign((size_t)V * (Ko > 0 ? Ko : 1) * n_stride, 0.0f);
    if (model == 3) ds->h_dur.assign((size_t)V * n_stride, 0.0f);
    if (model == 3) ds->h_ccell.assign((size_t)T * n_stride, 0.0f);
    const double LN2 = 0.69314718055994530942, LOG_TINY = -87.33654475055310898657;
    const int row_wc = KS, row_ka = KS + V * vw, row_kb = row_ka + T;
    double cop_const = 0.0; // occu_cop: sum over unmasked visits of y log(dur) - lgamma(y + 1)
    // nmixture: B[t][n][site] = sum over unmasked visits of log C(n, y), -inf for n below the largest count
    // (nmixture.py:150-155, 186-190 and numpyro's BinomialProbs.log_prob); one spare row for pair reads
    const int Kn = max_abundance;
    std::vector<float> tab(model == 4 ? ((size_t)T * (Kn + 1) + 1) * n_stride : 0, 0.0f);
    for (int i = 0; i < N; i++) {
        bool site_nan = false;
        for (int k = 0; k < Ks; k++) {
            float x = site_covs[(size_t)i * Ks + k];
            if (std::isnan(x)) { site_nan = true; x = 0.0f; }
            rows[(size_t)k * n_stride + i] = x;
        }
        for (int t = 0; t < T && model == 4; t++) {
            std::vector<double> ys;
            for (int j = 0; j < J; j++) {
                const int v = t * J + j;
                const size_t o = ((size_t)i * T + t) * J + j;
                bool cov_nan = site_nan;
                const size_t r0 = (size_t)(row_wc + v * vw);
                for (int k = 0; k < Ko; k++) {
                    float x = obs_covs[o * Ko + k];
                    if (std::isnan(x)) { cov_nan = true; x = 0.0f; }
                    ds->h_wraw[((size_t)v * Ko + k) * n_stride + i] = x;
                    rows[(r0 + 2 + k) * n_stride + i] = x;
                }
                const float y = obs[o];
                if (cov_nan || !std::isfinite(y)) {
                    for (int k = 0; k < Ko; k++) rows[(r0 + 2 + k) * n_stride + i] = 0.0f;
                    continue;
                }
                rows[r0 * n_stride + i] = y;          // m y
                rows[(r0 + 1) * n_stride + i] = 1.0f; // m
                ys.push_back((double)y);
            }
            double ymax = 0.0;
            for (double y : ys) ymax = std::max(ymax, y);
            for (int n = 0; n <= Kn; n++) {
                double b = 0.0;
                if ((double)n < ymax) b = -INFINITY;
                else for (double y : ys) b += std::lgamma(n + 1.0) - std::lgamma(y + 1.0) - std::lgamma(n - y + 1.0);
                tab[((size_t)t * (Kn + 1) + n) * n_stride + i] = (float)b;
            }
            rows[(size_t)(row_ka + t) * n_stride + i] = (float)ymax;
            rows[(size_t)(row_kb + t) * n_stride + i] = (float)ys.size();
        }
        for (int t = 0; t < T && model == 3; t++) {
            // occu_cop.py:150-156,236-255: visit = (y_m, d_m, w_1..w_Ko), masked visits contribute nothing
            double ysum = 0.0, dsum = 0.0, ccell = 0.0;
            for (int j = 0; j < J; j++) {
                const int v = t * J + j;
                const size_t o = ((size_t)i * T + t) * J + j;
                bool cov_nan = site_nan;
                const size_t r0 = (size_t)(row_wc + v * vw);
                for (int k = 0; k < Ko; k++) {
                    float x = obs_covs[o * Ko + k];
                    if (std::isnan(x)) { cov_nan = true; x = 0.0f; }
                    ds->h_wraw[((size_t)v * Ko + k) * n_stride + i] = x;
                    rows[(r0 + 2 + k) * n_stride + i] = x;
                }
                const float y = obs[o], dur = mo.session_duration[o];
                ds->h_dur[(size_t)v * n_stride + i] = dur;
                if (cov_nan || !std::isfinite(y)) {
                    for (int k = 0; k < Ko; k++) rows[(r0 + 2 + k) * n_stride + i] = 0.0f;
                    continue;
                }
                rows[r0 * n_stride + i] = y;
                rows[(r0 + 1) * n_stride + i] = dur;
                ysum += y; dsum += dur;
                const double c = (y > 0.0f ? (double)y * std::log((double)dur) : 0.0) - std::lgamma((double)y + 1.0);
                cop_const += c; ccell += c;
            }
            ds->h_ccell[(size_t)t * n_stride + i] = (float)ccell;
            rows[(size_t)(row_ka + t) * n_stride + i] = (float)ysum;
            rows[(size_t)(row_kb + t) * n_stride + i] = (float)dsum;
        }
        for (int sp = 0; sp < S && model != 3 && model != 4; sp++)
        for (int t = 0; t < T; t++) {
            const size_t sp_off = (size_t)sp * sp_rows;     // this species' block of rows
            const float *obs_sp = obs + (size_t)sp * N * T * J;
            int n_masked = 0, n_det = 0;
            for (int j = 0; j < J; j++) {
                const int v = t * J + j;
                const size_t o = ((size_t)i * T + t) * J + j;
                bool cov_nan = site_nan;
                float w[BL_MAX_COVS];
                for (int k = 0; k < Ko; k++) {
                    float x = obs_covs[o * Ko + k];
                    if (std::isnan(x)) { cov_nan = true; x = 0.0f; }
                    w[k] = x;
                    ds->h_wraw[((size_t)v * Ko + k) * n_stride + i] = x;
                }
                const float y = obs_sp[o];
                float c = 0.0f;
                if (cov_nan || !std::isfinite(y)) n_masked++;
                else if (y != 0.0f) { c = 1.0f; n_det++; }
                else c = -1.0f;
                const size_t r0 = sp_off + (size_t)(row_wc + v * vw);
                rows[r0 * n_stride + i] = c;
                for (int k = 0; k < Ko; k++) rows[(r0 + 1 + k) * n_stride + i] = c * w[k];
            }
            rows[(sp_off + (size_t)(row_ka + t)) * n_stride + i] = (float)(n_masked * LN2);
            rows[(sp_off + (size_t)(row_kb + t)) * n_stride + i] = (float)(n_det * LOG_TINY);
        }
    }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&ds->d_rows, rows.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(ds->d_rows, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && model == 4) e = hipMalloc((void **)&ds->d_tab, tab.size() * sizeof(float));
    if (e == hipSuccess && model == 4) e = hipMemcpy(ds->d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ds->h_abort, 64, hipHostMallocMapped);
    if (e == hipSuccess) { *ds->h_abort = 0; e = hipHostGetDevicePointer((void **)&ds->d_abort, ds->h_abort, 0); }
    if (e == hipSuccess) e = hipEventCreate(&ds->ev0);
    if (e == hipSuccess) e = hipEventCreate(&ds->ev1);
    if (e != hipSuccess) {
        const int rc = bl_fail(BL_ERR_NO_DEVICE, "dataset upload failed: %s", hipGetErrorString(e));
        bl_dataset_destroy(ds);
        return rc;
    }
    BlDevData &dd = ds->dd;
    dd.rows = ds->d_rows; dd.n_sites = N; dd.n_stride = n_stride; dd.T = T; dd.J = J;
    dd.Ks = Ks; dd.Ko = Ko; dd.KS = KS; dd.KO = KO;
    dd.loc_b = (float)pb.loc; dd.isc2_b = (float)(1.0 / (pb.scale * pb.scale));
    dd.loc_a = (float)pa.loc; dd.isc2_a = (float)(1.0 / (pa.scale * pa.scale));
    dd.prior_const = S * ((Ks + 1) * std::log(pb.scale) + (Ko + 1) * std::log(pa.scale) + (Ks + Ko + 2) * 0.91893853320467274178);
    dd.n_species = S;
    dd.dyn = model == 8 ? 1 : 0;
    if (model == 8) dd.prior_const = 3 * (Ks + 1) * std::log(pb.scale) + (Ko + 1) * std::log(pa.scale) + ds->D * 0.91893853320467274178;
    dd.has_fp = has_extra ? model : 0; dd.fp_a = (float)mo.fp_a; dd.fp_b = (float)mo.fp_b;
    if (model == 3) {
        dd.prior_const -= cop_const;                        // the parameter-free part of the Poisson log-pmf
        if (has_extra) dd.prior_const -= std::log(mo.fp_a); // phi = log f, f ~ Exponential(r): energy r e^phi - phi - log r
    }
    if (model == 2) // phi = logit f, f ~ Beta(a, b): the energy a softplus(-phi) + b softplus(phi) carries + log B(a, b)
        dd.prior_const += std::lgamma(mo.fp_a) + std::lgamma(mo.fp_b) - std::lgamma(mo.fp_a + mo.fp_b);
    *out = ds;
    return BL_OK;
}

extern "C" int bl_dataset_set_prior_family(bl_dataset *ds, int family_beta, int family_alpha)
{
    if (!ds) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if ((family_beta != BL_PRIOR_NORMAL && family_beta != BL_PRIOR_LAPLACE) || (family_alpha != BL_PRIOR_NORMAL && family_alpha != BL_PRIOR_LAPLACE))
        return bl_fail(BL_ERR_INVALID, "prior family must be BL_PRIOR_NORMAL or BL_PRIOR_LAPLACE");
    if (ds->in_flight) return bl_fail(BL_ERR_BUSY, "a NUTS launch is in flight on this handle");
    BlDevData &dd = ds->dd;
    // constant of the potential: log(scale) + log(2 pi) / 2 per Normal coefficient, log(2 scale) per Laplace one
    const double HL2PI = 0.91893853320467274178;
    auto konst = [&](int fam, double scale) { return fam == BL_PRIOR_LAPLACE ? std::log(2.0 * scale) : std::log(scale) + HL2PI; };
    const double before = ds->nsp * ((ds->Ks + 1) * konst(ds->fam_b, ds->pb.scale) + (ds->Ko + 1) * konst(ds->fam_a, ds->pa.scale));
    const double after = ds->nsp * ((ds->Ks + 1) * konst(family_beta, ds->pb.scale) + (ds->Ko + 1) * konst(family_alpha, ds->pa.scale));
    dd.prior_const += after - before;
    ds->fam_b = family_beta; ds->fam_a = family_alpha;
    dd.isc2_b = family_beta == BL_PRIOR_LAPLACE ? 0.0f : (float)(1.0 / (ds->pb.scale * ds->pb.scale));
    dd.l1_b = family_beta == BL_PRIOR_LAPLACE ? (float)(1.0 / ds->pb.scale) : 0.0f;
    dd.isc2_a = family_alpha == BL_PRIOR_LAPLACE ? 0.0f : (float)(1.0 / (ds->pa.scale * ds->pa.scale));
    dd.l1_a = family_alpha == BL_PRIOR_LAPLACE ? (float)(1.0 / ds->pa.scale) : 0.0f;
    if (ds->model == 6) {
        BlReModel &m = ds->re;
        m.u_const += after - before;
        m.isc2_b = dd.isc2_b; m.l1_b = dd.l1_b; m.isc2_a = dd.isc2_a; m.l1_a = dd.l1_a;
    }
    return BL_OK;
}

extern "C" int bl_dataset_destroy(bl_dataset *ds)
{
    if (!ds) return BL_OK;
    hipSetDevice(ds->device);
    if (ds->in_flight) { *ds->h_abort = 1; hipStreamSynchronize(ds->stream); }
    if (ds->d_rows) hipFree(ds->d_rows);
    if (ds->d_wraw) hipFree(ds->d_wraw);
    if (ds->d_araw) hipFree(ds->d_araw);
    if (ds->d_tab) hipFree(ds->d_tab);
    if (ds->d_dur) hipFree(ds->d_dur);
    if (ds->d_ccell) hipFree(ds->d_ccell);
    if (ds->d_run) hipFree(ds->d_run);
    if (ds->d_xchg) hipFree(ds->d_xchg);
    if (ds->d_restate) hipFree(ds->d_restate);
    if (ds->d_scores) hipFree(ds->d_scores);
    if (ds->h_abort) hipHostFree(ds->h_abort);
    if (ds->ev0) hipEventDestroy(ds->ev0);
    if (ds->ev1) hipEventDestroy(ds->ev1);
    delete ds;
    return BL_OK;
}

extern "C" int bl_dataset_param_dim(const bl_dataset *ds, int *D)
{
    if (!ds || !D) return bl_fail(BL_ERR_INVALID, "NULL argument");
    *D = ds->D;
    return BL_OK;
}

// Workgroups per chain / LDS staging decision.  One site per thread is the latency optimum
// (DESIGN.md "geometry"); fall back to several sites per thread, then to un-staged HBM rows.
// Dynamic occupancy: lanes that share one site pair (dyn_device.hpp) -- as many (a power of two, <= 8, <= the seasons) as the lanes of
// the workgroups one XCD offers a chain allow at one pair per lane group.
static int dyn_lanes_per_pair(const bl_dataset *ds, int chains)
{
    const int per_xcd = ((chains > 0 ? chains : 1) + 7) / 8;
    const int kmax = std::max(1, 32 / per_xcd);
    const long long npairs = (ds->dims.n_sites + 1) / 2;
    int G = 1;
    while (2 * G <= 8 && 2 * G <= ds->dims.n_periods) G *= 2;
    while (G > 1 && npairs * G > (long long)kmax * 4 * 64) G >>= 1; // (round 4: up to four compute waves per workgroup)
    if (const char *e = bl_env(BL_ENV_DYN_G)) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8) G = v; } // A/B knob
    return G;
}

// Plain occupancy model and its false-positive form: lanes that share one site pair (occu_device.hpp: bl_eval_sites_grp), as the code
// log2(period lanes) | log2(visit lanes) << 4; 0 = one pair per lane.  More lanes per pair while a lane would still walk more than
// BL_GRP_VISITS visits of its pair and the lanes one XCD offers the chain (4 compute waves on each of its <= kmax workgroups) allow it;
// the periods are split first (nothing to exchange between those lanes), then the visits of a period (one DPP fold per period).
#define BL_GRP_VISITS 6
#ifndef BL_WIDE_KMAX
#define BL_WIDE_KMAX 128   // workgroups of a chain in the wide geometry when lane groups ask for more than the slice needs (measured: tools/time_wide.py)
#endif
static int occu_lane_group(const bl_dataset *ds, int chains, int want_k, int kcap = 0)
{
    if (ds->model != 0 && ds->model != 2 && ds->model != 3 && ds->model != 4) return 0; // (occu, false positives, occu_cop, nmixture)
    const int T = ds->dims.n_periods, J = ds->dims.n_replicates;
    const long long V = (long long)T * J, npairs = (ds->dims.n_sites + 1) / 2;
    const int per_xcd = ((chains > 0 ? chains : 1) + 7) / 8;
    int kmax = std::max(1, 32 / per_xcd);
    if (kcap > 0) kmax = kcap; // (wide geometry: the chain's workgroups span XCDs -- the lanes of up to 256 / chains workgroups)
    if (want_k > 0) kmax = std::min(kmax, want_k);
    int target = BL_GRP_VISITS;
    if (const char *e = bl_env(BL_ENV_GRP_VISITS)) { const int v = atoi(e); if (v >= 1) target = v; } // A/B knob
    int lg = 0;
    while (lg < 4 && ((V + (1 << lg) - 1) >> lg) > target && (npairs << (lg + 1)) <= (long long)kmax * 4 * 64) lg++;
    if (const char *e = bl_env(BL_ENV_OCCU_G)) { // tests / A/B: force the lanes per pair (1, 2, 4, 8, 16)
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) { lg = 0; while ((1 << lg) < v) lg++; }
    }
    int lgt = 0;
    while (lgt < lg && (2 << lgt) <= T) lgt++;
    if (const char *e = bl_env(BL_ENV_OCCU_GT)) { const int v = atoi(e); if (v >= 0 && v <= lg) lgt = v; } // tests: log2 of the period lanes
    int lgj = lg - lgt;
    while (lgj > 0 && (1 << (lgj - 1)) >= J) lgj--; // (visit lanes beyond a period's visits would only idle)
    return lgt | (lgj << 4);
}

// Small problems (plain model and false positives): the whole chain on ONE workgroup of BL_CWAVES_SINGLE compute waves -- no exchange
// through L2 at all (nuts_kernel.hpp: the k == 1 path), the site pairs shared among as many lanes as the 448 offer.  Taken when a lane
// is then left with at most BL_SINGLE_VISITS visits of its pair (400 x 16, 8 visits per lane: 2.00 us on one workgroup against 1.86 on five) and the records fit one CU's LDS.  Returns the lane-group code or -1.
#define BL_SINGLE_VISITS 7
static int occu_single_workgroup(const bl_dataset *ds, int want_k)
{
    if ((ds->model != 0 && ds->model != 2) || want_k > 0 || ds->nsp > 1) return -1; // (several species: the partial table is sized for 4 waves)
    if (const char *e = bl_env(BL_ENV_SINGLE)) { if (e[0] == '0') return -1; } // A/B knob
    const int T = ds->dims.n_periods, J = ds->dims.n_replicates;
    const long long V = (long long)T * J, npairs = (ds->dims.n_sites + 1) / 2, lanes = BL_CWAVES_SINGLE * 64;
    if (npairs > lanes) return -1;
    int lg = 0;
    while (lg < 4 && (npairs << (lg + 1)) <= lanes && ((V + (1 << lg) - 1) >> lg) > 1) lg++;
    if (((V + (1 << lg) - 1) >> lg) > BL_SINGLE_VISITS) return -1;
    if (const char *e = bl_env(BL_ENV_OCCU_G)) { // tests / A/B: force the lanes per pair
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) { lg = 0; while ((1 << lg) < v) lg++; }
    }
    int lgt = 0;
    while (lgt < lg && (2 << lgt) <= T) lgt++;
    if (const char *e = bl_env(BL_ENV_OCCU_GT)) { const int v = atoi(e); if (v >= 0 && v <= lg) lgt = v; }
    int lgj = lg - lgt;
    while (lgj > 0 && (1 << (lgj - 1)) >= J) lgj--;
    return lgt | (lgj << 4);
}

static void choose_geometry(const bl_dataset *ds, int chains, int want_k, int *k_out, int *nloc_out, int *ld_out,
                            int *lds_bytes_out, int *staged_out, int *ncw_out, int *wide_out, int *grp_out = nullptr)
{
    const int N = ds->dims.n_sites;
    // chains are dealt to the 8 XCDs (32 CUs each); a chain's k workgroups share one XCD, one per CU
    const int per_xcd = ((chains > 0 ? chains : 1) + 7) / 8;
    int kmax = 32 / per_xcd;
    if (kmax < 1) kmax = 1;
    // occu / false positives: a lane evaluates a PAIR of sites (packed f32 math); one pair per lane is the
    // latency optimum.  With 3 compute waves every wave, the control wave included, owns a SIMD; that is
    // used whenever one pair per lane still fits the chain's workgroup budget, else 4 compute waves.
    // occu_rn (rn_device.hpp): 7 compute waves; its cost is per item of the sums over N, not per lane, so a chain takes
    // all the workgroups its XCD offers once it has more than a wave of sites for each.
    int ncw = BL_CWAVES_RN, per_wg = 64, grp = 0;
    if (ds->model != 1) {
        grp = occu_lane_group(ds, chains, want_k);
        const int G = 1 << ((grp & 15) + (grp >> 4)); // lanes per site pair
        ncw = (((long long)N * G + 2 * 3 * 64 - 1) / (2 * 3 * 64) <= kmax) ? 3 : 4;
        // A/B knob: only the counts this library was built with (3, 4, and BL_OCCU_CWX in a variant build of the plain model); anything
        // else is ignored rather than turned into a launch that no instantiation serves
        if (const char *e = bl_env(BL_ENV_CWAVES)) {
            const int v = atoi(e);
            bool built = v == 3 || v == 4;
#ifdef BL_OCCU_CWX
            built = built || (ds->model == 0 && v == BL_OCCU_CWX);
#endif
            if (built) ncw = v;
        }
        per_wg = std::max(2, 2 * ncw * 64 / G);
        if (ds->model == 8) { // one site pair per lane group; three compute waves while the chain's workgroups offer the lanes, else four
            const int Gd = dyn_lanes_per_pair(ds, chains);
            ncw = (((long long)N * Gd + 2 * 3 * 64 - 1) / (2 * 3 * 64) <= kmax) ? 3 : 4;
            if (const char *e = bl_env(BL_ENV_CWAVES)) { const int v = atoi(e); if (v == 3 || v == 4) ncw = v; }
            per_wg = std::max(2, 2 * ncw * 64 / Gd);
        }
    }
    int k = want_k > 0 ? want_k : (N + per_wg - 1) / per_wg;
    if (k > kmax) k = kmax;
    if (k < 1) k = 1;
    const int single_grp = occu_single_workgroup(ds, want_k);
    if (single_grp >= 0 && (long long)((N + 1) / 2) * bl_record_stride(ds->dims.n_periods, ds->dims.n_replicates, ds->KS, ds->ko_layout) * 4 * ds->nsp
                               <= BL_LDS_TOTAL - BL_OFF_DATA) {
        k = 1; ncw = BL_CWAVES_SINGLE; grp = single_grp; // one workgroup per chain: no exchange
    }
    // behind the records: occu_rn's tables; the dynamic model's lane-private columns (sized for 4 compute waves: ncw is settled below)
    const int rn_scratch = ds->model == 1 ? bl_rn_scratch_bytes(BL_CWAVES_RN) : (ds->model == 8 ? bl_dyn_scratch_bytes(ds->dims.n_periods, 4) : 0);
    const int lds_cap = BL_LDS_TOTAL - BL_OFF_DATA - rn_scratch;
    // LDS keeps one record of `stride` floats per PAIR of sites (occu_device.hpp)
    const int stride = bl_record_stride(ds->dims.n_periods, ds->dims.n_replicates, ds->KS, ds->ko_layout);
    auto fits = [&](int kk, int *nloc) { // (every species has a record region of its own)
        *nloc = (N + kk - 1) / kk;
        return (long long)((*nloc + 1) / 2) * stride * 4 * ds->nsp <= lds_cap;
    };
    int nloc;
    bool ok = fits(k, &nloc);
    // (an explicit count that does not fit is raised too for the models that have no HBM-row form -- fit()'s retry at k/2 after an engine
    // timeout must not turn into a refusal -- but kept for the plain model, whose HBM-row form serves any count)
    if (!ok && (want_k <= 0 || ds->model != 0))
        for (int kk = k + 1; kk <= kmax && !ok; kk++) { ok = fits(kk, &nloc); if (ok) k = kk; }
    // Wide geometry: the slice does not fit the LDS of one XCD's workgroups, but it does when the chain takes more
    // CUs than one XCD has.  The exchange then crosses XCDs (the kernel's placement census makes it take the fabric
    // form), which costs a few thousand cycles per tick -- little next to re-reading the rows from HBM every tick.
    int wide = 0;
    if (!ok && want_k <= 0) {
        const char *e = bl_env(BL_ENV_NO_WIDE);
        const int kwide = 256 / (chains > 0 ? chains : 1);
        if (!(e && e[0] == '1'))
            for (int kk = kmax + 1; kk <= kwide && !ok; kk++) { ok = fits(kk, &nloc); if (ok) { k = kk; wide = 1; } }
    }
    if (ok && !wide && ds->model == 1 && want_k <= 0) { // A/B knob: occu_rn over more workgroups than one XCD offers a chain
        if (const char *e = bl_env(BL_ENV_RN_K)) {
            const int kk = atoi(e), kwide = 256 / (chains > 0 ? chains : 1);
            int nl;
            if (kk > kmax && kk <= kwide && fits(kk, &nl)) { k = kk; nloc = nl; wide = 1; }
        }
    }
    if (ds->model == 0 && want_k <= 0) { // A/B knob: the plain model over kk workgroups across XCDs although one XCD's would do
        if (const char *e = bl_env(BL_ENV_WIDE_K)) {
            const int kk = atoi(e), kwide = 256 / (chains > 0 ? chains : 1);
            int nl;
            if (kk > 0 && kk <= kwide && fits(kk, &nl)) { k = kk; nloc = nl; wide = 1; ok = true; }
        }
    }
    // Wide geometry and many visits per site (the top rows of the reference's benchmark grid: 6 400 x 64, 12 800 x 90): the lanes of
    // one XCD no longer cap the lane groups -- a site pair is shared by as many lanes as BL_GRP_VISITS asks for and the chain takes
    // the workgroups that offer them (four compute waves each), up to 256 / chains.  More workgroups make the exchange longer (every
    // workgroup gathers every record over the fabric); BL_WIDE_KMAX bounds them where that costs more than the shorter visit loops save.
    if (wide && ok && (ds->model == 0 || ds->model == 2) && want_k <= 0 && !bl_env(BL_ENV_WIDE_K)) {
        const int kwide = std::min(256 / (chains > 0 ? chains : 1), BL_WIDE_KMAX);
        if (kwide > k) {
            const int g2 = occu_lane_group(ds, chains, 0, kwide);
            const int G2 = 1 << ((g2 & 15) + (g2 >> 4));
            int kk = (int)((((long long)N + 1) / 2 * G2 + 4 * 64 - 1) / (4 * 64));
            kk = std::min(std::max(kk, k), kwide);
            int nl;
            if (fits(kk, &nl)) { k = kk; nloc = nl; grp = g2; }
        }
    } else if (wide && ok && (ds->model == 0 || ds->model == 2) && want_k <= 0) {
        grp = occu_lane_group(ds, chains, 0, k); // (forced k: the groups its lanes allow)
    }
    if (!ok) fits(k, &nloc);
    if (!ok && ds->model == 0) ncw = 4; // HBM-row form is built for 4 compute waves only
    if (wide) ncw = ds->model == 1 ? BL_CWAVES_RN : 4; // full slices: all four SIMDs evaluate
    if (!ok) grp = 0; // (the HBM-row form keeps one pair per lane)
    if (grp_out) *grp_out = grp;
    *k_out = k; *nloc_out = nloc; *ld_out = stride; *staged_out = ok ? 1 : 0; *ncw_out = ncw; *wide_out = wide;
    *lds_bytes_out = ok ? BL_OFF_DATA + ((nloc + 1) / 2) * stride * 4 * ds->nsp + rn_scratch : BL_OFF_DATA;
}

// nmixture: the columns of the table B[t][n][site] that belong to a workgroup's sites go to LDS behind the records when they fit
// (T (K + 1) rows of 2 ceil(nloc / 2) floats); returns 1 and grows *lds_bytes if so.  BIOLITH_HIP_NMIX_LDS=0 keeps them in HBM / L2 (A/B).
static int nmix_table_in_lds(const bl_dataset *ds, int staged, int nloc, int *lds_bytes)
{
    if (ds->model != 4 || !staged) return 0;
    if (const char *e = bl_env(BL_ENV_NMIX_LDS)) { if (e[0] == '0') return 0; }
    const long long tb = (long long)ds->dims.n_periods * (ds->max_abundance + 1) * (2 * ((nloc + 1) / 2)) * 4;
    if (*lds_bytes + tb > BL_LDS_TOTAL) return 0;
    *lds_bytes += (int)tb;
    return 1;
}

// ------------------------------------------------------------- K1 logp ----
__global__ void bl_logp_final_kernel(BlDevData dd, int k, const double *theta, const double *partial, double *U, double *grad)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Dsp = dd.Ks + dd.Ko + 2, nsp = dd.n_species > 0 ? dd.n_species : 1;
    const int D = dd.dyn ? 3 * (dd.Ks + 1) + dd.Ko + 1 : nsp * Dsp + (dd.has_fp ? 1 : 0);
    const int lj = lane < nsp * Dsp ? lane % Dsp : lane; // index within the lane's species
    double acc = 0.0;
    if (lane <= D)
        for (int m = 0; m < k; m++) acc += partial[((size_t)b * k + m) * 64 + lane];
    double pr = 0.0;
    if (lane < D && dd.has_fp == 3 && lane == D - 1) {
        // phi = log f, f ~ Exponential(rate r), Jacobian included: r e^phi - phi  (log r is in prior_const)
        const double phi = theta[(size_t)b * D + lane], rf = dd.fp_a * exp(phi);
        pr = rf - phi;
        grad[(size_t)b * D + lane] = -acc + rf - 1.0;
    } else if (lane < D && dd.has_fp && lane == D - 1) {
        // phi = logit f, f ~ Beta(a, b), Jacobian included: a softplus(-phi) + b softplus(phi)
        const double phi = theta[(size_t)b * D + lane], l = log1p(exp(-fabs(phi)));
        const double sig = 1.0 / (1.0 + exp(-phi));
        pr = dd.fp_a * (fmax(-phi, 0.0) + l) + dd.fp_b * (fmax(phi, 0.0) + l);
        grad[(size_t)b * D + lane] = -acc + (dd.fp_a + dd.fp_b) * sig - dd.fp_a;
    } else if (lane < D) {
        const bool is_b = dd.dyn ? lane < 3 * (dd.Ks + 1) : lj <= dd.Ks;
        const double loc = is_b ? dd.loc_b : dd.loc_a, isc2 = is_b ? dd.isc2_b : dd.isc2_a, l1 = is_b ? dd.l1_b : dd.l1_a;
        const double dth = theta[(size_t)b * D + lane] - loc;
        pr = 0.5 * dth * dth * isc2 + fabs(dth) * l1; // Normal or Laplace (one of isc2, l1 is 0)
        grad[(size_t)b * D + lane] = -acc + dth * isc2 + ((dth > 0.0) - (dth < 0.0)) * l1;
    }
    const double prior = bl_wave_sum_d(pr);
    if (lane == D) U[b] = -acc + prior + dd.prior_const;
}

// Launch of the random-effects / occu_cs NUTS kernel instantiated for this run's capacity, model kind and LDS residency.
template <int MK, int KIND, bool LROWS, int LT>
static hipError_t re_nuts_launch_inst(const BlReRun &run, int grid, size_t lds, hipStream_t st)
{
    if (lds) {
        const hipError_t e = hipFuncSetAttribute((const void *)bl_re_nuts_kernel<MK, KIND, LROWS, LT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((bl_re_nuts_kernel<MK, KIND, LROWS, LT>), dim3(grid), dim3(BL_RE_NT), lds, st, run);
    snprintf(g_kernel_name, sizeof g_kernel_name, "bl_re_nuts_kernel<%d, %d, %s, %d, 0>", MK, KIND, LROWS ? "true" : "false", LT); // (as rocprofv3 prints it)
    return hipGetLastError();
}
// the bench form's instantiations with the model's effects as compile-time facts (re_kernel.hpp: EFF)
template <int EFF>
static hipError_t re_nuts_launch_eff(const BlReRun &run, int grid, size_t lds, hipStream_t st)
{
    if (lds) {
        const hipError_t e = hipFuncSetAttribute((const void *)bl_re_nuts_kernel<4, 0, true, 2, EFF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((bl_re_nuts_kernel<4, 0, true, 2, EFF>), dim3(grid), dim3(BL_RE_NT), lds, st, run);
    snprintf(g_kernel_name, sizeof g_kernel_name, "bl_re_nuts_kernel<4, 0, true, 2, %d>", EFF);
    return hipGetLastError();
}
template <int MK, int KIND>
static hipError_t re_nuts_dispatch_lds(const BlReRun &run, int grid, size_t lds, hipStream_t st)
{
    const int lt = run.m.lds_hot;
    if constexpr (MK == 4 && KIND == 0) {
        const char *e = bl_env(BL_ENV_RE_EFF); // A/B knob: 0 = the general kernel
        if (run.m.lds_rows && lt == 2 && run.m.n_species == 1 && !(e && e[0] == '0')) {
            // one period as a fact too, for site effects alone (same trajectories, one box: 8.91 -> 8.85 us on the bench shape; with
            // observation effects the same fact measured 0.1-2 % slower on four shapes -- profiles/r04/i_ab_re_t1_all.txt -- and is not
            // instantiated); knob 1: without it
            const int eff = (run.m.site_re ? 1 : 0) | (run.m.obs_re ? 2 : 0);
            if (eff == 1) return run.m.T == 1 && !(e && e[0] == '1') ? re_nuts_launch_eff<5>(run, grid, lds, st) : re_nuts_launch_eff<1>(run, grid, lds, st);
            if (eff == 2) return re_nuts_launch_eff<2>(run, grid, lds, st);
            if (eff == 3) return re_nuts_launch_eff<3>(run, grid, lds, st);
        }
    }
    if (run.m.lds_rows)
        return lt == 2 ? re_nuts_launch_inst<MK, KIND, true, 2>(run, grid, lds, st)
                       : (lt == 1 ? re_nuts_launch_inst<MK, KIND, true, 1>(run, grid, lds, st) : re_nuts_launch_inst<MK, KIND, true, 0>(run, grid, lds, st));
    return lt == 2 ? re_nuts_launch_inst<MK, KIND, false, 2>(run, grid, lds, st)
                   : (lt == 1 ? re_nuts_launch_inst<MK, KIND, false, 1>(run, grid, lds, st) : re_nuts_launch_inst<MK, KIND, false, 0>(run, grid, lds, st));
}
static hipError_t re_nuts_dispatch(int mk, const BlReRun &run, int grid, size_t lds, hipStream_t st)
{
    if (run.m.kind == 8) return mk == 4 ? re_nuts_dispatch_lds<4, 8>(run, grid, lds, st) : re_nuts_dispatch_lds<16, 8>(run, grid, lds, st);
    if (run.m.kind == 2) return mk == 4 ? re_nuts_dispatch_lds<4, 2>(run, grid, lds, st) : re_nuts_dispatch_lds<16, 2>(run, grid, lds, st);
    if (run.m.kind == 3) return mk == 4 ? re_nuts_dispatch_lds<4, 3>(run, grid, lds, st) : re_nuts_dispatch_lds<16, 3>(run, grid, lds, st);
    if (run.m.kind == 4) return mk == 4 ? re_nuts_dispatch_lds<4, 4>(run, grid, lds, st) : re_nuts_dispatch_lds<16, 4>(run, grid, lds, st);
    if (run.m.kind == 5) return mk == 4 ? re_nuts_dispatch_lds<4, 5>(run, grid, lds, st) : re_nuts_dispatch_lds<16, 5>(run, grid, lds, st);
    if (run.m.kind == 6) return mk == 4 ? re_nuts_dispatch_lds<4, 6>(run, grid, lds, st) : re_nuts_dispatch_lds<16, 6>(run, grid, lds, st);
    if (run.m.kind == 7) return mk == 4 ? re_nuts_dispatch_lds<4, 7>(run, grid, lds, st) : re_nuts_dispatch_lds<16, 7>(run, grid, lds, st);
    if (mk == 4) return run.m.kind == 1 ? re_nuts_dispatch_lds<4, 1>(run, grid, lds, st) : re_nuts_dispatch_lds<4, 0>(run, grid, lds, st);
    return run.m.kind == 1 ? re_nuts_dispatch_lds<16, 1>(run, grid, lds, st) : re_nuts_dispatch_lds<16, 0>(run, grid, lds, st);
}

// Geometry of the random-effects kernels for slices of `nloc` sites: threads sharing a site's visits, what lives in LDS.
// with_hot: also the sampler's hot (or hot and warm) vectors (NUTS only).  Returns the dynamic LDS bytes.
static size_t re_geometry(BlReModel &m, int nloc, int with_hot, int dl_max)
{
    int tps = 1;
    while (tps < 64 && 2 * tps * nloc <= BL_RE_NT && 2 * tps <= m.J) tps *= 2; // spare threads share a site's visits
    m.tps = tps;
    // two classes of waves (re_kernel.hpp: BlReSiteMap): more than four waves' worth of sites in one round -> the first four waves
    // full, the remaining sites on the other four waves with as many threads per site as fit
    m.w_a = BL_RE_NW; m.n_a = nloc; m.tps_b = tps;
    {
        const int lanes = nloc * tps, half = BL_RE_NT / 2;
        if (lanes > half && lanes <= BL_RE_NT) {
            const int n_a = half / tps, rest = nloc - n_a;
            int tb = tps;
            while (tb < 64 && 2 * tb * rest <= half && 2 * tb <= m.J) tb *= 2;
            const char *e = bl_env(BL_ENV_RE_NO_SPLIT); // (measurement)
            if (tb > tps && !(e && e[0] == '1')) { m.w_a = BL_RE_NW / 2; m.n_a = n_a; m.tps_b = tb; }
        }
    }
    // a workgroup's own LDS copy of its rows, and of the five vectors every leapfrog touches, when they fit (160 KB per CU,
    // one workgroup per CU; a few KB go to the reduction scratch)
    // (160 KB per workgroup; the kernels' static arrays -- reduction scratch, the exchange's [32][NRED] staging, per-species sums -- take up
    // to 10.3 KB at capacity 16)
    const size_t row_bytes = (size_t)m.n_rows * nloc * 4, budget = (size_t)148 * 1024;
    const size_t hot_bytes = (size_t)RE_HOT * dl_max * 4, warm_bytes = (size_t)RE_WARM * dl_max * 4;
    m.lds_rows = row_bytes <= budget ? 1 : 0;
    if (const char *e = bl_env(BL_ENV_RE_LDS_ROWS)) m.lds_rows = std::min(m.lds_rows, atoi(e)); // (tests: every instantiation)
    const size_t used = m.lds_rows ? row_bytes : 0;
    m.lds_hot = !with_hot ? 0 : (used + warm_bytes <= budget ? 2 : (used + hot_bytes <= budget ? 1 : 0));
    if (const char *e = bl_env(BL_ENV_RE_LDS_TIER)) m.lds_hot = std::min(m.lds_hot, atoi(e)); // (measurement)
    return used + (m.lds_hot == 2 ? warm_bytes : (m.lds_hot == 1 ? hot_bytes : 0));
}

static int create_re_impl(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                          int site_random_effects, int obs_random_effects, double prior_site_re_sd_scale,
                          double prior_obs_re_sd_scale, int fp_mode, double fp_a, double fp_b, int count_model, int count_K, const bl_normal_prior *prior_beta,
                          const bl_normal_prior *prior_alpha, int device, bl_dataset **out, const float *session_duration = nullptr);

// occu_cop(site_random_effects / obs_random_effects = True [, false_positives_constant / _unoccupied = True]): occu_cop.py:158-170,
// 183-186, 204-210, 229-248.  theta = [beta, alpha, (phi = log rate_fp), (log sds), site_re_occ [N], site_re_det [N], obs_re [N][T][J]];
// `counts` / `session_duration` / fp_mode / prior_fp_rate as bl_dataset_create_cop; one species.
extern "C" int bl_dataset_create_cop_re(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *counts,
                                        const float *session_duration, int fp_mode, double prior_fp_rate, int site_random_effects,
                                        int obs_random_effects, double prior_site_re_sd_scale, double prior_obs_re_sd_scale,
                                        const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    if (fp_mode != 0 && fp_mode != BL_FP_CONSTANT && fp_mode != BL_FP_UNOCCUPIED)
        return bl_fail(BL_ERR_INVALID, "fp_mode must be 0, BL_FP_CONSTANT or BL_FP_UNOCCUPIED");
    if (fp_mode && (!(prior_fp_rate > 0.0) || !std::isfinite(prior_fp_rate))) return bl_fail(BL_ERR_INVALID, "Exponential prior needs a finite rate > 0");
    if (!session_duration) return bl_fail(BL_ERR_INVALID, "session_duration is NULL");
    if (dims && dims->n_species != 1)
        return bl_fail(BL_ERR_UNSUPPORTED, "occu_cop with random effects: one species per dataset (n_species=%d)", dims->n_species);
    return create_re_impl(dims, site_covs, obs_covs, counts, site_random_effects, obs_random_effects, prior_site_re_sd_scale,
                          prior_obs_re_sd_scale, fp_mode, fp_mode ? prior_fp_rate : 1.0, 0.0, 3, 0, prior_beta, prior_alpha, device, out, session_duration);
}

extern "C" int bl_dataset_create_re(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                    int site_random_effects, int obs_random_effects, double prior_site_re_sd_scale,
                                    double prior_obs_re_sd_scale, const bl_normal_prior *prior_beta,
                                    const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    return create_re_impl(dims, site_covs, obs_covs, obs, site_random_effects, obs_random_effects, prior_site_re_sd_scale,
                          prior_obs_re_sd_scale, 0, 0.0, 0.0, 0, 0, prior_beta, prior_alpha, device, out);
}

// occu_rn(false_positives_constant = True [, site_random_effects / obs_random_effects = True]): occu_rn.py:133-138, 214-221 --
// y ~ Bernoulli(1 - (1 - p)(1 - f)), f ~ Beta(a, b).  theta = [beta, alpha, phi = logit f, (log sds), (effects)]; one species.  The
// model runs on the random-effects kernels also WITHOUT effects (kind 5; the work-proportional kernel of the plain model has no such term).
extern "C" int bl_dataset_create_rn_fp(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                       int max_abundance, int site_random_effects, int obs_random_effects,
                                       double prior_site_re_sd_scale, double prior_obs_re_sd_scale, const bl_beta_prior *prior_fp,
                                       const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    if (max_abundance < 1 || max_abundance >= BL_RN_NB)
        return bl_fail(BL_ERR_UNSUPPORTED, "max_abundance=%d outside 1..%d", max_abundance, BL_RN_NB - 1);
    if (dims && dims->n_species != 1)
        return bl_fail(BL_ERR_UNSUPPORTED, "Royle-Nichols with a false-positive rate: one species per dataset (n_species=%d)", dims->n_species);
    const double a = prior_fp ? prior_fp->a : 2.0, b = prior_fp ? prior_fp->b : 5.0;
    if (!(a > 0.0) || !(b > 0.0) || !std::isfinite(a) || !std::isfinite(b)) return bl_fail(BL_ERR_INVALID, "Beta prior needs finite a, b > 0");
    return create_re_impl(dims, site_covs, obs_covs, obs, site_random_effects, obs_random_effects,
                          site_random_effects ? prior_site_re_sd_scale : 1.0, obs_random_effects ? prior_obs_re_sd_scale : 1.0,
                          BL_FP_CONSTANT, a, b, 1, max_abundance, prior_beta, prior_alpha, device, out);
}

// occu(site_random_effects / obs_random_effects = True, false_positives_constant / _unoccupied = True): occu.py:146-157 with
// :170-173, 191-196.  theta = [beta, alpha, phi = logit(rate), (log sds), (effects)]; one species.
extern "C" int bl_dataset_create_re_fp(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                       int site_random_effects, int obs_random_effects, double prior_site_re_sd_scale,
                                       double prior_obs_re_sd_scale, int fp_mode, const bl_beta_prior *prior_fp,
                                       const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    if (fp_mode != BL_FP_CONSTANT && fp_mode != BL_FP_UNOCCUPIED)
        return bl_fail(BL_ERR_INVALID, "fp_mode must be BL_FP_CONSTANT or BL_FP_UNOCCUPIED");
    const double a = prior_fp ? prior_fp->a : 2.0, b = prior_fp ? prior_fp->b : 5.0;
    if (!(a > 0.0) || !(b > 0.0) || !std::isfinite(a) || !std::isfinite(b)) return bl_fail(BL_ERR_INVALID, "Beta prior needs finite a, b > 0");
    if (dims && dims->n_species != 1)
        return bl_fail(BL_ERR_UNSUPPORTED, "random effects with a false-positive rate: one species per dataset (n_species=%d)", dims->n_species);
    return create_re_impl(dims, site_covs, obs_covs, obs, site_random_effects, obs_random_effects, prior_site_re_sd_scale,
                          prior_obs_re_sd_scale, fp_mode, a, b, 0, 0, prior_beta, prior_alpha, device, out);
}

// nmixture(site_random_effects / obs_random_effects = True): nmixture.py:139-141, 166-172, 199-214.  theta = [beta, alpha, (log sds),
// site_re_abu [N], site_re_det [N], obs_re [N][T][J]]; `counts` as bl_dataset_create_nmix; one species.
extern "C" int bl_dataset_create_nmix_re(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *counts,
                                         int max_abundance, int site_random_effects, int obs_random_effects,
                                         double prior_site_re_sd_scale, double prior_obs_re_sd_scale, const bl_normal_prior *prior_beta,
                                         const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    if (max_abundance < 1 || max_abundance >= BL_RN_NB)
        return bl_fail(BL_ERR_UNSUPPORTED, "max_abundance=%d outside 1..%d", max_abundance, BL_RN_NB - 1);
    if (dims && dims->n_species != 1)
        return bl_fail(BL_ERR_UNSUPPORTED, "N-mixture with random effects: one species per dataset (n_species=%d)", dims->n_species);
    return create_re_impl(dims, site_covs, obs_covs, counts, site_random_effects, obs_random_effects, prior_site_re_sd_scale,
                          prior_obs_re_sd_scale, 0, 0.0, 0.0, 4, max_abundance, prior_beta, prior_alpha, device, out);
}

// occu_rn(site_random_effects / obs_random_effects = True): occu_rn.py:151-154, 172-184, 199-212.  theta = [beta, alpha, (log sds),
// site_re_abu [N], site_re_det [N], obs_re [N][T][J]]; one species.
extern "C" int bl_dataset_create_rn_re(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                                       int max_abundance, int site_random_effects, int obs_random_effects,
                                       double prior_site_re_sd_scale, double prior_obs_re_sd_scale, const bl_normal_prior *prior_beta,
                                       const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    if (max_abundance < 1 || max_abundance >= BL_RN_NB)
        return bl_fail(BL_ERR_UNSUPPORTED, "max_abundance=%d outside 1..%d", max_abundance, BL_RN_NB - 1);
    if (dims && dims->n_species != 1)
        return bl_fail(BL_ERR_UNSUPPORTED, "Royle-Nichols with random effects: one species per dataset (n_species=%d)", dims->n_species);
    return create_re_impl(dims, site_covs, obs_covs, obs, site_random_effects, obs_random_effects, prior_site_re_sd_scale,
                          prior_obs_re_sd_scale, 0, 0.0, 0.0, 1, max_abundance, prior_beta, prior_alpha, device, out);
}

static int create_re_impl(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                          int site_random_effects, int obs_random_effects, double prior_site_re_sd_scale,
                          double prior_obs_re_sd_scale, int fp_mode, double fp_a, double fp_b, int count_model, int count_K, const bl_normal_prior *prior_beta,
                          const bl_normal_prior *prior_alpha, int device, bl_dataset **out, const float *session_duration /* occu_cop only */)
{
    bl_env_snapshot();
    if (!site_random_effects && !obs_random_effects && !(count_model == 1 && fp_mode))
        return bl_fail(BL_ERR_INVALID, "bl_dataset_create_re: neither random effect requested (use bl_dataset_create)");
    if (dims && (dims->n_site_covs > BL_RE_MAXK || dims->n_obs_covs > BL_RE_MAXK))
        return bl_fail(BL_ERR_UNSUPPORTED, "random-effects kernels are built for at most %d covariates per side (Ks=%d, Ko=%d)",
                       BL_RE_MAXK, dims->n_site_covs, dims->n_obs_covs);
    if ((site_random_effects && !(prior_site_re_sd_scale > 0.0)) || (obs_random_effects && !(prior_obs_re_sd_scale > 0.0)))
        return bl_fail(BL_ERR_INVALID, "HalfNormal prior needs scale > 0");
    if (dims && dims->n_species > BL_RE_SMAX)
        return bl_fail(BL_ERR_UNSUPPORTED, "random effects: at most %d species under one chain (n_species=%d)", BL_RE_SMAX, dims->n_species);
    // the rows of the plain model (mask, NaN -> 0, sign folding; one block of visit rows per species) are exactly what the
    // random-effects site pass reads
    // (N-mixture: the count model's rows -- visit = (m y, m, w..) -- and its table of log-binomial sums)
    ModelOpts mo; mo.vector_kernels = true;
    if (count_model) { mo.model = count_model; mo.max_abundance = count_K; } // 4: N-mixture, 1: Royle-Nichols, 3: occu_cop (no false positives)
    if (count_model == 3) { mo.fp_mode = fp_mode; mo.fp_a = fp_mode ? fp_a : 1.0; mo.session_duration = session_duration; } // (fp_a: the Exponential prior's rate)
    int rc = dataset_create_impl(mo, dims, site_covs, obs_covs, obs, prior_beta, prior_alpha, device, out);
    if (rc) return rc;
    bl_dataset *ds = *out;
    const int S = dims->n_species, N = dims->n_sites, T = dims->n_periods, J = dims->n_replicates, Ks = ds->Ks, Ko = ds->Ko;
    // draws: [species 0: beta, alpha | species 1: ... | log site_re_sd | log obs_re_sd | site_re_occ [S][N] | site_re_det [S][N] | obs_re [S][N][T][J]]
    const long long Dll = (long long)S * (Ks + Ko + 2) + (fp_mode ? 1 : 0) + (site_random_effects ? 1 + 2LL * S * N : 0) + (obs_random_effects ? 1 + (long long)S * N * T * J : 0);
    if (Dll > (1LL << 24)) { bl_dataset_destroy(ds); *out = nullptr; return bl_fail(BL_ERR_UNSUPPORTED, "%lld coordinates", Dll); }
    BlReModel &m = ds->re;
    m.rows = ds->dd.rows; m.n_sites = N; m.n_stride = ds->dd.n_stride; m.T = T; m.J = J; m.Ks = Ks; m.Ko = Ko; m.KS = ds->KS; m.KO = ds->KO;
    m.site_re = site_random_effects ? 1 : 0; m.obs_re = obs_random_effects ? 1 : 0;
    m.n_species = S; m.G0s = Ks + Ko + 2; m.sp = 0; m.cb = 0; m.rv0 = ds->KS; m.sp_rows = T * J * (ds->KO + 1 + (count_model ? 1 : 0)) + 2 * T;
    m.G0 = S * m.G0s; m.G = m.G0 + (fp_mode ? 1 : 0) + m.site_re + m.obs_re; m.D = (int)Dll;
    int at = m.G0;
    m.kind = count_model == 4 ? 3 : (count_model == 1 ? (fp_mode ? 5 : 4) : (count_model == 3 ? (fp_mode ? 7 : 6) : (fp_mode ? 2 : 0))); m.fp_mode = fp_mode; m.fp_a = (float)fp_a; m.fp_b = (float)fp_b;
    m.tab = ds->d_tab; m.tab_ld = ds->n_stride; m.max_abundance = count_K;
    m.o_fp = fp_mode ? at++ : -1;       // phi = logit(false-positive rate): right behind the regression coefficients
    m.o_phi_s = m.site_re ? at++ : -1;
    m.o_phi_o = m.obs_re ? at++ : -1;
    m.o_u = m.o_v = m.o_e = -1;
    if (m.site_re) { m.o_u = at; m.o_v = at + S * N; at += 2 * S * N; }
    if (m.obs_re) { m.o_e = at; at += S * N * T * J; }
    m.loc_b = ds->dd.loc_b; m.isc2_b = ds->dd.isc2_b; m.loc_a = ds->dd.loc_a; m.isc2_a = ds->dd.isc2_a;
    m.l1_b = 0.0f; m.l1_a = 0.0f;
    m.hn_is2_s = site_random_effects ? (float)(1.0 / (prior_site_re_sd_scale * prior_site_re_sd_scale)) : 0.0f;
    m.hn_is2_o = obs_random_effects ? (float)(1.0 / (prior_obs_re_sd_scale * prior_obs_re_sd_scale)) : 0.0f;
    const double HL2PI = 0.91893853320467274178, HN0 = 0.5 * std::log(2.0 / 3.14159265358979323846);
    m.u_const = ds->dd.prior_const;
    if (fp_mode && count_model != 3) m.u_const += std::lgamma(fp_a) + std::lgamma(fp_b) - std::lgamma(fp_a + fp_b); // + log B(a, b)  (occu_cop: -log rate is in prior_const)
    if (m.site_re) m.u_const += -HN0 + std::log(prior_site_re_sd_scale) + 2.0 * S * N * HL2PI;
    if (m.obs_re) m.u_const += -HN0 + std::log(prior_obs_re_sd_scale) + (double)S * N * T * J * HL2PI;
    m.n_total = N; m.s0 = 0; m.x_u = m.o_u; m.x_v = m.o_v; m.x_e = m.o_e;
    m.n_rows = ds->KS + m.sp_rows; // what ONE workgroup stages: the site covariates and its species' block
    re_geometry(m, N, 0, 0); // one workgroup over all sites (bl_logp_grad); bl_nuts_launch picks its own slices
    ds->model = 6; ds->D = m.D;
    return BL_OK;
}

// occu_cs (biolith/models/occu_cs.py): the continuous-score model runs on the random-effects kernels' framework (a chain over
// several workgroups, vectors in device memory) with four extra fixed coordinates and no effects.
extern "C" int bl_dataset_create_cs(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *scores,
                                    const double *prior_mu /*[4]: loc, scale of mu0; of mu1's base*/,
                                    const double *prior_sigma /*[4]: concentration, rate of sigma0; of sigma1*/,
                                    const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    if (!dims || !scores || !prior_mu || !prior_sigma || !out) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (dims->n_site_covs > BL_RE_MAXK || dims->n_obs_covs > BL_RE_MAXK)
        return bl_fail(BL_ERR_UNSUPPORTED, "occu_cs kernels are built for at most %d covariates per side (Ks=%d, Ko=%d)", BL_RE_MAXK,
                       dims->n_site_covs, dims->n_obs_covs);
    if (!(prior_mu[1] > 0.0) || !(prior_mu[3] > 0.0) || !(prior_sigma[0] > 0.0) || !(prior_sigma[1] > 0.0) || !(prior_sigma[2] > 0.0) || !(prior_sigma[3] > 0.0))
        return bl_fail(BL_ERR_INVALID, "occu_cs priors need positive scales / concentrations / rates");
    const size_t n = (size_t)dims->n_species * dims->n_sites * dims->n_periods * dims->n_replicates;
    // the plain model's rows with "has a score" as the observation: c = 1 for a scored replicate, 0 for a masked one
    std::vector<float> has(n);
    for (size_t i = 0; i < n; i++) has[i] = std::isfinite(scores[i]) ? 1.0f : NAN;
    int rc = dataset_create_impl(ModelOpts{}, dims, site_covs, obs_covs, has.data(), prior_beta, prior_alpha, device, out);
    if (rc) return rc;
    bl_dataset *ds = *out;
    const int N = dims->n_sites, V = dims->n_periods * dims->n_replicates, Ks = ds->Ks, Ko = ds->Ko;
    std::vector<float> sc((size_t)V * ds->n_stride, 0.0f);
    for (int i = 0; i < N; i++)
        for (int v = 0; v < V; v++) {
            const float x = scores[(size_t)i * V + v];
            sc[(size_t)v * ds->n_stride + i] = std::isfinite(x) ? x : 0.0f;
        }
    if (hipMalloc((void **)&ds->d_scores, sc.size() * 4) != hipSuccess ||
        hipMemcpy(ds->d_scores, sc.data(), sc.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        bl_dataset_destroy(ds); *out = nullptr;
        return bl_fail(BL_ERR_NO_DEVICE, "occu_cs: score upload failed");
    }
    BlReModel &m = ds->re;
    m.rows = ds->dd.rows; m.n_sites = N; m.n_stride = ds->dd.n_stride; m.T = dims->n_periods; m.J = dims->n_replicates;
    m.Ks = Ks; m.Ko = Ko; m.KS = ds->KS; m.KO = ds->KO;
    m.site_re = 0; m.obs_re = 0; m.kind = 1; m.scores = ds->d_scores;
    m.G0 = Ks + Ko + 2; m.G = m.G0 + 4; m.D = m.G;
    m.n_species = 1; m.G0s = m.G0; m.sp = 0; m.cb = 0; m.rv0 = ds->KS; m.sp_rows = V * (ds->KO + 1) + 2 * dims->n_periods;
    m.o_phi_s = m.o_phi_o = m.o_u = m.o_v = m.o_e = -1;
    m.loc_b = ds->dd.loc_b; m.isc2_b = ds->dd.isc2_b; m.loc_a = ds->dd.loc_a; m.isc2_a = ds->dd.isc2_a; m.l1_b = 0.0f; m.l1_a = 0.0f;
    m.hn_is2_s = m.hn_is2_o = 0.0f;
    for (int k = 0; k < 4; k++) { m.cs_mu[k] = (float)prior_mu[k]; m.cs_sg[k] = (float)prior_sigma[k]; }
    // constants of the potential: the coefficients' (dd.prior_const), the two Normal normalisers of mu0 / mu1, the Gammas'
    const double HL2PI = 0.91893853320467274178;
    m.u_const = ds->dd.prior_const + std::log(prior_mu[1]) + std::log(prior_mu[3]) + 2.0 * HL2PI;
    for (int f = 0; f < 2; f++) m.u_const += -prior_sigma[2 * f] * std::log(prior_sigma[2 * f + 1]) + std::lgamma(prior_sigma[2 * f]);
    m.n_total = N; m.s0 = 0; m.x_u = m.x_v = m.x_e = -1;
    m.n_rows = ds->n_rows;
    re_geometry(m, N, 0, 0);
    ds->model = 6; ds->D = m.D;
    return BL_OK;
}

// occu_comb (biolith/models/occu_comb.py:150-349): point counts, ARU detections and scores on the random-effects kernels' framework
// (kind 8), one species, no effects: D = G = (Ks + 1) + (Kpc + 1) + (Karu + 1) + 6.  The handle is made as a plain occu handle
// over the point counts (device, events, the abort flag); the kind-8 rows replace what the kernels read.
extern "C" int bl_dataset_create_comb(const bl_comb_dims *cd, const float *site_covs, const float *pc_covs, const float *pc_obs,
                                      const float *aru_covs, const float *aru_obs, const float *scores, const bl_beta_prior *prior_fc,
                                      const bl_beta_prior *prior_fu, const double *prior_mu, const double *prior_sigma,
                                      const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out)
{
    if (!cd || !pc_obs || !aru_obs || !scores || !prior_mu || !prior_sigma || !out) return bl_fail(BL_ERR_INVALID, "NULL argument");
    const int N = cd->n_sites, T = cd->n_periods, Jp = cd->n_pc, Ja = cd->n_aru, Js = cd->n_scores;
    const int Ks = cd->n_site_covs, Kp = cd->n_pc_covs, Ka = cd->n_aru_covs;
    if (N <= 0 || T <= 0 || Jp < 0 || Ja < 0 || Js < 0 || Ks < 0 || Kp < 0 || Ka < 0) return bl_fail(BL_ERR_INVALID, "negative dimension");
    if (Ks > BL_RE_MAXK || Kp > BL_RE_MAXK || Ka > BL_RE_MAXK)
        return bl_fail(BL_ERR_UNSUPPORTED, "occu_comb kernels are built for at most %d covariates per block (Ks=%d, Kpc=%d, Karu=%d)",
                       BL_RE_MAXK, Ks, Kp, Ka);
    if ((Kp > 0 && !pc_covs) || (Ka > 0 && !aru_covs) || (Ks > 0 && !site_covs)) return bl_fail(BL_ERR_INVALID, "NULL covariates");
    const double fca = prior_fc ? prior_fc->a : 2.0, fcb = prior_fc ? prior_fc->b : 5.0, fua = prior_fu ? prior_fu->a : 2.0, fub = prior_fu ? prior_fu->b : 5.0;
    if (!(fca > 0.0) || !(fcb > 0.0) || !(fua > 0.0) || !(fub > 0.0) || !std::isfinite(fca + fcb + fua + fub))
        return bl_fail(BL_ERR_INVALID, "Beta prior needs finite a, b > 0");
    if (!(prior_mu[1] > 0.0) || !(prior_mu[3] > 0.0) || !(prior_sigma[0] > 0.0) || !(prior_sigma[1] > 0.0) || !(prior_sigma[2] > 0.0) || !(prior_sigma[3] > 0.0))
        return bl_fail(BL_ERR_INVALID, "occu_comb priors need positive scales / concentrations / rates");
    // the handle: a plain occu handle over the point counts (at least one replicate: a stand-in of NaN when there are none)
    bl_dims pd{1, N, T, Jp > 0 ? Jp : 1, Ks, Kp};
    std::vector<float> nan_obs;
    const float *pobs = pc_obs, *pcov = pc_covs;
    if (Jp == 0) { nan_obs.assign((size_t)N * T, NAN); pobs = nan_obs.data(); pd.n_obs_covs = 0; pcov = nullptr; }
    int rc = dataset_create_impl(ModelOpts{}, &pd, site_covs, pcov, pobs, prior_beta, prior_alpha, device, out);
    if (rc) return rc;
    bl_dataset *ds = *out;
    // ---- rows: site covariates (+ a zero row), PC visits, ARU visits, six rows per period (bl_comb_site_pass) ----
    const int ns = ds->n_stride, vp = Kp + 1, va = Ka + 1, KSc = Ks + 1;
    const int r_pc = KSc, r_ar = r_pc + T * Jp * vp, r_per = r_ar + T * Ja * va, n_rows = r_per + 6 * T;
    std::vector<float> rows((size_t)n_rows * ns, 0.0f);
    // the ARU block's raw covariates, NaN -> 0, as dataset_create_impl keeps the point counts' (h_wraw): the rows below are folded by the
    // observation, so bl_predict_comb / bl_deterministic_comb, which withhold it, read these
    ds->h_araw.assign((size_t)std::max(T * Ja * Ka, 1) * ns, 0.0f);
    for (int i = 0; i < N; i++)
        for (int v = 0; v < T * Ja; v++)
            for (int k = 0; k < Ka; k++) {
                const float x = aru_covs[((size_t)i * T * Ja + v) * Ka + k];
                ds->h_araw[((size_t)v * Ka + k) * ns + i] = std::isnan(x) ? 0.0f : x;
            }
    const double LOG_TINY = -87.33654475055310898657;
    for (int i = 0; i < N; i++) {
        bool site_nan = false;
        for (int k = 0; k < Ks; k++) {
            float x = site_covs[(size_t)i * Ks + k];
            if (std::isnan(x)) { site_nan = true; x = 0.0f; }
            rows[(size_t)k * ns + i] = x;
        }
        for (int t = 0; t < T; t++) {
            // one block of sign-folded visits: returns (detections, non-detections)
            auto block = [&](int J, int K, int vw, int r0, const float *covs, const float *obs, int &nd, int &nn) {
                nd = nn = 0;
                for (int j = 0; j < J; j++) {
                    const size_t o = ((size_t)i * T + t) * J + j;
                    bool nan = site_nan;
                    for (int k = 0; k < K; k++) nan = nan || std::isnan(covs[o * K + k]);
                    const float y = obs[o];
                    const float c = (nan || !std::isfinite(y)) ? 0.0f : (y != 0.0f ? 1.0f : -1.0f);
                    nd += c > 0.0f; nn += c < 0.0f;
                    const size_t rr = (size_t)r0 + (size_t)(t * J + j) * vw;
                    rows[rr * ns + i] = c;
                    for (int k = 0; k < K; k++) rows[(rr + 1 + k) * ns + i] = c == 0.0f ? 0.0f : c * covs[o * K + k];
                }
            };
            int pd_, pn_, ad_, an_;
            block(Jp, Kp, vp, r_pc, pc_covs, pc_obs, pd_, pn_);
            block(Ja, Ka, va, r_ar, aru_covs, aru_obs, ad_, an_);
            // the period's scores: count, mean, sum of squared deviations (f64 on the host)
            double n = 0.0, mean = 0.0, m2 = 0.0;
            for (int j = 0; j < Js && !site_nan; j++) {
                const double x = scores[((size_t)i * T + t) * Js + j];
                if (!std::isfinite(x)) continue;
                n += 1.0;
                const double dlt = x - mean;
                mean += dlt / n;
                m2 += dlt * (x - mean);
            }
            const size_t rp = (size_t)r_per + 6 * t;
            rows[rp * ns + i] = (float)(pd_ * LOG_TINY);
            rows[(rp + 1) * ns + i] = (float)ad_; rows[(rp + 2) * ns + i] = (float)an_;
            rows[(rp + 3) * ns + i] = (float)n; rows[(rp + 4) * ns + i] = (float)mean; rows[(rp + 5) * ns + i] = (float)m2;
        }
    }
    if (hipMalloc((void **)&ds->d_scores, rows.size() * 4) != hipSuccess ||
        hipMemcpy(ds->d_scores, rows.data(), rows.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        bl_dataset_destroy(ds); *out = nullptr;
        return bl_fail(BL_ERR_NO_DEVICE, "occu_comb: row upload failed");
    }
    const bl_normal_prior pb = prior_beta ? *prior_beta : bl_normal_prior{0.0, 1.0}, pa = prior_alpha ? *prior_alpha : bl_normal_prior{0.0, 1.0};
    BlReModel &m = ds->re;
    m.rows = ds->d_scores; m.n_sites = N; m.n_stride = ns; m.T = T; m.J = std::max(std::max(Jp, Ja), 1);
    m.Ks = Ks; m.Ko = std::max(Kp, Ka); m.KS = KSc; m.KO = m.Ko;
    BlCombModel &cm = ds->comb;
    cm.Jpc = Jp; cm.Jaru = Ja; cm.Jsc = Js; cm.Kpc = Kp; cm.Karu = Ka; cm.r_aru = r_ar - r_pc; cm.r_per = r_per - r_pc;
    cm.fc_a = (float)fca; cm.fc_b = (float)fcb; cm.fu_a = (float)fua; cm.fu_b = (float)fub;
    m.site_re = 0; m.obs_re = 0; m.kind = 8; m.scores = nullptr;
    m.G0 = Ks + Kp + Ka + 3; m.G = m.G0 + 6; m.D = m.G;
    m.n_species = 1; m.G0s = m.G0; m.sp = 0; m.cb = 0; m.rv0 = KSc; m.sp_rows = n_rows - KSc;
    m.o_fp = -1; m.o_phi_s = m.o_phi_o = m.o_u = m.o_v = m.o_e = -1;
    m.loc_b = (float)pb.loc; m.isc2_b = (float)(1.0 / (pb.scale * pb.scale)); m.loc_a = (float)pa.loc; m.isc2_a = (float)(1.0 / (pa.scale * pa.scale));
    m.l1_b = 0.0f; m.l1_a = 0.0f; m.hn_is2_s = m.hn_is2_o = 0.0f;
    for (int k = 0; k < 4; k++) { m.cs_mu[k] = (float)prior_mu[k]; m.cs_sg[k] = (float)prior_sigma[k]; }
    // constants of the potential: the coefficients' Normal normalisers, the rates' log B(a, b), those of mu0 / mu1 and the Gammas'
    const double HL2PI = 0.91893853320467274178;
    m.u_const = (Ks + 1) * (std::log(pb.scale) + HL2PI) + (Kp + Ka + 2) * (std::log(pa.scale) + HL2PI);
    m.u_const += std::lgamma(fca) + std::lgamma(fcb) - std::lgamma(fca + fcb) + std::lgamma(fua) + std::lgamma(fub) - std::lgamma(fua + fub);
    m.u_const += std::log(prior_mu[1]) + std::log(prior_mu[3]) + 2.0 * HL2PI;
    for (int f = 0; f < 2; f++) m.u_const += -prior_sigma[2 * f] * std::log(prior_sigma[2 * f + 1]) + std::lgamma(prior_sigma[2 * f]);
    m.n_total = N; m.s0 = 0; m.x_u = m.x_v = m.x_e = -1;
    m.n_rows = n_rows;
    re_geometry(m, N, 0, 0);
    // (bl_dataset_set_prior_family counts the alpha coefficients as Ko + 1: both detection blocks)
    ds->Ko = Kp + Ka + 1;
    ds->model = 6; ds->D = m.D;
    return BL_OK;
}

static int re_logp_grad(bl_dataset *ds, int B, const double *theta, double *U, double *grad)
{
    const size_t D = ds->D;
    std::vector<float> th32((size_t)B * D);
    for (size_t i = 0; i < th32.size(); i++) th32[i] = (float)theta[i];
    float *d_th = nullptr, *d_work = nullptr;
    double *d_U = nullptr, *d_grad = nullptr;
    DevScratch scratch;
    BL_HIP(scratch.alloc((void **)&d_th, th32.size() * 4));
    BL_HIP(scratch.alloc((void **)&d_work, (size_t)B * 2 * D * 4));
    BL_HIP(scratch.alloc((void **)&d_U, (size_t)B * 8));
    BL_HIP(scratch.alloc((void **)&d_grad, (size_t)B * D * 8));
    BL_HIP(hipMemcpy(d_th, th32.data(), th32.size() * 4, hipMemcpyHostToDevice));
    BlReModel m = ds->re;
    const size_t lds = re_geometry(m, m.n_sites, 0, 0);
    if (m.kind == 8) { // occu_comb: its own parity kernel (m.Ko = the wider detection block)
        const bool c4 = m.Ks <= 4 && m.Ko <= 4;
        const void *f = c4 ? (const void *)bl_comb_logp_kernel<4> : (const void *)bl_comb_logp_kernel<16>;
        if (lds) BL_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (c4) hipLaunchKernelGGL(bl_comb_logp_kernel<4>, dim3(B), dim3(BL_RE_NT), lds, nullptr, m, ds->comb, B, d_th, d_work, d_U, d_grad);
        else hipLaunchKernelGGL(bl_comb_logp_kernel<16>, dim3(B), dim3(BL_RE_NT), lds, nullptr, m, ds->comb, B, d_th, d_work, d_U, d_grad);
    } else
    // capacity 4 (the common case: short register arrays) or 16 covariates per side
    if (m.Ks <= 4 && m.Ko <= 4) {
        if (lds) BL_HIP(hipFuncSetAttribute((const void *)bl_re_logp_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(bl_re_logp_kernel<4>, dim3(B), dim3(BL_RE_NT), lds, nullptr, m, B, d_th, d_work, d_U, d_grad);
    } else {
        if (lds) BL_HIP(hipFuncSetAttribute((const void *)bl_re_logp_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(bl_re_logp_kernel<16>, dim3(B), dim3(BL_RE_NT), lds, nullptr, m, B, d_th, d_work, d_U, d_grad);
    }
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpy(U, d_U, (size_t)B * 8, hipMemcpyDeviceToHost));
    BL_HIP(hipMemcpy(grad, d_grad, (size_t)B * D * 8, hipMemcpyDeviceToHost));
    return BL_OK;
}

extern "C" int bl_logp_grad(bl_dataset *ds, int B, const double *theta, double *U, double *grad, int staged)
{
    if (!ds || !theta || !U || !grad || B <= 0) return bl_fail(BL_ERR_INVALID, "bl_logp_grad: bad argument");
    bl_env_snapshot();
    if (ds->in_flight) return bl_fail(BL_ERR_BUSY, "a NUTS launch is in flight on this handle");
    int rc = set_device(ds);
    if (rc) return rc;
    if (ds->model == 6) return re_logp_grad(ds, B, theta, U, grad);
    const int D = ds->D;
    int k, nloc, ld, lds_bytes, can_stage, ncw, wide, grp;
    choose_geometry(ds, 1, 0, &k, &nloc, &ld, &lds_bytes, &can_stage, &ncw, &wide, &grp);
    const int use_staged = staged && can_stage;
    if (!use_staged) { lds_bytes = BL_OFF_DATA; ncw = 4; grp = 0; }
    std::vector<float> th32((size_t)B * D);
    for (size_t i = 0; i < th32.size(); i++) th32[i] = (float)theta[i];
    float *d_th32 = nullptr;
    double *d_th = nullptr, *d_partial = nullptr, *d_U = nullptr, *d_grad = nullptr;
    DevScratch scratch;
    BL_HIP(scratch.alloc((void **)&d_th32, th32.size() * 4));
    BL_HIP(scratch.alloc((void **)&d_th, (size_t)B * D * 8));
    BL_HIP(scratch.alloc((void **)&d_partial, (size_t)B * k * 64 * 8));
    BL_HIP(scratch.alloc((void **)&d_U, (size_t)B * 8));
    BL_HIP(scratch.alloc((void **)&d_grad, (size_t)B * D * 8));
    BL_HIP(hipMemcpy(d_th32, th32.data(), th32.size() * 4, hipMemcpyHostToDevice));
    BL_HIP(hipMemcpy(d_th, theta, (size_t)B * D * 8, hipMemcpyHostToDevice));
    BL_HIP(hipMemset(d_partial, 0, (size_t)B * k * 64 * 8));
    BlLogpParams p{};
    p.dd = ds->dd; p.k = k; p.nloc = nloc; p.rec_stride = ld; p.B = B; p.theta = d_th32; p.partial = d_partial;
    p.max_abundance = ds->max_abundance;
    p.rn_off = BL_OFF_DATA + ((nloc + 1) / 2) * ld * 4; // (occu_rn: one species)
    p.lane_grp = ds->model == 8 ? dyn_lanes_per_pair(ds, 1) : grp;
    p.nmix_lds = nmix_table_in_lds(ds, use_staged, nloc, &lds_bytes);
    p.fp_mode = ds->fp_mode;
    p.nmix_tab = ds->d_tab;
    p.ncw = ncw;
    p.n_species = ds->nsp; p.sp_lds = ((nloc + 1) / 2) * ld;
    if (ds->nsp > 1 && !use_staged)
        return bl_fail(BL_ERR_UNSUPPORTED, "joint sampling of %d species needs the LDS-staged path (slice too large, or staged=0 requested)", ds->nsp);
    if (ds->model != 0 && !use_staged)
        return bl_fail(BL_ERR_UNSUPPORTED, "occu_rn / false-positive models need the LDS-staged path (slice too large, or staged=0 requested)");
    const int lrc = ds->kern->logp(&p, k, lds_bytes, use_staged, ds->model, nullptr);
    if (lrc != 0) return bl_fail(BL_ERR_NO_DEVICE, "logp kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
    hipLaunchKernelGGL(bl_logp_final_kernel, dim3(B), dim3(64), 0, nullptr, ds->dd, k, d_th, d_partial, d_U, d_grad);
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpy(U, d_U, (size_t)B * 8, hipMemcpyDeviceToHost));
    BL_HIP(hipMemcpy(grad, d_grad, (size_t)B * D * 8, hipMemcpyDeviceToHost));
    return BL_OK;
}

// ------------------------------------------------------------------- NUTS ----
static size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// Head of the run slab = the RESULT BLOCK of a launch: everything bl_nuts_fetch returns, contiguous, so that the gather
// over RCCL (comm_rccl.hpp) ships it as one buffer.  Offsets are a function of (chains, draws kept, D) only.
struct RunLayout { size_t draws, div, steps, acc, pot, eps, minv, nleap, end; };
static RunLayout result_layout(size_t C, size_t Sa, size_t D)
{
    RunLayout L{};
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off = align256(off + bytes); return o; };
    L.draws = carve(C * Sa * D * 4); L.div = carve(C * Sa); L.steps = carve(C * Sa * 4); L.acc = carve(C * Sa * 4);
    L.pot = carve(C * Sa * 4); L.eps = carve(C * 4); L.minv = carve(C * D * 4); L.nleap = carve(C * 16);
    L.end = off;
    return L;
}

// Random-effects model: k workgroups per chain, each with a slice of the sites; sampler state in device memory / LDS
// (re_kernel.hpp).  Outputs land in the same run-slab fields as the other models', so poll / wait / fetch are shared.
static int re_nuts_launch(bl_dataset *ds, const bl_nuts_config *cfg, hipStream_t st, int max_depth)
{
    const int C = cfg->num_chains, S = cfg->num_samples, W = cfg->num_warmup;
    const size_t D = ds->D, Sa = S > 0 ? S : 1;
    const BlReModel &g = ds->re;
    const int N = g.n_sites, V = g.T * g.J, per_site = (g.site_re ? 2 : 0) + (g.obs_re ? V : 0);
    // workgroups per chain: about a thousand coordinates, or eight thousand visits, each; all C k of them must be resident
    // at once (one per CU: they spin on each other's sums)
    int k = cfg->wgs_per_chain;
    if (k <= 0) {
        const long long work = std::max<long long>((long long)D, (long long)N * V / 8);
        k = (int)((2 * work + BL_RE_NT - 1) / BL_RE_NT);
        if (const char *e = bl_env(BL_ENV_RE_WGS)) k = atoi(e);
    }
    int ncu = 256;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, ds->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount; }
    k = std::max(1, std::min(std::min(k, 32), std::min(ncu * 7 / 8 / C, N * g.n_species))); // (an eighth of the CUs spare: nobody may wait for a CU)
    // several species: the chain's workgroups are n_species groups of kps, each group slicing the sites of its species
    const int nsp = g.n_species;
    int kps = std::max(1, k / nsp);
    const int nloc = (N + kps - 1) / kps;
    kps = (N + nloc - 1) / nloc; // no empty slice
    k = nsp * kps;
    if (k > 32) return bl_fail(BL_ERR_UNSUPPORTED, "n_species=%d needs %d workgroups per chain (at most 32)", nsp, k);
    if (C * k > ncu) return bl_fail(BL_ERR_UNSUPPORTED, "num_chains=%d random-effects chains need %d resident workgroups (%d CUs)", C, C * k, ncu);
    const int dl_max = g.G + nloc * per_site;

    const RunLayout RL = result_layout((size_t)C, Sa, D);
    size_t off = RL.end;
    auto carve = [&](size_t bytes) { size_t o = off; off = align256(off + bytes); return o; };
    const size_t o_draws = RL.draws, o_div = RL.div, o_steps = RL.steps, o_acc = RL.acc, o_pot = RL.pot, o_eps = RL.eps,
                 o_minv = RL.minv, o_nleap = RL.nleap, o_status = carve(16),
                 o_rng = carve((size_t)C * k * (dl_max + 2) * 16), o_init = carve((size_t)C * D * 4), o_dbg = carve(BL_DBG_SLOTS * 8),
                 o_xchg = carve((size_t)C * 2 * k * BL_RE_NRED_MAX * 8), o_loc = carve((size_t)C * 4), o_run = carve(sizeof(BlReRun));
    if (off > ds->run_bytes) {
        if (ds->d_run) hipFree(ds->d_run);
        ds->d_run = nullptr; ds->run_bytes = 0;
        BL_HIP(hipMalloc(&ds->d_run, off));
        ds->run_bytes = off;
    }
    const size_t state_bytes = (size_t)C * k * RE_SLOTS * dl_max * 4;
    if (state_bytes > ds->restate_bytes) {
        if (ds->d_restate) hipFree(ds->d_restate);
        ds->d_restate = nullptr; ds->restate_bytes = 0;
        BL_HIP(hipMalloc((void **)&ds->d_restate, state_bytes));
        ds->restate_bytes = state_bytes;
    }
    char *base = (char *)ds->d_run;
    ds->d_draws = (float *)(base + o_draws); ds->d_div = (unsigned char *)(base + o_div); ds->d_steps = (int *)(base + o_steps);
    ds->d_acc = (float *)(base + o_acc); ds->d_pot = (float *)(base + o_pot); ds->d_eps = (float *)(base + o_eps);
    ds->d_minv = (float *)(base + o_minv); ds->d_nleap = (long long *)(base + o_nleap); ds->d_status = (int *)(base + o_status);
    ds->d_rng = (uint32_t *)(base + o_rng); ds->d_init = (float *)(base + o_init); ds->d_dbg = (long long *)(base + o_dbg);
    ds->d_loc = (int *)(base + o_loc);

    // RNG: one stream per coordinate (the model's order), then the scalar and the direction stream; chains are D + 2 streams
    // apart (>= 64).  Each workgroup gets the streams of ITS coordinates in its own order; the fixed effects' and the two
    // scalar streams are replicated (every workgroup advances its copy identically).
    // (With at most 61 coordinates -- occu_cs, occu_rn with a false-positive rate and no effects -- the layout is the small models':
    // chains 64 streams apart, the scalar stream 63 and the direction stream 62, as the oracle's orc_nuts_run lays them out.)
    const bool small_layout = D + 2 <= (size_t)BL_RNG_STREAMS_PER_CHAIN - 1;
    const int stride = small_layout ? BL_RNG_STREAMS_PER_CHAIN : (int)D + 2;
    const int ext_scalar = small_layout ? BL_RNG_STREAMS_PER_CHAIN - 1 : (int)D, ext_dir = small_layout ? BL_RNG_STREAMS_PER_CHAIN - 2 : (int)D + 1;
    std::vector<uint32_t> all((size_t)C * stride * 4), rs((size_t)C * k * (dl_max + 2) * 4, 0u);
    rng_streams_strided(cfg->seed, cfg->chain_offset, stride, C, all.data());
    for (int c = 0; c < C; c++)
        for (int w = 0; w < k; w++) {
            const int sp = w / kps, s0 = (w - sp * kps) * nloc, cnt = std::min(nloc, N - s0);
            uint32_t *dst = rs.data() + ((size_t)c * k + w) * (dl_max + 2) * 4;
            const uint32_t *src = all.data() + (size_t)c * stride * 4;
            auto put = [&](int local, int ext) { memcpy(dst + (size_t)local * 4, src + (size_t)ext * 4, 16); };
            int at = 0;
            for (; at < g.G; at++) put(at, at);
            if (g.site_re) {
                for (int i = 0; i < cnt; i++) put(at + i, g.o_u + sp * N + s0 + i);
                for (int i = 0; i < cnt; i++) put(at + cnt + i, g.o_v + sp * N + s0 + i);
                at += 2 * cnt;
            }
            if (g.obs_re)
                for (int v = 0; v < V; v++)
                    for (int i = 0; i < cnt; i++) put(at + v * cnt + i, g.o_e + (sp * N + s0 + i) * V + v);
            put(dl_max, ext_scalar);   // scalar stream
            put(dl_max + 1, ext_dir);  // direction stream
        }
    BL_HIP(hipMemcpyAsync(ds->d_rng, rs.data(), rs.size() * 4, hipMemcpyHostToDevice, st));
    std::vector<float> it32;
    if (cfg->init_theta) {
        it32.resize((size_t)C * D);
        for (size_t i = 0; i < it32.size(); i++) it32[i] = (float)cfg->init_theta[i];
        BL_HIP(hipMemcpyAsync(ds->d_init, it32.data(), it32.size() * 4, hipMemcpyHostToDevice, st));
    }
    BlReRun run{};
    run.m = g;
    run.comb = ds->comb;
    const size_t lds = re_geometry(run.m, nloc, 1, dl_max);
    const bool cap4 = g.Ks <= 4 && g.Ko <= 4;
    run.num_chains = C; run.num_warmup = W; run.num_samples = S; run.max_depth = max_depth;
    run.k = k; run.nloc = nloc; run.dl_max = dl_max;
    run.xchg = (unsigned long long *)(base + o_xchg);
    { const char *e1 = bl_env(BL_ENV_NO_LOCAL); run.allow_local = (e1 && e1[0] == '1') ? 0 : 1; }
    run.xcd_local = ds->d_loc;
    run.target_accept = (float)(cfg->target_accept > 0.0 ? cfg->target_accept : 0.8);
    int32_t ws[32], we[32];
    run.nwin = adaptation_schedule(W, ws, we, 32);
    if (run.nwin > 32) return bl_fail(BL_ERR_INVALID, "adaptation schedule too long");
    for (int i = 0; i < 32; i++) run.win_end[i] = i < run.nwin ? we[i] : 0x7fffffff;
    run.state = ds->d_restate; run.rng = ds->d_rng;
    run.init_theta = cfg->init_theta ? ds->d_init : nullptr;
    run.abort_flag = ds->d_abort;
    run.draws = ds->d_draws; run.diverging = ds->d_div; run.num_steps = ds->d_steps; run.accept_prob = ds->d_acc;
    run.potential = ds->d_pot; run.step_size = ds->d_eps; run.inv_mass = ds->d_minv; run.nleap = ds->d_nleap; run.status = ds->d_status;
    run.dbg = ds->d_dbg;
    BlReRun *d_runp = (BlReRun *)(base + o_run);
    BL_HIP(hipMemcpyAsync(d_runp, &run, sizeof run, hipMemcpyHostToDevice, st));
    BL_HIP(hipStreamSynchronize(st));
    *ds->h_abort = 0;
    BL_HIP(hipEventRecord(ds->ev0, st));
    BL_HIP(hipMemsetAsync(ds->d_status, 0, 16, st));
    BL_HIP(hipMemsetAsync(ds->d_dbg, 0, BL_DBG_SLOTS * 8, st));
    BL_HIP(hipMemsetAsync(run.xchg, 0, (size_t)C * 2 * k * BL_RE_NRED_MAX * 8, st));
    BL_HIP(hipMemsetAsync(ds->d_loc, 0, (size_t)C * 4, st));
    // XCD-aware mapping in the kernel (surplus blocks exit at once)
    BL_HIP(re_nuts_dispatch(cap4 ? 4 : 16, run, 8 * k * ((C + 7) / 8), lds, st));
    snprintf(ds->kernel_name, sizeof ds->kernel_name, "%s", g_kernel_name);
    BL_HIP(hipEventRecord(ds->ev1, st));
    ds->stream = st; ds->in_flight = true; ds->have_run = true;
    ds->C = C; ds->S = S; ds->W = W; ds->k = k; ds->nloc = nloc; ds->lds_ld = 0; ds->lds_bytes = (int)lds; ds->staged = run.m.lds_rows | (run.m.lds_hot << 1); ds->nvp = 0; ds->ncw = BL_RE_NW; ds->lane_grp = 0;
    return BL_OK;
}

extern "C" int bl_nuts_launch(bl_dataset *ds, const bl_nuts_config *cfg, void *stream)
{
    if (!ds || !cfg) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (ds->in_flight) return bl_fail(BL_ERR_BUSY, "a NUTS launch is already in flight on this handle");
    bl_env_snapshot(); // the one read of the environment for this launch
    snprintf(ds->env_overrides, sizeof ds->env_overrides, "%s", bl_env_active().c_str());
    const int C = cfg->num_chains, S = cfg->num_samples, W = cfg->num_warmup, D = ds->D;
    if (C <= 0 || S < 0 || W < 0 || S + W <= 0) return bl_fail(BL_ERR_INVALID, "num_chains/num_samples/num_warmup out of range");
    if (C > 256) return bl_fail(BL_ERR_UNSUPPORTED, "num_chains=%d > 256 per device launch", C);
    const int max_depth = cfg->max_tree_depth > 0 ? cfg->max_tree_depth : 10;
    if (max_depth > BL_MAX_DEPTH) return bl_fail(BL_ERR_INVALID, "max_tree_depth > %d", BL_MAX_DEPTH);
    if (cfg->chain_offset < 0) return bl_fail(BL_ERR_INVALID, "chain_offset < 0");
    int rc = set_device(ds);
    if (rc) return rc;

    if (ds->model == 6) return re_nuts_launch(ds, cfg, (hipStream_t)stream, max_depth);

    int k, nloc, ld, lds_bytes, staged;
    int ncw, wide, grp;
    choose_geometry(ds, C, cfg->wgs_per_chain, &k, &nloc, &ld, &lds_bytes, &staged, &ncw, &wide, &grp);
    const int nvp = (D + 4 <= 16) ? 16 : (D + 4 <= 32 ? 32 : 64);

    // ---- (re)allocate run slab ----
    const size_t Sa = S > 0 ? S : 1;
    const RunLayout RL = result_layout((size_t)C, Sa, (size_t)D);
    size_t off = RL.end;
    auto carve = [&](size_t bytes) { size_t o = off; off = align256(off + bytes); return o; };
    const size_t o_draws = RL.draws, o_div = RL.div, o_steps = RL.steps, o_acc = RL.acc, o_pot = RL.pot, o_eps = RL.eps,
                 o_minv = RL.minv, o_nleap = RL.nleap, o_status = carve(16),
                 o_rng = carve((size_t)C * BL_RNG_STREAMS_PER_CHAIN * 16), o_init = carve((size_t)C * D * 4), o_dbg = carve(BL_DBG_SLOTS * 8), o_loc = carve((size_t)C * 4),
                 o_cold = carve(sizeof(BlNutsCold));
    if (off > ds->run_bytes) {
        if (ds->d_run) hipFree(ds->d_run);
        ds->d_run = nullptr; ds->run_bytes = 0;
        BL_HIP(hipMalloc(&ds->d_run, off));
        ds->run_bytes = off;
    }
    char *base = (char *)ds->d_run;
    ds->d_draws = (float *)(base + o_draws); ds->d_div = (unsigned char *)(base + o_div); ds->d_steps = (int *)(base + o_steps);
    ds->d_acc = (float *)(base + o_acc); ds->d_pot = (float *)(base + o_pot); ds->d_eps = (float *)(base + o_eps);
    ds->d_minv = (float *)(base + o_minv); ds->d_nleap = (long long *)(base + o_nleap); ds->d_status = (int *)(base + o_status);
    ds->d_rng = (uint32_t *)(base + o_rng); ds->d_init = (float *)(base + o_init); ds->d_dbg = (long long *)(base + o_dbg); ds->d_loc = (int *)(base + o_loc);
    int pitch = nvp; // granules between workgroup records
    { const char *e = bl_env(BL_ENV_PITCH); if (e && atoi(e) >= nvp && atoi(e) <= 4096) pitch = atoi(e); }
    pitch += pitch & 1; // (even: the paired records' 16-byte loads stay aligned -- nuts_kernel.hpp BL_POLL_PAIRS)
    // (which record form runs is the dispatcher's choice -- BIOLITH_HIP_GENERAL=1 among its inputs -- so the allocation and the clear
    // cover both: the pitched records and the compact form's fixed 2 KB slots, nuts_kernel.hpp BL_POLL_COMPACT)
    const size_t xb_pitched = (size_t)C * BL_XCHG_SLOTS * k * pitch * 8, xb_compact = (size_t)C * BL_XCHG_SLOTS * BL_COMPACT_SLOT_BYTES;
    const size_t xb = align256(xb_pitched > xb_compact ? xb_pitched : xb_compact);
    if (xb > ds->xchg_bytes) {
        if (ds->d_xchg) hipFree(ds->d_xchg);
        ds->d_xchg = nullptr; ds->xchg_bytes = 0;
        BL_HIP(hipMalloc((void **)&ds->d_xchg, xb));
        ds->xchg_bytes = xb;
    }

    hipStream_t st = (hipStream_t)stream;
    // ---- inputs: RNG streams (host-jumped), optional init ----
    std::vector<uint32_t> rs((size_t)C * BL_RNG_STREAMS_PER_CHAIN * 4);
    for (int c = 0; c < C; c++)
        rng_streams(cfg->seed, cfg->chain_offset + c, BL_RNG_STREAMS_PER_CHAIN, rs.data() + (size_t)c * BL_RNG_STREAMS_PER_CHAIN * 4);
    BL_HIP(hipMemcpyAsync(ds->d_rng, rs.data(), rs.size() * 4, hipMemcpyHostToDevice, st));
    if (cfg->init_theta) {
        std::vector<float> it32((size_t)C * D);
        for (size_t i = 0; i < it32.size(); i++) it32[i] = (float)cfg->init_theta[i];
        BL_HIP(hipMemcpyAsync(ds->d_init, it32.data(), it32.size() * 4, hipMemcpyHostToDevice, st));
    }
    // rarely-read constants + output pointers: one device-memory block
    BlNutsCold cold{};
    cold.num_warmup = W; cold.num_samples = S;
    cold.target_accept = (float)(cfg->target_accept > 0.0 ? cfg->target_accept : 0.8);
    int32_t ws[32], we[32];
    cold.nwin = adaptation_schedule(W, ws, we, 32);
    if (cold.nwin > 32) return bl_fail(BL_ERR_INVALID, "adaptation schedule too long");
    for (int i = 0; i < 32; i++) cold.win_end[i] = i < cold.nwin ? we[i] : 0x7fffffff;
    cold.loc_b = ds->dd.loc_b; cold.isc2_b = ds->dd.isc2_b; cold.loc_a = ds->dd.loc_a; cold.isc2_a = ds->dd.isc2_a;
    cold.l1_b = ds->dd.l1_b; cold.l1_a = ds->dd.l1_a;
    cold.prior_const = ds->dd.prior_const;
    cold.fp_a = (float)ds->fp_a; cold.fp_b = (float)ds->fp_b;
    cold.rng = ds->d_rng;
    cold.init_theta = cfg->init_theta ? ds->d_init : nullptr;
    cold.abort_flag = ds->d_abort;
    cold.draws = ds->d_draws; cold.diverging = ds->d_div; cold.num_steps = ds->d_steps; cold.accept_prob = ds->d_acc;
    cold.potential = ds->d_pot; cold.step_size = ds->d_eps; cold.inv_mass = ds->d_minv; cold.nleap = ds->d_nleap;
    cold.status = ds->d_status; cold.xcd_local = ds->d_loc; cold.dbg = ds->d_dbg;
    BlNutsCold *d_cold = (BlNutsCold *)(base + o_cold);
    BL_HIP(hipMemcpyAsync(d_cold, &cold, sizeof cold, hipMemcpyHostToDevice, st));
    BL_HIP(hipStreamSynchronize(st)); // staging buffers die with this scope
    *ds->h_abort = 0;

    BlNutsParams p{};
    p.rows = ds->dd.rows; p.n_sites = ds->dd.n_sites; p.n_stride = ds->dd.n_stride;
    p.T = ds->dd.T; p.J = ds->dd.J; p.Ks = ds->dd.Ks; p.Ko = ds->dd.Ko;
    p.num_chains = C;
    p.k = k; p.nloc = nloc; p.rec_stride = ld; p.nvp = nvp;
    p.max_depth = max_depth;
    p.max_abundance = ds->max_abundance;
    p.rn_off = BL_OFF_DATA + ((nloc + 1) / 2) * ld * 4; // (occu_rn: one species)
    p.lane_grp = ds->model == 8 ? dyn_lanes_per_pair(ds, C) : grp;
    p.nmix_lds = nmix_table_in_lds(ds, staged, nloc, &lds_bytes);
    // the GRP instantiation (lane groups; the exchange-free path of a one-workgroup chain) only where it is needed: the headline's kernel
    // stays the one-pair-per-lane form alone
    // (a chain of ONE workgroup always runs on BL_CWAVES_SINGLE compute waves: that kernel alone has the exchange-free path)
    p.grp_kernel = ((ds->model == 0 || ds->model == 2) && staged && (grp > 0 || ncw == BL_CWAVES_SINGLE)) ? 1 : 0;
    if (ncw == BL_CWAVES_SINGLE && k != 1) return bl_fail(BL_ERR_INVALID, "internal: %d compute waves are the one-workgroup form, k = %d", ncw, k);
    if (const char *e = bl_env(BL_ENV_GRP_KERNEL)) { if (e[0] == '1' && (ds->model == 0 || ds->model == 2) && staged) p.grp_kernel = 1; } // A/B knob: the GRP form although it is not needed
    p.fp_mode = ds->fp_mode;
    p.nmix_tab = ds->d_tab;
    p.ncw = ncw;
    p.n_species = ds->nsp; p.sp_lds = ((nloc + 1) / 2) * ld;
    if (ds->nsp > 1 && !staged)
        return bl_fail(BL_ERR_UNSUPPORTED, "joint sampling of %d species: the dataset slice does not fit the LDS-staged path", ds->nsp);
    p.wide = wide;
    p.xchg = ds->d_xchg;
    p.cold = d_cold;
    p.spin_limit = 5000000u; // microseconds (BIOLITH_HIP_SPIN_US overrides: tests of the bound)
    { const char *e = bl_env(BL_ENV_SPIN_US); if (e && atoi(e) > 0) p.spin_limit = (unsigned)atoi(e); }
    {   // developer knobs (A/B measurements): exchange form and poll spacing
        const char *e1 = bl_env(BL_ENV_NO_LOCAL), *e2 = bl_env(BL_ENV_POLL_SLEEP);
        p.allow_local = (e1 && e1[0] == '1') ? 0 : 1;
        p.poll_sleep = e2 ? atoi(e2) : 3;
        if (p.poll_sleep < 0 || p.poll_sleep > 127) p.poll_sleep = 3;
        const char *e3 = bl_env(BL_ENV_FIRST_DELAY);
        p.pitch = pitch;
        p.first_delay = e3 ? atoi(e3) : 0;
        if (p.first_delay < 0 || p.first_delay > 127) p.first_delay = 0;
    }

    // timed region: state re-init (guide G16 "re-initialise every call") + the persistent kernel
    BL_HIP(hipEventRecord(ds->ev0, st));
    BL_HIP(hipMemsetAsync(ds->d_xchg, 0, xb, st));
    BL_HIP(hipMemsetAsync(ds->d_status, 0, 16, st));
    BL_HIP(hipMemsetAsync(ds->d_dbg, 0, BL_DBG_SLOTS * 8, st));
    BL_HIP(hipMemsetAsync(ds->d_loc, 0, (size_t)C * 4, st));
    // XCD-aware mapping in the kernel (surplus blocks exit at once), or consecutive blocks per chain in the wide geometry
    const int grid = wide ? C * k : 8 * k * ((C + 7) / 8);
    if (ds->model != 0 && !staged)
        return bl_fail(BL_ERR_UNSUPPORTED, "occu_rn / false-positive model: the dataset slice does not fit the LDS-staged path");
    const int lrc = ds->kern->nuts(&p, grid, lds_bytes, staged, ds->model, st);
    if (lrc != 0) return bl_fail(BL_ERR_NO_DEVICE, "NUTS kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
    snprintf(ds->kernel_name, sizeof ds->kernel_name, "%s", g_kernel_name);
    BL_HIP(hipEventRecord(ds->ev1, st));
    ds->stream = st; ds->in_flight = true; ds->have_run = true;
    ds->C = C; ds->S = S; ds->W = W; ds->k = k; ds->nloc = nloc; ds->lds_ld = ld; ds->lds_bytes = lds_bytes; ds->staged = staged; ds->nvp = nvp; ds->ncw = ncw; ds->lane_grp = p.lane_grp;
    return BL_OK;
}

extern "C" int bl_nuts_poll(bl_dataset *ds, int *done)
{
    if (!ds || !done) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (!ds->in_flight) { *done = 1; return BL_OK; }
    hipSetDevice(ds->device);
    hipError_t e = hipEventQuery(ds->ev1);
    if (e == hipSuccess) { *done = 1; return BL_OK; }
    if (e == hipErrorNotReady) {
        (void)hipGetLastError(); // "not ready" is an answer, not an error: do not leave it behind as this thread's last error
        *done = 0;
        return BL_OK;
    }
    return bl_fail(BL_ERR_NO_DEVICE, "hipEventQuery: %s", hipGetErrorString(e));
}

extern "C" int bl_nuts_abort(bl_dataset *ds)
{
    if (!ds) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (ds->h_abort) __atomic_store_n(ds->h_abort, 1, __ATOMIC_SEQ_CST);
    return BL_OK;
}

extern "C" int bl_nuts_wait(bl_dataset *ds)
{
    if (!ds) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (!ds->have_run) return bl_fail(BL_ERR_INVALID, "no NUTS launch on this handle");
    int rc = set_device(ds);
    if (rc) return rc;
    if (ds->in_flight) {
        BL_HIP(hipEventSynchronize(ds->ev1));
        ds->in_flight = false;
    }
    int status = 0;
    BL_HIP(hipMemcpy(&status, ds->d_status, 4, hipMemcpyDeviceToHost));
    if (status == BL_ERR_TIMEOUT) return bl_fail(BL_ERR_TIMEOUT, "in-kernel exchange spin bound hit (a workgroup was not resident?)");
    if (status == BL_ERR_ABORTED) return bl_fail(BL_ERR_ABORTED, "sampling aborted on request");
    if (status != 0) return bl_fail(BL_ERR_NO_DEVICE, "kernel reported status %d", status);
    return BL_OK;
}

extern "C" int bl_nuts_fetch(bl_dataset *ds, bl_nuts_output *out)
{
    if (!ds || !out) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (!ds->have_run || ds->in_flight) return bl_fail(BL_ERR_BUSY, "no finished NUTS launch to fetch");
    int rc = set_device(ds);
    if (rc) return rc;
    const size_t C = ds->C, S = ds->S, D = ds->D;
    if (out->draws && S) BL_HIP(hipMemcpy(out->draws, ds->d_draws, C * S * D * 4, hipMemcpyDeviceToHost));
    if (out->diverging && S) BL_HIP(hipMemcpy(out->diverging, ds->d_div, C * S, hipMemcpyDeviceToHost));
    if (out->num_steps && S) BL_HIP(hipMemcpy(out->num_steps, ds->d_steps, C * S * 4, hipMemcpyDeviceToHost));
    if (out->accept_prob && S) BL_HIP(hipMemcpy(out->accept_prob, ds->d_acc, C * S * 4, hipMemcpyDeviceToHost));
    if (out->potential_energy && S) BL_HIP(hipMemcpy(out->potential_energy, ds->d_pot, C * S * 4, hipMemcpyDeviceToHost));
    if (out->step_size) BL_HIP(hipMemcpy(out->step_size, ds->d_eps, C * 4, hipMemcpyDeviceToHost));
    if (out->inv_mass) BL_HIP(hipMemcpy(out->inv_mass, ds->d_minv, C * D * 4, hipMemcpyDeviceToHost));
    if (out->n_leapfrog) BL_HIP(hipMemcpy(out->n_leapfrog, ds->d_nleap, C * 16, hipMemcpyDeviceToHost));
    return BL_OK;
}

extern "C" int bl_nuts_run(bl_dataset *ds, const bl_nuts_config *cfg, bl_nuts_output *out)
{
    int rc = bl_nuts_launch(ds, cfg, nullptr);
    if (rc) return rc;
    rc = bl_nuts_wait(ds);
    if (rc) return rc;
    return out ? bl_nuts_fetch(ds, out) : BL_OK;
}

extern "C" int bl_nuts_elapsed_ms(bl_dataset *ds, float *ms)
{
    if (!ds || !ms) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (!ds->have_run || ds->in_flight) return bl_fail(BL_ERR_BUSY, "no finished NUTS launch");
    BL_HIP(hipEventElapsedTime(ms, ds->ev0, ds->ev1));
    return BL_OK;
}

extern "C" int bl_nuts_device_draws(bl_dataset *ds, void **dev_ptr, size_t *bytes)
{
    if (!ds || !dev_ptr || !bytes) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (!ds->have_run) return bl_fail(BL_ERR_INVALID, "no NUTS launch on this handle");
    *dev_ptr = ds->d_draws;
    *bytes = (size_t)ds->C * ds->S * ds->D * 4;
    return BL_OK;
}

extern "C" int bl_nuts_debug_counters(bl_dataset *ds, int64_t *out, int n)
{
    if (!ds || !out || n <= 0 || n > BL_DBG_SLOTS) return bl_fail(BL_ERR_INVALID, "bad argument");
    if (!ds->have_run || ds->in_flight) return bl_fail(BL_ERR_BUSY, "no finished NUTS launch");
    BL_HIP(hipMemcpy(out, ds->d_dbg, (size_t)n * 8, hipMemcpyDeviceToHost));
    return BL_OK;
}

extern "C" int bl_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0) return bl_fail(BL_ERR_INVALID, "bl_host_alloc: NULL / empty");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bl_fail(BL_ERR_NO_DEVICE, "no HIP device visible");
    BL_HIP(hipHostMalloc(out, bytes, hipHostMallocPortable));
    return BL_OK;
}
extern "C" int bl_host_free(void *ptr)
{
    if (ptr) BL_HIP(hipHostFree(ptr));
    return BL_OK;
}

// (kernels_inst.hip: bl_launch hands over the name of the instantiation it launches)
extern "C" void bl_note_kernel_name(const char *name)
{
    snprintf(g_kernel_name, sizeof g_kernel_name, "%s", name ? name : "");
}

extern "C" int bl_nuts_kernel_name(bl_dataset *ds, char *buf, int n)
{
    if (!ds || !buf || n <= 0) return bl_fail(BL_ERR_INVALID, "bl_nuts_kernel_name: bad argument");
    if (!ds->have_run) return bl_fail(BL_ERR_INVALID, "no NUTS launch on this handle");
    snprintf(buf, (size_t)n, "%s", ds->kernel_name);
    return BL_OK;
}

extern "C" int bl_nuts_lane_group(bl_dataset *ds, int *period_lanes, int *visit_lanes)
{
    if (!ds) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (!ds->have_run) return bl_fail(BL_ERR_INVALID, "no NUTS launch on this handle");
    int gt = 1, gj = 1;
    if (ds->model == 8) gt = ds->lane_grp > 0 ? ds->lane_grp : 1;                                    // dynamic occupancy: the seasons
    else if (ds->model == 0 || ds->model == 2 || ds->model == 3 || ds->model == 4) { gt = 1 << (ds->lane_grp & 15); gj = 1 << (ds->lane_grp >> 4); }
    if (period_lanes) *period_lanes = gt;
    if (visit_lanes) *visit_lanes = gj;
    return BL_OK;
}

extern "C" int bl_nuts_env_overrides(bl_dataset *ds, char *buf, int n)
{
    if (!ds || !buf || n <= 0) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (!ds->have_run) return bl_fail(BL_ERR_INVALID, "no NUTS launch on this handle");
    snprintf(buf, (size_t)n, "%s", ds->env_overrides);
    return BL_OK;
}

extern "C" int bl_nuts_geometry(bl_dataset *ds, int *wgs_per_chain, int *threads_per_wg, int *lds_bytes, int *lds_staged,
                                int *chains_on_l2_local_exchange)
{
    if (!ds) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (!ds->have_run) return bl_fail(BL_ERR_INVALID, "no NUTS launch on this handle");
    if (wgs_per_chain) *wgs_per_chain = ds->k;
    if (threads_per_wg) *threads_per_wg = ds->model == 6 ? BL_RE_NT : 64 * (ds->ncw + 1);
    if (lds_bytes) *lds_bytes = ds->lds_bytes;
    if (lds_staged) *lds_staged = ds->staged;
    if (chains_on_l2_local_exchange) {
        *chains_on_l2_local_exchange = 0;
        if (!ds->in_flight && ds->d_loc) {
            std::vector<int> loc(ds->C, 0);
            BL_HIP(hipMemcpy(loc.data(), ds->d_loc, (size_t)ds->C * 4, hipMemcpyDeviceToHost));
            for (int v : loc) *chains_on_l2_local_exchange += v;
        }
    }
    return BL_OK;
}

// Bytes of one workgroup's exchange record in the last FINISHED launch: 64 where the kernel that ran laid out compact records (it says
// so itself, in the status block's second word), else granules per record x 8 (128, 256 or 512); 0 for the random-effects samplers,
// whose exchange is their own.
extern "C" int bl_nuts_record_bytes(bl_dataset *ds, int *record_bytes)
{
    if (!ds || !record_bytes) return bl_fail(BL_ERR_INVALID, "NULL argument");
    if (!ds->have_run || ds->in_flight) return bl_fail(BL_ERR_BUSY, "no finished NUTS launch");
    int rc = set_device(ds);
    if (rc) return rc;
    int said = 0;
    if (ds->model != 6) BL_HIP(hipMemcpy(&said, ds->d_status + 1, 4, hipMemcpyDeviceToHost));
    *record_bytes = said > 0 ? said : ds->nvp * 8;
    return BL_OK;
}

// ------------------------------------------------- deterministic sites ----
// psi[n][t][i] = sigmoid(beta0 + x_i . beta), prob_detection[n][j][t][i] = sigmoid(alpha0 + w_itj . alpha), with the handle's random
// effects; the abundance models' psi and occu_cop's prob_detection are rates, exp of the predictor.  Kernels: predict.hip.
extern "C" int bl_deterministic(bl_dataset *ds, int n_draws, const float *draws, float *psi, float *prob_detection)
{
    if (!ds || !draws || n_draws <= 0) return bl_fail(BL_ERR_INVALID, "bl_deterministic: bad argument");
    if (ds->nsp > 1) return bl_fail(BL_ERR_UNSUPPORTED, "bl_deterministic: a joint-species handle samples; take the sites from one handle per species");
    if (ds->model == 8) return bl_fail(BL_ERR_UNSUPPORTED, "bl_deterministic: the dynamic occupancy model's sites (psi, gamma, eps) are formed by the caller from the draws");
    if (ds->model == 6 && ds->re.kind == 8)
        return bl_fail(BL_ERR_UNSUPPORTED, "bl_deterministic: occu_comb's sites (psi, PC / ARU detection probabilities) are formed by the caller from the draws");
    if (ds->in_flight) return bl_fail(BL_ERR_BUSY, "a NUTS launch is in flight on this handle");
    int rc = set_device(ds);
    if (rc || (prob_detection && (rc = upload_once(&ds->d_wraw, ds->h_wraw)))) return rc;
    BlPredictParams p = predict_params(ds, 0);
    const size_t cells = (size_t)p.T * p.N * 4; // per draw
    const DrawOut outs[] = {{psi, cells, (void **)&p.psi, false}, {prob_detection, cells * p.J, (void **)&p.prob, false}};
    return run_over_draws(ds, n_draws, draws, cells * (prob_detection ? (size_t)p.J : 1), outs, p, bl_launch_deterministic);
}

// ---- the deterministic sites' summary over the draws: mean, sd and order statistics per cell, fused ----
// (No counterpart in the reference.)  Kernels: site_summary.hip.  They read what bl_deterministic's kernels read and every draw, and
// write per cell: a launch per wanted site over all the draws, which goes out when they are up (run_over_draws's one chunk: nothing
// here grows with the draws) and is done before run_over_draws lets go of them.
extern "C" int bl_site_summary(bl_dataset *ds, int n_draws, const float *draws, int n_ranks, const int32_t *ranks, double *psi_mean,
                               double *psi_sd, float *psi_order, double *prob_mean, double *prob_sd, float *prob_order)
{
    const bool first = psi_mean || psi_sd || psi_order, second = prob_mean || prob_sd || prob_order, order = psi_order || prob_order;
    if (!ds || !draws || n_draws <= 0 || !(first || second)) return bl_fail(BL_ERR_INVALID, "bl_site_summary: bad argument");
    if (ds->nsp > 1) return bl_fail(BL_ERR_UNSUPPORTED, "bl_site_summary: a joint-species handle samples; take the sites from one handle per species");
    if (ds->model == 8) return bl_fail(BL_ERR_UNSUPPORTED, "bl_site_summary: the dynamic occupancy model's sites (psi, gamma, eps) are formed by the caller from the draws");
    if (ds->model == 6 && ds->re.kind == 8)
        return bl_fail(BL_ERR_UNSUPPORTED, "bl_site_summary: occu_comb's sites (psi, PC / ARU detection probabilities) are formed by the caller from the draws");
    if (ds->in_flight) return bl_fail(BL_ERR_BUSY, "a NUTS launch is in flight on this handle");
    if (order) {
        if (n_ranks <= 0 || !ranks) return bl_fail(BL_ERR_INVALID, "bl_site_summary: an order output is wanted and n_ranks=%d", n_ranks);
        if (n_ranks > BL_SUMMARY_MAX_RANKS)
            return bl_fail(BL_ERR_UNSUPPORTED, "bl_site_summary: n_ranks=%d above BL_SUMMARY_MAX_RANKS=%d", n_ranks, BL_SUMMARY_MAX_RANKS);
        for (int r = 0; r < n_ranks; r++)
            if (ranks[r] < 0 || ranks[r] >= n_draws)
                return bl_fail(BL_ERR_INVALID, "bl_site_summary: ranks[%d]=%d outside 0 .. n_draws - 1 = %d", r, (int)ranks[r], n_draws - 1);
    }
    int rc = set_device(ds);
    if (rc || (second && (rc = upload_once(&ds->d_wraw, ds->h_wraw)))) return rc;
    BlSiteSummaryParams p{};
    p.rows = ds->d_rows; p.wraw = ds->d_wraw; p.ns = ds->n_stride;
    p.N = ds->dims.n_sites; p.T = ds->dims.n_periods; p.J = ds->dims.n_replicates; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = ds->D;
    p.model = branch_model(ds); p.c = draw_coords(ds); p.n_draws = n_draws;
    p.n_ranks = order ? n_ranks : 0;
    for (int r = 0; r < p.n_ranks; r++) p.ranks[r] = ranks[r];
    const size_t sites = (size_t)p.N, visits = sites * p.T * p.J;
    // one site's device outputs and the host arrays they go back to
    struct Site {
        size_t cells;
        double *mean, *sd;
        float *order;
        double *d_mean = nullptr, *d_sd = nullptr;
        float *d_order = nullptr;
    } site[2] = {{sites, psi_mean, psi_sd, psi_order}, {visits, prob_mean, prob_sd, prob_order}};
    DevScratch scratch;
    for (Site &s : site) {
        if (s.mean) BL_HIP(scratch.alloc((void **)&s.d_mean, s.cells * 8));
        if (s.sd) BL_HIP(scratch.alloc((void **)&s.d_sd, s.cells * 8));
        if (s.order) BL_HIP(scratch.alloc((void **)&s.d_order, s.cells * 4 * p.n_ranks));
    }
    void *none = nullptr;
    const DrawOut outs[] = {{nullptr, 0, &none, false}}; // (nothing per draw)
    rc = run_over_draws(ds, n_draws, draws, 0, outs, [&](const float *d_draws, int n0, int, int) {
        if (n0 != 0) return hipSuccess;
        p.draws = d_draws;
        int e = 0;
        for (int k = 0; k < 2 && !e; k++) {
            p.mean = site[k].d_mean; p.sd = site[k].d_sd; p.order = site[k].d_order;
            if (p.mean || p.sd || p.order) e = k ? bl_launch_site_summary_prob(&p, nullptr) : bl_launch_site_summary_psi(&p, nullptr);
        }
        if (!e) e = (int)hipStreamSynchronize(nullptr);
        return (hipError_t)e;
    });
    if (rc) return rc;
    for (const Site &s : site) {
        if (s.mean) BL_HIP(hipMemcpy(s.mean, s.d_mean, s.cells * 8, hipMemcpyDeviceToHost));
        if (s.sd) BL_HIP(hipMemcpy(s.sd, s.d_sd, s.cells * 8, hipMemcpyDeviceToHost));
        if (s.order) BL_HIP(hipMemcpy(s.order, s.d_order, s.cells * 4 * p.n_ranks, hipMemcpyDeviceToHost));
    }
    return BL_OK;
}

// ---- the deterministic sites' convergence diagnostics over the chains' draws: n_eff, split r_hat, mean and sd per cell, fused ----
// (No counterpart in the reference.)  Kernels: site_diagnostics.hip.  As bl_site_summary: a launch per wanted site over all the draws,
// which goes out when they are up and is done before run_over_draws lets go of them.
extern "C" int bl_site_diagnostics(bl_dataset *ds, int n_draws, const float *draws, int n_chains, double *psi_n_eff, double *psi_r_hat,
                                   double *psi_mean, double *psi_sd, double *prob_n_eff, double *prob_r_hat, double *prob_mean,
                                   double *prob_sd)
{
    const bool first = psi_n_eff || psi_r_hat || psi_mean || psi_sd, second = prob_n_eff || prob_r_hat || prob_mean || prob_sd;
    if (!ds || !draws || n_draws <= 0 || !(first || second)) return bl_fail(BL_ERR_INVALID, "bl_site_diagnostics: bad argument");
    if (ds->nsp > 1) return bl_fail(BL_ERR_UNSUPPORTED, "bl_site_diagnostics: a joint-species handle samples; take the sites from one handle per species");
    if (ds->model == 8) return bl_fail(BL_ERR_UNSUPPORTED, "bl_site_diagnostics: the dynamic occupancy model's sites (psi, gamma, eps) are formed by the caller from the draws");
    if (ds->model == 6 && ds->re.kind == 8)
        return bl_fail(BL_ERR_UNSUPPORTED, "bl_site_diagnostics: occu_comb's sites (psi, PC / ARU detection probabilities) are formed by the caller from the draws");
    if (ds->in_flight) return bl_fail(BL_ERR_BUSY, "a NUTS launch is in flight on this handle");
    if (n_chains < 1 || n_draws % n_chains != 0)
        return bl_fail(BL_ERR_INVALID, "bl_site_diagnostics: n_draws=%d is not n_chains=%d chains of equal length", n_draws, n_chains);
    if (n_draws / n_chains < 2)
        return bl_fail(BL_ERR_INVALID, "bl_site_diagnostics: %d draws per chain, at least 2", n_draws / n_chains);
    int rc = set_device(ds);
    if (rc || (second && (rc = upload_once(&ds->d_wraw, ds->h_wraw)))) return rc;
    BlSiteDiagnosticsParams p{};
    p.rows = ds->d_rows; p.wraw = ds->d_wraw; p.ns = ds->n_stride;
    p.N = ds->dims.n_sites; p.T = ds->dims.n_periods; p.J = ds->dims.n_replicates; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = ds->D;
    p.model = branch_model(ds); p.c = draw_coords(ds); p.n_chains = n_chains; p.n = n_draws / n_chains;
    const size_t sites = (size_t)p.N, visits = sites * p.T * p.J;
    // one site's host arrays and the device outputs they come back from: n_eff, r_hat, mean, sd
    struct Site {
        size_t cells;
        double *host[4];
        double *dev[4] = {nullptr, nullptr, nullptr, nullptr};
    } site[2] = {{sites, {psi_n_eff, psi_r_hat, psi_mean, psi_sd}}, {visits, {prob_n_eff, prob_r_hat, prob_mean, prob_sd}}};
    DevScratch scratch;
    for (Site &s : site)
        for (int k = 0; k < 4; k++)
            if (s.host[k]) BL_HIP(scratch.alloc((void **)&s.dev[k], s.cells * 8));
    // the chains' means: one workspace, sized for the larger of the launches (they run one after the other)
    const size_t ws = std::max(first ? bl_site_diagnostics_workspace(&p, false) : 0, second ? bl_site_diagnostics_workspace(&p, true) : 0);
    BL_HIP(scratch.alloc((void **)&p.means, ws * 8));
    void *none = nullptr;
    const DrawOut outs[] = {{nullptr, 0, &none, false}}; // (nothing per draw)
    rc = run_over_draws(ds, n_draws, draws, 0, outs, [&](const float *d_draws, int n0, int, int) {
        if (n0 != 0) return hipSuccess;
        p.draws = d_draws;
        int e = 0;
        for (int k = 0; k < 2 && !e; k++) {
            p.n_eff = site[k].dev[0]; p.r_hat = site[k].dev[1]; p.mean = site[k].dev[2]; p.sd = site[k].dev[3];
            if (p.n_eff || p.r_hat || p.mean || p.sd) e = k ? bl_launch_site_diagnostics_prob(&p, nullptr) : bl_launch_site_diagnostics_psi(&p, nullptr);
        }
        if (!e) e = (int)hipStreamSynchronize(nullptr);
        return (hipError_t)e;
    });
    if (rc) return rc;
    for (const Site &s : site)
        for (int k = 0; k < 4; k++)
            if (s.host[k]) BL_HIP(hipMemcpy(s.host[k], s.dev[k], s.cells * 8, hipMemcpyDeviceToHost));
    return BL_OK;
}

// ---- totals over regions: per draw the weighted total of the first site and of the latent state per region, fused ----
// (No counterpart in the reference.)  Kernels: regional_totals.hip.  They read the site covariates at the head of the handle's rows and
// nothing else of it, so nothing is uploaded but the slots: the site indices stable-sorted by region, every region padded to whole
// 64-lane waves (regional_totals.hpp).  run_over_draws cuts the draws so that the workspace and the chunk's totals stay within its 256 MB
// each (BL_TOTALS_WORKSPACE_BYTES says so in the header).
static_assert(BL_TOTALS_WORKSPACE_BYTES == (256u << 20), "bl_regional_totals states run_over_draws' bound");

// The slots of the totals' kernels (regional_totals.hpp, trajectory_totals.hpp), checked, laid out and taken to the device for `entry`.
struct RegionSlots {
    int n_waves = 0;
    int *site = nullptr, *wave_first = nullptr; // device; scratch's
    double *w = nullptr;                        // device, NULL without weights
};
static int region_slots(const char *entry, int N, int G, const int32_t *region, const double *weight, DevScratch &scratch, RegionSlots &out)
{
    if (G < 1) return bl_fail(BL_ERR_INVALID, "%s: n_regions=%d, at least 1", entry, G);
    std::vector<int> wave_first((size_t)G + 1, 0);
    for (int i = 0; i < N; i++) {
        if (region[i] < -1 || region[i] >= G)
            return bl_fail(BL_ERR_INVALID, "%s: region[%d]=%d outside -1 .. n_regions - 1 = %d", entry, i, (int)region[i], G - 1);
        if (weight && !std::isfinite(weight[i])) return bl_fail(BL_ERR_INVALID, "%s: weight[%d]=%g is not finite", entry, i, weight[i]);
        if (region[i] >= 0) wave_first[(size_t)region[i] + 1]++; // (the region's sites for now)
    }
    if ((size_t)N + (size_t)63 * G > (size_t)INT_MAX)
        return bl_fail(BL_ERR_UNSUPPORTED, "%s: %d sites in %d regions need more than 2^31 slots", entry, N, G);
    for (int g = 0; g < G; g++) wave_first[(size_t)g + 1] = wave_first[g] + (wave_first[(size_t)g + 1] + 63) / 64;
    const int W = wave_first[G];
    std::vector<int> slot_site((size_t)W * 64, -1), cursor(G);
    std::vector<double> slot_w(weight ? (size_t)W * 64 : 0, 0.0);
    for (int g = 0; g < G; g++) cursor[g] = wave_first[g] * 64;
    for (int i = 0; i < N; i++) { // (in site order: a stable sort by region)
        if (region[i] < 0) continue;
        const int s = cursor[region[i]]++;
        slot_site[s] = i;
        if (weight) slot_w[s] = weight[i];
    }
    out.n_waves = W;
    BL_HIP(scratch.alloc((void **)&out.site, slot_site.size() * 4));
    BL_HIP(scratch.alloc((void **)&out.wave_first, wave_first.size() * 4));
    BL_HIP(hipMemcpy(out.site, slot_site.data(), slot_site.size() * 4, hipMemcpyHostToDevice));
    BL_HIP(hipMemcpy(out.wave_first, wave_first.data(), wave_first.size() * 4, hipMemcpyHostToDevice));
    if (weight) {
        BL_HIP(scratch.alloc((void **)&out.w, slot_w.size() * 8));
        BL_HIP(hipMemcpy(out.w, slot_w.data(), slot_w.size() * 8, hipMemcpyHostToDevice));
    }
    return BL_OK;
}

extern "C" int bl_regional_totals(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, int n_regions, const int32_t *region,
                                  const double *weight, double *site_total, double *latent_total)
{
    int rc = per_draw_front("bl_regional_totals", ds, n_draws, draws, (site_total || latent_total) && region,
                            [](const bl_dataset *d) {
                                return d->nsp == 1 && ((d->model >= 0 && d->model <= 4) || re_kind_in(d, {0, 1, 2, 3, 4, 5, 6, 7}));
                            },
                            "occu, occu_cs, occu_cop, occu_rn and nmixture: the handles of bl_predict, bl_predict_counts and bl_predict_scores");
    if (rc) return rc;
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, G = n_regions;
    DevScratch scratch;
    RegionSlots slots;
    if ((rc = region_slots("bl_regional_totals", N, G, region, weight, scratch, slots))) return rc;
    const int W = slots.n_waves;

    BlRegionalTotalsParams p{};
    p.rows = ds->d_rows; p.ns = ds->n_stride; p.N = N; p.T = T; p.Ks = ds->Ks; p.D = ds->D;
    p.model = branch_model(ds); p.scores = re_kind_in(ds, {1}); p.K = ds->max_abundance; p.c = draw_coords(ds);
    p.seed = (unsigned long long)seed;
    p.n_slots = W * 64; p.n_waves = W; p.n_regions = G;
    p.site_rows = site_total ? 1 : 0; p.latent_rows = latent_total ? T : 0;
    p.slot_site = slots.site; p.slot_w = slots.w; p.wave_first = slots.wave_first;
    const size_t rows = (size_t)p.site_rows + p.latent_rows;
    const DrawOut outs[] = {{site_total, (size_t)G * 8, (void **)&p.site_total, false},
                            {latent_total, (size_t)T * G * 8, (void **)&p.latent_total, false},
                            {nullptr, rows * W * 8, (void **)&p.part, true}};
    return run_over_draws(ds, n_draws, draws, rows * std::max(W, G) * 8, outs, p, bl_launch_regional_totals);
}

// ---- response curves: per draw and grid value the weighted total over the sites with one covariate set to the value, fused ----
// (No counterpart in the reference.)  Kernels: response_curves.hip.  The site side reads the site covariates at the head of the handle's
// rows, the obs side the raw observation covariates (up on first use); next to them go up the grid values and the weights, nothing
// else.  run_over_draws cuts the draws so that the workspace, n_values rows of one double per run of 64 sites a draw, stays within
// BL_TOTALS_WORKSPACE_BYTES.
extern "C" int bl_response_curves(bl_dataset *ds, int n_draws, const float *draws, int side, int covariate, int n_values,
                                  const float *values, const double *weight, double *curve_total)
{
    int rc = per_draw_front("bl_response_curves", ds, n_draws, draws, true,
                            [](const bl_dataset *d) {
                                return d->nsp == 1 && ((d->model >= 0 && d->model <= 4) || re_kind_in(d, {0, 1, 2, 3, 4, 5, 6, 7}));
                            },
                            "occu, occu_cs, occu_cop, occu_rn and nmixture: the handles of bl_regional_totals");
    if (rc) return rc;
    const int N = ds->dims.n_sites, V = n_values;
    if (side != 0 && side != 1) return bl_fail(BL_ERR_INVALID, "bl_response_curves: side=%d, 0 (site) or 1 (obs)", side);
    const int K = side ? ds->Ko : ds->Ks;
    if (covariate < 0 || covariate >= K)
        return bl_fail(BL_ERR_INVALID, "bl_response_curves: covariate=%d outside 0 .. %s - 1 = %d", covariate, side ? "Ko" : "Ks", K - 1);
    if (V < 1) return bl_fail(BL_ERR_INVALID, "bl_response_curves: n_values=%d, at least 1", V);
    if (!values) return bl_fail(BL_ERR_INVALID, "bl_response_curves: values is NULL");
    if (!curve_total) return bl_fail(BL_ERR_INVALID, "bl_response_curves: curve_total is NULL");
    for (int g = 0; g < V; g++)
        if (!std::isfinite(values[g])) return bl_fail(BL_ERR_INVALID, "bl_response_curves: values[%d]=%g is not finite", g, (double)values[g]);
    for (int i = 0; weight && i < N; i++)
        if (!std::isfinite(weight[i])) return bl_fail(BL_ERR_INVALID, "bl_response_curves: weight[%d]=%g is not finite", i, weight[i]);
    if (side && (rc = upload_once(&ds->d_wraw, ds->h_wraw))) return rc;

    BlResponseCurvesParams p{};
    p.rows = ds->d_rows; p.wraw = ds->d_wraw; p.ns = ds->n_stride;
    p.N = N; p.T = ds->dims.n_periods; p.J = ds->dims.n_replicates; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = ds->D;
    p.model = branch_model(ds); p.c = draw_coords(ds);
    p.side = side; p.k = covariate; p.n_values = V; p.n_runs = (N + 63) / 64;
    DevScratch scratch;
    float *d_values = nullptr;
    double *d_w = nullptr;
    BL_HIP(scratch.alloc((void **)&d_values, (size_t)V * 4));
    BL_HIP(hipMemcpy(d_values, values, (size_t)V * 4, hipMemcpyHostToDevice));
    if (weight) {
        BL_HIP(scratch.alloc((void **)&d_w, (size_t)N * 8));
        BL_HIP(hipMemcpy(d_w, weight, (size_t)N * 8, hipMemcpyHostToDevice));
    }
    p.values = d_values; p.weight = d_w;
    const size_t per_draw = (size_t)V * p.n_runs * 8; // the workspace's bytes a draw (>= the totals')
    const DrawOut outs[] = {{curve_total, (size_t)V * 8, (void **)&p.total, false}, {nullptr, per_draw, (void **)&p.part, true}};
    return run_over_draws(ds, n_draws, draws, per_draw, outs, p, bl_launch_response_curves);
}

// ---- trajectory totals: per draw of an occu_dyn handle and region the weighted totals of the occupancy over the seasons, fused ----
// (BUILDER-DEFINED, like the model.)  Kernels: trajectory_totals.hip.  They read the site covariates at the head of the handle's rows and
// no visit; T is the call's.  The slots, the workspace and the chunking of the draws are bl_regional_totals'.
static_assert(BL_TT_MAX_KS == BL_DYN_MAX_KS, "trajectory_totals.hip stages the site covariates an occu_dyn handle takes");
extern "C" int bl_trajectory_totals(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, int n_periods, int n_regions,
                                    const int32_t *region, const double *weight, double *occupancy, double *colonised, double *extinct,
                                    double *equilibrium, double *z, double *z_colonised, double *z_extinct)
{
    double *const host[BL_TT_OUTPUTS] = {occupancy, colonised, extinct, equilibrium, z, z_colonised, z_extinct};
    const bool any = std::any_of(host, host + BL_TT_OUTPUTS, [](const double *h) { return h != nullptr; });
    int rc = per_draw_front("bl_trajectory_totals", ds, n_draws, draws, any && region,
                            [](const bl_dataset *d) { return d->model == 8; },
                            "occu_dyn only; the static models' totals are bl_regional_totals");
    if (rc) return rc;
    const int N = ds->dims.n_sites, T = n_periods, G = n_regions;
    if (T < 1) return bl_fail(BL_ERR_INVALID, "bl_trajectory_totals: n_periods=%d, at least 1", T);
    if (T > (INT_MAX - 1) / 6) return bl_fail(BL_ERR_UNSUPPORTED, "bl_trajectory_totals: n_periods=%d, at most %d", T, (INT_MAX - 1) / 6);
    DevScratch scratch;
    RegionSlots slots;
    if ((rc = region_slots("bl_trajectory_totals", N, G, region, weight, scratch, slots))) return rc;
    const int W = slots.n_waves;

    BlTrajectoryTotalsParams p{};
    p.rows = ds->d_rows; p.ns = ds->n_stride; p.N = N; p.T = T; p.Ks = ds->Ks; p.D = ds->D;
    p.seed = (unsigned long long)seed;
    p.n_slots = W * 64; p.n_waves = W; p.n_regions = G;
    p.slot_site = slots.site; p.slot_w = slots.w; p.wave_first = slots.wave_first;
    const int rows_of[BL_TT_OUTPUTS] = {T, T - 1, T - 1, 1, T, T - 1, T - 1};
    for (int k = 0; k < BL_TT_OUTPUTS; k++) p.row_first[k + 1] = p.row_first[k] + (host[k] ? rows_of[k] : 0);
    const size_t rows = (size_t)p.row_first[BL_TT_OUTPUTS];
    if (!rows) return BL_OK; // (T = 1 and per-pair outputs alone: they are empty)
    DrawOut outs[BL_TT_OUTPUTS + 1];
    for (int k = 0; k < BL_TT_OUTPUTS; k++)
        outs[k] = DrawOut{host[k], (size_t)(p.row_first[k + 1] - p.row_first[k]) * G * 8, (void **)&p.out[k], false};
    outs[BL_TT_OUTPUTS] = DrawOut{nullptr, rows * W * 8, (void **)&p.part, true};
    return run_over_draws(ds, n_draws, draws, rows * std::max(W, G) * 8, outs, p, bl_launch_trajectory_totals);
}

// ---- species richness: per site the pmf of the number of species present and its expectation over the draws, per draw and region the
// weighted area holding exactly r species, fused ----
// (BUILDER-DEFINED, no counterpart in the reference.)  Kernels: species_richness.hip.  They read the site covariates at the head of ONE
// species' handle and the draws of all of them, stacked (run_over_draws' width: n_species D).  The area side's slots, workspace and
// chunking are bl_regional_totals'; the site side is one launch over all the draws when they are up, as bl_site_summary's, done before
// run_over_draws lets go of them.
extern "C" int bl_species_richness(bl_dataset *ds, int n_species, int n_draws, const float *draws, int n_regions, const int32_t *region,
                                   const double *weight, double *site_pmf, double *site_expected_mean, double *site_expected_sd,
                                   double *area_total)
{
    const bool site = site_pmf || site_expected_mean || site_expected_sd;
    int rc = per_draw_front("bl_species_richness", ds, n_draws, draws, (site || area_total) && (region || !area_total), serves_occu,
                            "occu, with or without false positives / random effects, one handle for all the species");
    if (rc) return rc;
    const int N = ds->dims.n_sites, S = n_species, G = n_regions;
    if (S < 1) return bl_fail(BL_ERR_INVALID, "bl_species_richness: n_species=%d, at least 1", S);
    if (S > BL_RICHNESS_MAX_SPECIES)
        return bl_fail(BL_ERR_UNSUPPORTED, "bl_species_richness: n_species=%d above BL_RICHNESS_MAX_SPECIES=%d", S, BL_RICHNESS_MAX_SPECIES);
    DevScratch scratch;
    RegionSlots slots;
    if (area_total && (rc = region_slots("bl_species_richness", N, G, region, weight, scratch, slots))) return rc;
    const int W = slots.n_waves;

    BlSpeciesRichnessParams p{};
    p.rows = ds->d_rows; p.ns = ds->n_stride; p.N = N; p.Ks = ds->Ks; p.D = ds->D; p.S = S; p.c = draw_coords(ds);
    p.n_draws = n_draws;
    p.n_slots = W * 64; p.n_waves = W; p.n_regions = G;
    p.slot_site = slots.site; p.slot_w = slots.w; p.wave_first = slots.wave_first;
    double *const host[3] = {site_pmf, site_expected_mean, site_expected_sd};
    double **const dev[3] = {&p.pmf, &p.mean, &p.sd};
    const size_t cells[3] = {(size_t)N * (S + 1), (size_t)N, (size_t)N};
    for (int k = 0; k < 3; k++)
        if (host[k]) BL_HIP(scratch.alloc((void **)dev[k], cells[k] * 8));
    const size_t rows = area_total ? (size_t)S + 1 : 0;
    const DrawOut outs[] = {{area_total, rows * G * 8, (void **)&p.area_total, false}, {nullptr, rows * W * 8, (void **)&p.part, true}};
    rc = run_over_draws(ds, n_draws, draws, rows * std::max(W, G) * 8, outs, [&](const float *d_draws, int n0, int n1, int grid_y) {
        p.draws = d_draws; p.n0 = n0; p.n1 = n1;
        int e = 0;
        if (site && n0 == 0) e = bl_launch_species_richness_site(&p, nullptr);
        if (!e && area_total) e = bl_launch_species_richness_area(&p, grid_y, nullptr);
        if (!e && n1 == n_draws) e = (int)hipStreamSynchronize(nullptr); // the site kernel reads all the draws
        return (hipError_t)e;
    }, (size_t)S * ds->D);
    if (rc) return rc;
    for (int k = 0; k < 3; k++)
        if (host[k]) BL_HIP(hipMemcpy(host[k], *dev[k], cells[k] * 8, hipMemcpyDeviceToHost));
    return BL_OK;
}

// ---- residual Moran: per draw and period Moran's I of the occupancy and detection residuals and of their replicates over a sparse
// neighbour graph, and the residuals' means per site, fused ----
// (BUILDER-DEFINED; the reference ships the residuals alone.)  Kernels: residual_moran.hip.  They read what bl_site_posterior reads (the
// sign-folded records: the observations and the masks) and what bl_predict reads (the raw observation covariates, up on first use);
// next to them goes up the graph.  The Moran side's workspace is 32 bytes per (draw of a chunk, period, site); run_over_draws cuts the
// draws so that it stays within its 256 MB.  The site side is one launch over all the draws when they are up, as bl_species_richness'.
static_assert(BL_RM_VAL_BYTES == 32, "bl_residual_moran's comment in the header states the record");
extern "C" int bl_residual_moran(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, uint64_t seed_rep, int32_t nnz,
                                 const int32_t *nbr_ptr, const int32_t *nbr_idx, const double *nbr_w, double *moran_occ, double *moran_det,
                                 int32_t *det_sites, double *occ_mean, double *det_mean, int32_t *n_occupied)
{
    const bool gather = moran_occ || moran_det, moran = gather || det_sites, site = occ_mean || det_mean || n_occupied;
    if (n_draws < 1) return bl_fail(BL_ERR_INVALID, "bl_residual_moran: n_draws=%d, at least 1", n_draws);
    int rc = per_draw_front("bl_residual_moran", ds, n_draws, draws, moran || site, serves_occu,
                            "occu, with or without false positives / random effects, one species a handle");
    if (rc) return rc;
    const int N = ds->dims.n_sites, T = ds->dims.n_periods, J = ds->dims.n_replicates;
    if (gather) {
        if (!nbr_ptr || (!nbr_idx && nnz > 0)) return bl_fail(BL_ERR_INVALID, "bl_residual_moran: Moran's I is wanted and the neighbour graph is NULL");
        if (nnz < 0) return bl_fail(BL_ERR_INVALID, "bl_residual_moran: nnz=%d is negative", (int)nnz);
        if (nbr_ptr[0] != 0) return bl_fail(BL_ERR_INVALID, "bl_residual_moran: nbr_ptr[0]=%d, not 0", (int)nbr_ptr[0]);
        for (int i = 0; i < N; i++)
            if (nbr_ptr[i + 1] < nbr_ptr[i])
                return bl_fail(BL_ERR_INVALID, "bl_residual_moran: nbr_ptr[%d]=%d below nbr_ptr[%d]=%d", i + 1, (int)nbr_ptr[i + 1], i, (int)nbr_ptr[i]);
        if (nbr_ptr[N] != nnz) return bl_fail(BL_ERR_INVALID, "bl_residual_moran: nbr_ptr[%d]=%d, not nnz=%d", N, (int)nbr_ptr[N], (int)nnz);
        for (int i = 0; i < N; i++)
            for (int e = nbr_ptr[i]; e < nbr_ptr[i + 1]; e++) {
                if (nbr_idx[e] < 0 || nbr_idx[e] >= N)
                    return bl_fail(BL_ERR_INVALID, "bl_residual_moran: nbr_idx[%d]=%d outside 0 .. N - 1 = %d", e, (int)nbr_idx[e], N - 1);
                if (nbr_idx[e] == i) return bl_fail(BL_ERR_INVALID, "bl_residual_moran: nbr_idx[%d]=%d is a self-loop of site %d", e, (int)nbr_idx[e], i);
                if (nbr_w && !std::isfinite(nbr_w[e])) return bl_fail(BL_ERR_INVALID, "bl_residual_moran: nbr_w[%d]=%g is not finite", e, nbr_w[e]);
            }
    }
    const size_t cells = (size_t)T * N; // per draw
    if (moran && cells * BL_RM_VAL_BYTES > BL_TOTALS_WORKSPACE_BYTES)
        return bl_fail(BL_ERR_UNSUPPORTED, "bl_residual_moran: %d periods x %d sites need more than the workspace's %u bytes a draw", T, N,
                       (unsigned)BL_TOTALS_WORKSPACE_BYTES);
    if ((rc = upload_once(&ds->d_wraw, ds->h_wraw))) return rc;

    BlResidualMoranParams p{};
    p.rows = ds->d_rows; p.wraw = ds->d_wraw; p.ns = ds->n_stride; p.N = N; p.T = T; p.J = J; p.Ks = ds->Ks; p.Ko = ds->Ko; p.D = ds->D;
    p.a = BlSitePostBlock{ds->KS, J, ds->model == 6 ? ds->re.Ko : ds->Ko, ds->KO + 1, ds->Ks + 1}; // (bl_site_posterior's)
    p.c = draw_coords(ds);
    p.seed = (unsigned long long)seed; p.seed_rep = (unsigned long long)seed_rep;
    p.n_draws = n_draws; p.n_waves = (N + 63) / 64;
    DevScratch scratch;
    if (gather) {
        int *d_ptr = nullptr, *d_idx = nullptr;
        double *d_w = nullptr;
        BL_HIP(scratch.alloc((void **)&d_ptr, ((size_t)N + 1) * 4));
        BL_HIP(hipMemcpy(d_ptr, nbr_ptr, ((size_t)N + 1) * 4, hipMemcpyHostToDevice));
        BL_HIP(scratch.alloc((void **)&d_idx, (size_t)nnz * 4));
        if (nnz) BL_HIP(hipMemcpy(d_idx, nbr_idx, (size_t)nnz * 4, hipMemcpyHostToDevice));
        if (nbr_w && nnz) {
            BL_HIP(scratch.alloc((void **)&d_w, (size_t)nnz * 8));
            BL_HIP(hipMemcpy(d_w, nbr_w, (size_t)nnz * 8, hipMemcpyHostToDevice));
        }
        p.nbr_ptr = d_ptr; p.nbr_idx = d_idx; p.nbr_w = d_w;
    }
    void *const host[3] = {occ_mean, det_mean, n_occupied};
    void **const dev[3] = {(void **)&p.occ_mean, (void **)&p.det_mean, (void **)&p.n_occupied};
    const size_t bytes[3] = {cells * 8, cells * 8, cells * 4};
    for (int k = 0; k < 3; k++)
        if (host[k]) BL_HIP(scratch.alloc(dev[k], bytes[k]));
    const size_t W = (size_t)p.n_waves, per = moran ? 1 : 0; // (no Moran output: no workspace)
    const DrawOut outs[] = {{moran_occ, (size_t)T * 16, (void **)&p.moran_occ, false},
                            {moran_det, (size_t)T * 16, (void **)&p.moran_det, false},
                            {det_sites, (size_t)T * 8, (void **)&p.det_sites, false},
                            {nullptr, per * cells * BL_RM_VAL_BYTES, (void **)&p.val, true},
                            {nullptr, per * T * W * BL_RM_FIELDS * 4 * 8, (void **)&p.part1, true},
                            {nullptr, per * T * BL_RM_FIELDS * 2 * 8, (void **)&p.stat, true},
                            {nullptr, (gather ? 1 : 0) * T * W * BL_RM_FIELDS * 3 * 8, (void **)&p.part3, true}};
    rc = run_over_draws(ds, n_draws, draws, std::max<size_t>(per * cells * BL_RM_VAL_BYTES, (size_t)T * 16), outs,
                        [&](const float *d_draws, int n0, int n1, int grid_y) {
        p.draws = d_draws; p.n0 = n0; p.n1 = n1;
        int e = 0;
        if (site && n0 == 0) e = bl_launch_residual_moran_site(&p, nullptr);
        if (!e && moran) e = bl_launch_residual_moran(&p, grid_y, nullptr);
        if (!e && n1 == n_draws) e = (int)hipStreamSynchronize(nullptr); // the site kernel reads all the draws
        return (hipError_t)e;
    });
    if (rc) return rc;
    for (int k = 0; k < 3; k++)
        if (host[k]) BL_HIP(hipMemcpy(host[k], *dev[k], bytes[k], hipMemcpyDeviceToHost));
    return BL_OK;
}

// ------------------------------------------------------- multi-GPU: the gather of the draws over RCCL ----
#include "comm_rccl.hpp"
