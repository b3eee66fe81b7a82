/*
 * biolith_hip.h -- C-ABI of the MI355X-native occupancy-model NUTS engine.
 *
 * This is the drop-in boundary for ONE path of timmh/biolith:
 *     biolith.utils.fit(biolith.models.occu, ...)          (biolith/utils/fit.py:16-135)
 * Everything numpyro/jax did behind `mcmc.run(...)` (fit.py:128-130) happens behind these
 * entry points in hand-written HIP for gfx950.  Plain pointers and sizes only; no torch / C++
 * types cross the boundary; no exception crosses it (int status + bl_last_error()).
 *
 * Ownership: the caller allocates every output.  bl_dataset_create copies its inputs; the
 * library keeps nothing of the caller's after any call returns, except its own opaque handle.
 * A handle is not thread-safe; use one host thread (or process) per handle.
 */
#ifndef BIOLITH_HIP_H
#define BIOLITH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BL_ABI_VERSION 1

enum {
    BL_OK = 0,
    BL_ERR_INVALID = 1,      /* bad argument / unsupported shape (message says which)       */
    BL_ERR_NO_DEVICE = 2,    /* no HIP device / HIP runtime error                            */
    BL_ERR_UNSUPPORTED = 3,  /* model option outside the built path                          */
    BL_ERR_TIMEOUT = 4,      /* in-kernel spin bound hit (a cooperating workgroup vanished)  */
    BL_ERR_ABORTED = 5,      /* bl_nuts_abort() was honoured                                 */
    BL_ERR_BUSY = 6,         /* a launch is still in flight on this handle                   */
    BL_ERR_COMM = 7          /* RCCL could not be loaded, or a communicator call failed      */
};

#define BL_RNG_STREAMS_PER_CHAIN 64
#define BL_MAX_COVS 16 /* per side (site / observation) */

/* Shapes as the reference names them (biolith/models/occu.py:116-133). */
typedef struct bl_dims {
    int32_t n_species;    /* S : the "species" plate (occu.py:182).  S > 1 = ONE chain over all species' coefficients:
                           *     bl_dataset_create / _fp (S (Ks + Ko + 2) (+ 1) <= 60 coordinates) and _re (S <= 8); the other
                           *     models take one species per handle                                                       */
    int32_t n_sites;      /* N                                                               */
    int32_t n_periods;    /* T : stacked periods sharing psi (occu.py:198-210)               */
    int32_t n_replicates; /* J : visits per period                                           */
    int32_t n_site_covs;  /* Ks                                                              */
    int32_t n_obs_covs;   /* Ko                                                              */
} bl_dims;

/* prior.expand([K+1]).to_event(1) with prior = Normal(loc, scale)
 * (biolith/regression/linear.py:28, defaults occu.py:28-29). */
typedef struct bl_normal_prior {
    double loc;
    double scale;
} bl_normal_prior;

typedef struct bl_dataset bl_dataset;

int bl_abi_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char *bl_last_error(void);
int bl_device_count(int *count);

/*
 * Replaces what numpyro traces out of occu() on first call (fit.py:128 -> occu.py:102-242):
 * validates shapes (occu.py:103-133), builds the missing-data mask (occu.py:136-142,
 * utils/modeling.py:15-17), NaN->0 on covariates, and lays the data out site-fastest in HBM.
 *   site_covs [N][Ks]  obs_covs [N][T][J][Ko]  obs [S][N][T][J]   (row-major float32, NaN = missing)
 * exactly the arrays prepare_data() produces (utils/data.py:135-140).
 */
int bl_dataset_create(const bl_dims *dims, const float *site_covs, const float *obs_covs,
                      const float *obs, const bl_normal_prior *prior_beta,
                      const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/*
 * Same for the Royle-Nichols model biolith.models.occu_rn (models/occu_rn.py:20-222): latent
 * abundance N ~ RightTruncatedPoisson(exp(beta0 + x beta), max_abundance) (utils/distributions.py:6-40)
 * summed out in the kernel, detection 1 - (1 - sigmoid(alpha0 + w alpha))^N.  Built for
 * max_abundance <= 127 (covariates: up to BL_MAX_COVS per side, as for every model).  The handle then behaves exactly like an
 * occu handle (bl_logp_grad, bl_nuts_*); bl_deterministic's first output becomes
 * `abundance` = exp(beta0 + x beta) (occu_rn.py:192).
 */
int bl_dataset_create_rn(const bl_dims *dims, const float *site_covs, const float *obs_covs,
                         const float *obs, int max_abundance, const bl_normal_prior *prior_beta,
                         const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/*
 * Dynamic (multi-season) occupancy -- BUILDER-DEFINED, NO REFERENCE COUNTERPART: BASELINE.json configs[4] names a model
 * timmh/biolith does not have (its periods share one psi, models/occu.py:198-210).  Initial occupancy psi, colonisation gamma and
 * extinction eps, each logit-linear in the site covariates; detection as in occu; the latent paths summed out by the forward
 * recursion in the kernel (csrc/dyn_device.hpp).  theta = [b_psi | b_gamma | b_eps (n_site_covs + 1 each) | alpha (n_obs_covs + 1)],
 * every coefficient under the Normal priors given (prior_beta for the three site-side blocks).  n_site_covs <= 8; one species.
 * The handle serves bl_logp_grad and bl_nuts_*; deterministic sites are formed by the caller from the draws.
 */
int bl_dataset_create_dyn(const bl_dims *dims, const float *site_covs, const float *obs_covs,
                          const float *obs, const bl_normal_prior *prior_beta,
                          const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/*
 * Same for occu with a false-positive rate (models/occu.py:146-157, 229-241):
 *   P(y=1 | z) = 1 - (1 - z p)(1 - f_c)(1 - (1 - z) f_u),  exactly one of f_c / f_u sampled:
 *   fp_mode BL_FP_CONSTANT   = false_positives_constant=True   (site "prob_fp_constant",   prior occu.py:32)
 *   fp_mode BL_FP_UNOCCUPIED = false_positives_unoccupied=True (site "prob_fp_unoccupied", prior occu.py:33)
 * prior_fp is the Beta(a, b) prior of that rate (NULL = Beta(2, 5), the reference default).  The handle's
 * parameter vector gains one trailing coordinate phi = logit(rate) (NumPyro's unconstrained space for
 * a unit-interval site), so bl_dataset_param_dim = Ks + Ko + 3 and draws[..., D-1] is phi.
 */
typedef struct { double a, b; } bl_beta_prior;
enum { BL_FP_CONSTANT = 1, BL_FP_UNOCCUPIED = 2 };
int bl_dataset_create_fp(const bl_dims *dims, const float *site_covs, const float *obs_covs,
                         const float *obs, int fp_mode, const bl_beta_prior *prior_fp,
                         const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha,
                         int device, bl_dataset **out);
/*
 * Same for the count occupancy model biolith.models.occu_cop (models/occu_cop.py:17-255):
 *   y_itj ~ Poisson(session_duration_itj * (z lambda_itj + (1 - z) f_u + f_c)),  lambda = exp(alpha0 + w alpha),
 * obs holds counts, session_duration [N][T][J] the exposure (occu_cop.py:176, 250-254).  fp_mode 0: no
 * false-positive rate; BL_FP_CONSTANT / BL_FP_UNOCCUPIED: sites "rate_fp_constant" / "rate_fp_unoccupied"
 * with an Exponential(prior_fp_rate) prior (occu_cop.py:31-32, 158-170) sampled as a trailing coordinate
 * phi = log(rate).  bl_deterministic's second output becomes `rate_detection` = exp(alpha0 + w alpha)
 * (occu_cop.py:236-243).  Predictive draws: bl_predict_counts.
 */
int bl_dataset_create_cop(const bl_dims *dims, const float *site_covs, const float *obs_covs,
                          const float *obs, const float *session_duration, int fp_mode,
                          double prior_fp_rate, const bl_normal_prior *prior_beta,
                          const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/*
 * Same for the N-mixture model biolith.models.nmixture (models/nmixture.py:17-220): obs holds counts,
 * N ~ Poisson(exp(beta0 + x beta)) enumerated over 0..max_abundance (raw, un-renormalised weights: the model's
 * "N_i_trunc_norm" factor, nmixture.py:183-196; support cut below the largest count of each (site, period),
 * nmixture.py:150-155), y ~ Binomial(N, sigmoid(alpha0 + w alpha)).  bl_deterministic's outputs are `abundance`
 * and `prob_detection`.  Built for max_abundance <= 127; predictive draws: bl_predict_counts.
 */
int bl_dataset_create_nmix(const bl_dims *dims, const float *site_covs, const float *obs_covs,
                           const float *obs, int max_abundance, const bl_normal_prior *prior_beta,
                           const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/*
 * Same for biolith.models.occu with site_random_effects / obs_random_effects (models/occu.py:36-39, 170-173, 191-196,
 * 215-218): site_re_sd, obs_re_sd ~ HalfNormal(scale) sampled before the plates; per site site_re_occ, site_re_det ~
 * Normal(0, site_re_sd) join the occupancy and detection predictors; per replicate obs_re ~ Normal(0, obs_re_sd) joins
 * the detection predictor (masked replicates keep their prior term).  Coordinates, in NumPyro's
 * unconstrained space:  theta = [beta, alpha, (log site_re_sd), (log obs_re_sd), (site_re_occ[N], site_re_det[N]),
 * (obs_re[N][T][J])], D = bl_dataset_param_dim().  Several species (dims->n_species <= 8, obs [S][N][T][J]) are ONE chain, as in
 * the reference: beta, alpha and the effects sit inside the species plate (occu.py:182-196), the two sds outside it
 * (occu.py:170-173), i.e. shared:  theta = [species 0: beta, alpha | species 1: ... | (log site_re_sd) | (log obs_re_sd) |
 * site_re_occ [S][N] | site_re_det [S][N] | obs_re [S][N][T][J]]; a chain then runs on a multiple of S workgroups, each
 * slicing the sites of one species; bl_deterministic / bl_predict take one-species handles (cut the draws per species).
 * bl_logp_grad / bl_nuts_* work as for the other models (the sampler
 * runs k workgroups per chain -- site slices, partial sums exchanged through device memory; all num_chains x k must be
 * resident, so num_chains x k <= compute units -- with its vectors in device memory / LDS; RNG: one stream per coordinate, D + 2 per chain;
 * with D <= 61 the layout of the other models: 64 per chain, the two scalar streams last).
 * At most 16 covariates per side.  bl_deterministic adds the effects to both predictors; bl_predict draws z and y from them.
 */
int bl_dataset_create_re(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                         int site_random_effects, int obs_random_effects, double prior_site_re_sd_scale,
                         double prior_obs_re_sd_scale, const bl_normal_prior *prior_beta,
                         const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/* The same with a false-positive rate on top (occu.py:146-157 together with :170-173, 191-196; fp_mode / prior_fp as for
 * bl_dataset_create_fp): theta = [beta, alpha, phi = logit(rate), (log sds), (effects)].  One species per dataset. */
int bl_dataset_create_re_fp(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                            int site_random_effects, int obs_random_effects, double prior_site_re_sd_scale,
                            double prior_obs_re_sd_scale, int fp_mode, const bl_beta_prior *prior_fp,
                            const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/* The N-mixture model with the same random effects (biolith/models/nmixture.py:139-141, 166-172, 199-214: site_re_abu joins the
 * abundance predictor, site_re_det and obs_re the detection predictor): `counts` / max_abundance as for bl_dataset_create_nmix,
 * theta = [beta, alpha, (log site_re_sd), (log obs_re_sd), (site_re_abu[N], site_re_det[N]), (obs_re[N][T][J])].  One species
 * per dataset.  bl_logp_grad / bl_nuts_* as above; bl_deterministic returns abundance = exp(eta + site_re_abu) and the
 * detection probability with its effects; bl_predict_counts draws N and the counts from them. */
int bl_dataset_create_nmix_re(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *counts,
                              int max_abundance, int site_random_effects, int obs_random_effects,
                              double prior_site_re_sd_scale, double prior_obs_re_sd_scale, const bl_normal_prior *prior_beta,
                              const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/* The Royle-Nichols model with the same random effects (biolith/models/occu_rn.py:151-154, 172-184, 199-212): `obs` / max_abundance
 * as for bl_dataset_create_rn, theta laid out as for bl_dataset_create_nmix_re.  One species per dataset.  bl_deterministic returns
 * abundance = exp(eta + site_re_abu) and the detection probability with its effects; bl_predict draws N and y from them. */
int bl_dataset_create_rn_re(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                            int max_abundance, int site_random_effects, int obs_random_effects,
                            double prior_site_re_sd_scale, double prior_obs_re_sd_scale, const bl_normal_prior *prior_beta,
                            const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/* ... and with a false-positive rate (occu_rn.py:133-138, 214-221: y ~ Bernoulli(1 - (1 - p)(1 - f)), f ~ Beta(a, b)), with or without the
 * random effects: theta = [beta, alpha, phi = logit f, (log sds), (effects)].  One species.  Runs on the random-effects kernels in
 * either case; bl_deterministic / bl_predict apply the effects and the rate. */
int bl_dataset_create_rn_fp(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *obs,
                            int max_abundance, int site_random_effects, int obs_random_effects,
                            double prior_site_re_sd_scale, double prior_obs_re_sd_scale, const bl_beta_prior *prior_fp,
                            const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/* occu_cop with the same random effects (biolith/models/occu_cop.py:183-186, 204-210, 229-243: site_re_occ joins the occupancy
 * predictor, site_re_det and obs_re the log detection rate), with or without a false-positive rate (occu_cop.py:158-170, 244-248):
 * `counts` / `session_duration` / fp_mode / prior_fp_rate as for bl_dataset_create_cop, theta = [beta, alpha, (phi = log rate_fp),
 * (log sds), (effects)].  One species.  bl_deterministic returns psi and rate_detection with the effects; bl_predict_counts draws z
 * and the counts from them. */
int bl_dataset_create_cop_re(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *counts,
                             const float *session_duration, int fp_mode, double prior_fp_rate, int site_random_effects,
                             int obs_random_effects, double prior_site_re_sd_scale, double prior_obs_re_sd_scale,
                             const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/*
 * The continuous-score occupancy model biolith.models.occu_cs (models/occu_cs.py:17-232; Rhinehart et al. 2022): `scores`
 * [S=1][N][T][J] (NaN = missing) ~ Normal(mu_f, sigma_f) with f ~ Bernoulli(z p) and z ~ Bernoulli(psi) summed out.
 * prior_mu = {loc, scale of mu0; loc, scale of the Normal that mu1 follows truncated below at mu0}; prior_sigma =
 * {concentration, rate of sigma0's Gamma; of sigma1's}.  theta = [beta, alpha, mu0, log(mu1 - mu0), log sigma0, log sigma1]
 * (NumPyro's unconstrained space), D = Ks + Ko + 6.  Runs on the random-effects kernels' framework (bl_dataset_create_re);
 * bl_deterministic gives psi and prob_detection; predictive draws: bl_predict_scores.
 */
int bl_dataset_create_cs(const bl_dims *dims, const float *site_covs, const float *obs_covs, const float *scores,
                         const double *prior_mu, const double *prior_sigma, const bl_normal_prior *prior_beta,
                         const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/*
 * The combined point-count / ARU / score occupancy model biolith.models.occu_comb (models/occu_comb.py:19-349), one species
 * per handle.  Per (site, period) one enumerated z ~ Bernoulli(psi) is shared by three blocks of replicates:
 *   point counts  pc_obs [N][T][Jpc]     y ~ Bernoulli(z p_pc)                       (no false positives),
 *   ARU           aru_obs [N][T][Jaru]   y ~ Bernoulli(1 - (1 - z p_aru)(1 - fc)(1 - (1 - z) fu)),
 *   scores        scores [N][T][Js]      s ~ Normal(z ? mu1 : mu0, z ? sigma1 : sigma0),
 * p_pc = sigmoid(alpha_PC . (1, pc_covs [N][T][Jpc][Kpc])), p_aru likewise with aru_covs [N][T][Jaru][Karu].  NaN = missing: a
 * visit is masked where its y, any of its block's covariates or any site covariate is NaN; a score where it or a site covariate is.
 * Every Bernoulli probability is clamped to [tiny, 1 - eps] as NumPyro clamps it (a point-count detection at z = 0 costs log tiny).
 * theta (NumPyro's unconstrained space), D = (Ks + 1) + (Kpc + 1) + (Karu + 1) + 6:
 *   [beta (Ks+1) | alpha_PC (Kpc+1) | alpha_ARU (Karu+1) | logit fc | logit fu | mu0 | log(mu1 - mu0) | log sigma0 | log sigma1]
 * with fc ~ Beta(prior_fc), fu ~ Beta(prior_fu), mu0 ~ Normal(prior_mu[0..1]), mu1 ~ Normal(prior_mu[2..3]) truncated below at mu0,
 * sigma_f ~ Gamma(prior_sigma[2f], prior_sigma[2f+1]); beta ~ prior_beta, both alphas ~ prior_alpha (bl_dataset_set_prior_family
 * applies).  At most 16 covariates per block.  bl_logp_grad and bl_nuts_* serve the handle (the random-effects kernels' framework);
 * bl_deterministic / bl_predict* do not (the fit's sites are formed by the caller from the draws); the model's own entries are
 * bl_deterministic_comb and bl_predict_comb.
 */
typedef struct bl_comb_dims {
    int32_t n_sites, n_periods;           /* N, T                                          */
    int32_t n_pc, n_aru, n_scores;        /* Jpc, Jaru, Js: replicates of each block       */
    int32_t n_site_covs, n_pc_covs, n_aru_covs; /* Ks, Kpc, Karu                            */
} bl_comb_dims;
int bl_dataset_create_comb(const bl_comb_dims *dims, const float *site_covs, const float *pc_covs, const float *pc_obs,
                           const float *aru_covs, const float *aru_obs, const float *scores, const bl_beta_prior *prior_fc,
                           const bl_beta_prior *prior_fu, const double *prior_mu, const double *prior_sigma,
                           const bl_normal_prior *prior_beta, const bl_normal_prior *prior_alpha, int device, bl_dataset **out);
/*
 * The other prior family biolith.utils.grid_search_priors tries for the regression coefficients
 * (utils/grid_search.py:366-371): Laplace(loc, scale) instead of Normal(loc, scale), per side, with the (loc, scale) the
 * dataset was created with.  Call between bl_dataset_create* and the first use; applies to every model.
 */
#define BL_PRIOR_NORMAL 0
#define BL_PRIOR_LAPLACE 1
int bl_dataset_set_prior_family(bl_dataset *ds, int family_beta, int family_alpha);
int bl_dataset_destroy(bl_dataset *ds);
/* Coordinates of theta.  occu / occu_rn / nmixture / occu_cop without a rate: D = Ks+1 + Ko+1, theta = [beta_0..beta_Ks,
 * alpha_0..alpha_Ko]; with a false-positive coordinate (bl_dataset_create_fp, occu_cop with a rate): + 1 (trailing phi);
 * S species under one chain: S (Ks + Ko + 2) (+ 1); dynamic occupancy: 3 (Ks + 1) + Ko + 1; occu_cs: Ks + Ko + 6; occu_comb: Ks + Kpc + Karu + 9; random
 * effects: Ks + Ko + 2 + the log sds + 2 N (site effects) + N T J (observation effects), per species where S > 1. */
int bl_dataset_param_dim(const bl_dataset *ds, int *D);

/*
 * Parity hook for the likelihood kernel: U = -log p(theta, y) (z marginalised, Normal prior
 * normaliser included) and dU/dtheta for B parameter vectors.  Replaces
 * jax.value_and_grad(potential_fn) over occu.py:136-242 + funsor enumeration (occu.py:208-210).
 * `staged` != 0 evaluates through the same LDS-staged code path the NUTS kernel uses.
 */
int bl_logp_grad(bl_dataset *ds, int B, const double *theta /*[B][D]*/, double *U /*[B]*/,
                 double *grad /*[B][D]*/, int staged);

/* MCMC(NUTS(model), num_samples, num_warmup, num_chains).run(PRNGKey(seed))  (fit.py:92-130) */
typedef struct bl_nuts_config {
    int32_t num_warmup;     /* fit.py:23 default 1000 */
    int32_t num_samples;    /* fit.py:22 default 1000 */
    int32_t num_chains;     /* chains run by THIS call (fit.py:25 default 5)                 */
    int32_t chain_offset;   /* global id of this call's first chain: selects its RNG streams */
    uint64_t seed;          /* fit.py:24 / fit.py:122                                       */
    int32_t max_tree_depth; /* numpyro NUTS default 10                                       */
    int32_t wgs_per_chain;  /* 0 = auto; workgroups (CUs) cooperating on one chain           */
    double target_accept;   /* numpyro NUTS default 0.8                                      */
    const double *init_theta; /* NULL = init_to_uniform(radius 2) (fit.py:93); else [C][D]  */
} bl_nuts_config;

/* Host pointers, caller-allocated; NULL = not wanted.  C = num_chains, S = num_samples. */
typedef struct bl_nuts_output {
    float *draws;            /* [C][S][D] post-warmup positions (mcmc.get_samples, fit.py:132) */
    uint8_t *diverging;      /* [C][S]   extra field "diverging" (diagnostics.py:34-38)        */
    int32_t *num_steps;      /* [C][S]   leapfrogs of each transition                          */
    float *accept_prob;      /* [C][S]                                                          */
    float *potential_energy; /* [C][S]                                                          */
    float *step_size;        /* [C]      adapted step size                                      */
    float *inv_mass;         /* [C][D]   adapted diagonal inverse mass                          */
    int64_t *n_leapfrog;     /* [C][2]   gradient evaluations: warmup, sampling                 */
} bl_nuts_output;

/* Blocking convenience: launch + wait + fetch. */
int bl_nuts_run(bl_dataset *ds, const bl_nuts_config *cfg, bl_nuts_output *out);

/* Asynchronous form (timeouts, overlap, timing).  `stream` is a hipStream_t or NULL.
 * The kernel is persistent and its workgroups exchange data while they run, so all of them must be resident
 * at once: launches on ONE device belong on one stream (they then run back to back), launches on different
 * devices overlap freely.  If the device is shared and a workgroup cannot become resident, the bounded spins
 * expire and bl_nuts_wait returns BL_ERR_TIMEOUT instead of hanging. */
int bl_nuts_launch(bl_dataset *ds, const bl_nuts_config *cfg, void *stream);
int bl_nuts_poll(bl_dataset *ds, int *done);
int bl_nuts_abort(bl_dataset *ds); /* fit(timeout=...) (fit.py:124-128): kernel exits at its next leapfrog */
int bl_nuts_wait(bl_dataset *ds);  /* returns BL_ERR_TIMEOUT / BL_ERR_ABORTED if the kernel reported it */
int bl_nuts_fetch(bl_dataset *ds, bl_nuts_output *out);
/* HIP-event time of the last launch (kernel + its memset), on the launch stream. */
int bl_nuts_elapsed_ms(bl_dataset *ds, float *ms);
/* Device address of the last launch's draws [C][S][D] float32 (for an RCCL gather). */
int bl_nuts_device_draws(bl_dataset *ds, void **dev_ptr, size_t *bytes);
/* Geometry the last launch used; the last field counts the chains whose workgroups were verified
 * (HW_REG_XCC_ID census) to share one XCD and therefore ran the L2-local exchange.  lds_staged: bit 0 = the
 * site data were staged in LDS; random-effects / occu_cs launches: bits 1-2 = how many of the sampler's
 * vectors lived in LDS (0 none, 1 the five of the leaf in flight, 2 every vector a leapfrog touches). */
int bl_nuts_geometry(bl_dataset *ds, int *wgs_per_chain, int *threads_per_wg, int *lds_bytes, int *lds_staged,
                     int *chains_on_l2_local_exchange);
/* Bytes of one workgroup's exchange record in the last finished launch: 64 = the compact records of the lean plain-model kernels
 * (8 granules, the ninth value and the rare words in the tags' spare bits), 128 / 256 / 512 = 16 / 32 / 64 granules of 8 bytes. */
int bl_nuts_record_bytes(bl_dataset *ds, int *record_bytes);

/* Lanes that shared one site pair in the last launch (1, 1 = one pair per lane): period_lanes split the pair's periods, visit_lanes
 * the visits of a period -- the layout SURVEY.md 7.1 asks for when a site has many visits (simulate() defaults: 52 per site,
 * biolith/models/occu.py:251-252, 336; benchmarks/occu_spoccupancy.py:16-70: up to 90).  Environment knobs for tests and A/B
 * runs: BIOLITH_HIP_OCCU_G = 1 | 2 | 4 | 8 | 16 forces the lanes per pair, BIOLITH_HIP_OCCU_GT the log2 of the period lanes. */
int bl_nuts_lane_group(bl_dataset *ds, int *period_lanes, int *visit_lanes);

/* Name of the sampler instantiation the last launch ran, as a profiler prints it (e.g. "bl_nuts_kernel<3, 3, true, 0, 3, false, 5, true>":
 * capacities, LDS-staged, model, compute waves, lane-group form, visits-per-period form, lean form; or, for the random-effects models,
 * "bl_re_nuts_kernel<4, 0, true, 2, 5>": covariate capacity, model kind, rows in LDS, sampler-vector tier in LDS, effects / one period as
 * compile-time facts).  Measurement only: bench.py's roofline.kernel. */
int bl_nuts_kernel_name(bl_dataset *ds, char *buf, int n);

/* The BIOLITH_HIP_* environment knobs (tests, A/B runs, measurement; INTEGRATION.md lists every one) that were SET when the last
 * launch on this handle read the environment, as "NAME=value,NAME=value" ("" = none: the geometry and the kernel form are the
 * engine's own choice).  The launch path reads the environment in one place, once per launch.  bl_env_overrides: the same for the
 * environment as it is now (no handle).  Not part of the reference's interface (numpyro has no such knobs); bench.py prints it so
 * that a stray variable cannot change a measured geometry silently. */
int bl_nuts_env_overrides(bl_dataset *ds, char *buf, int n);
int bl_env_overrides(char *buf, int n);

/* Page-locked host memory for large outputs (bl_deterministic / bl_predict write into caller memory; into page-locked memory the
 * device copies at PCIe rate instead of staging through the runtime's bounce buffers).  The caller owns and frees it.  The
 * reference's counterpart is jax.device_get() of a deterministic site (utils/fit.py:132). */
int bl_host_alloc(size_t bytes, void **out);
int bl_host_free(void *ptr);

/* In-kernel phase cycle counters of the last launch; all zero unless the library is a diagnostic
 * BL_STAMPS build (make -C biolith_amd/csrc stamps).  Not part of the reference's interface. */
int bl_nuts_debug_counters(bl_dataset *ds, int64_t *out /*[n<=560]*/, int n);

/*
 * Deterministic sites (occu.py:207, 221-228), recomputed from draws on the device:
 *   psi            [n_draws][T][N]      = sigmoid(beta_0 + X beta)       (constant over T)
 *   prob_detection [n_draws][J][T][N]   = sigmoid(alpha_0 + W alpha)
 * draws is [n_draws][D] float32 on the host; outputs are host float32 (NULL = skip).
 */
int bl_deterministic(bl_dataset *ds, int n_draws, const float *draws, float *psi, float *prob_detection);

/*
 * The summary of the deterministic sites over the posterior draws, fused -- BUILDER-DEFINED (the reference's users reduce predict()'s
 * arrays on the host): per cell of bl_deterministic's two sites, over all n_draws draws, without the arrays [n_draws][T][N] and
 * [n_draws][J][T][N] ever being stored.  With v_0 .. v_{n-1} the cell's float32 values of bl_deterministic, bit for bit, in draw order:
 *   mean   = (sum_n v_n) / n_draws, summed in float64 in draw order
 *   sd     = sqrt(sum_n (v_n - mean)^2 / (n_draws - 1)), float64, in draw order; NaN for n_draws == 1
 *   order  [r] = the float32 value of rank ranks[r] (0 = the smallest) in the sorted order of the cell's values, bit for bit
 * The first site (psi; occu_rn, nmixture: abundance) is constant over the periods and comes back per site: psi_mean, psi_sd [N],
 * psi_order [n_ranks][N].  The second (prob_detection; occu_cop: rate_detection): prob_mean, prob_sd [J][T][N], prob_order
 * [n_ranks][J][T][N].  float64 / float32 on the host, NULL = skip (all six NULL: BL_ERR_INVALID); the kernel of a site none of whose
 * outputs is wanted is not launched, and a skipped output never changes another.  ranks holds n_ranks values in 0 .. n_draws - 1, in any
 * order, duplicates allowed; it is read only if an order output is wanted (then n_ranks <= 0 or a rank outside the range:
 * BL_ERR_INVALID; n_ranks > BL_SUMMARY_MAX_RANKS: BL_ERR_UNSUPPORTED, the message names the cap).  n_draws itself is not limited.
 * Both sites are >= 0 (a sigmoid or an exponential), so the order statistics are selected on the unsigned bit pattern of the values; a
 * NaN value has no place in that order: NaN draws are not served (the caller keeps non-finite draws out; what comes back for a cell
 * that met one is unspecified).  Every sum runs in a fixed order, no atomics: a cell's outputs are a function of its covariates, its
 * effects and the draws alone, and two calls return the same bits.  Serves what bl_deterministic serves, with its refusals
 * (BL_ERR_UNSUPPORTED: a joint-species handle, occu_dyn, occu_comb; BL_ERR_BUSY while a NUTS launch is in flight on the handle).
 */
#define BL_SUMMARY_MAX_RANKS 16
int bl_site_summary(bl_dataset *ds, int n_draws, const float *draws, int n_ranks, const int32_t *ranks, double *psi_mean, double *psi_sd,
                    float *psi_order, double *prob_mean, double *prob_sd, float *prob_order);

/*
 * The convergence diagnostics of the deterministic sites, fused -- BUILDER-DEFINED (the reference's users run
 * numpyro.diagnostics.summary over predict()'s arrays on the host): per cell of bl_deterministic's two sites, the effective sample size
 * and the split R-hat over the draws of n_chains chains, without the arrays [n_draws][T][N] and [n_draws][J][T][N] ever being stored.
 * draws is chain-major: with n = n_draws / n_chains, chain c owns draws c n .. c n + n - 1.  With x[c][t] the cell's float32 value of
 * bl_deterministic under draw c n + t, bit for bit, widened to float64, and C = n_chains -- numpyro's estimator:
 *   m_c     = (sum_t x[c][t]) / n;   s2_c = sum_t (x[c][t] - m_c)^2 / (n - 1)
 *   W       = (sum_c s2_c) / C;   plus = W (n - 1) / n;   C > 1: plus += sum_c (m_c - mean_c m_c)^2 / (C - 1);   C == 1: W = plus
 *   gamma_k = (sum_c sum_{t < n - k} (x[c][t] - m_c)(x[c][t + k] - m_c)) / C / n
 *   rho_k   = 1 - (W - gamma_k) / plus,  rho_0 = 1;   P_p = rho_{2p} + rho_{2p+1} for p < n / 2 (an odd last lag is dropped)
 *   tau     = -1 + 2 (P_0 + sum_{p >= 1} min_{1 <= q <= p} max(P_q, 0));   n_eff = C n / tau
 *   r_hat   = sqrt(plus' / W'), plus' and W' as above over the 2 C half chains x[c][0 .. h - 1] and x[c][n - h .. n - 1], h = n / 2
 *   mean, sd: bl_site_summary's, over all C n draws in draw order
 * P_0 is not clipped; for very short chains tau, and with it n_eff, may be negative.  A cell whose values are all equal has 0 / 0 in
 * rho and in r_hat: NaN for both; r_hat is NaN where a half holds one draw (n < 4).  Every sum runs in float64 in draw order, chain after
 * chain; the lagged sums are formed directly, a block of lags a pass over the chains.  Once a clipped pair is 0 every later term of tau
 * is +0, so a cell stops there, exactly; how many passes its neighbours take changes nothing.  No atomics: a cell's outputs are a
 * function of its covariates, its effects and the draws alone -- not of N, of the other outputs asked for or of the launch --, and two
 * calls return the same bits.
 * The first site (psi; occu_rn, nmixture: abundance) is constant over the periods and comes back per site, [N]; the second
 * (prob_detection; occu_cop: rate_detection) [J][T][N].  float64 on the host, NULL = skip (all eight NULL: BL_ERR_INVALID); the kernel
 * of a site none of whose outputs is wanted is not launched.  n_chains < 1, n_draws not divisible by n_chains, or fewer than 2 draws per
 * chain: BL_ERR_INVALID.  Draws must be finite.  Device workspace: three float64 per chain and cell; nothing grows with n.  Serves what
 * bl_site_summary serves, with its refusals (BL_ERR_UNSUPPORTED: a joint-species handle, occu_dyn, occu_comb; BL_ERR_BUSY while a NUTS
 * launch is in flight on the handle).
 */
int bl_site_diagnostics(bl_dataset *ds, int n_draws, const float *draws, int n_chains, double *psi_n_eff, double *psi_r_hat,
                        double *psi_mean, double *psi_sd, double *prob_n_eff, double *prob_r_hat, double *prob_mean, double *prob_sd);

/*
 * The posterior of totals over sets of sites, fused -- BUILDER-DEFINED (the reference's users form predict()'s arrays and sum them on
 * the host): per posterior draw and region, the weighted total of the first deterministic site and of the latent state, without the
 * arrays [n_draws][T][N] ever being stored.  region[i] in 0 .. n_regions - 1 is site i's region, -1 = in no region; weight[i] is finite
 * and may be zero or negative, NULL = 1.  With v_i(n) bl_deterministic's float32 value of the first site (psi; occu_rn, nmixture:
 * abundance; it is constant over the periods) and z_{t,i}(n) the latent state bl_predict / bl_predict_counts / bl_predict_scores draw
 * for the same seed (z; occu_rn, nmixture: N_i), both bit for bit:
 *   site_total  [n][g]    = sum_{i in g} weight_i * (double) v_i(n)           [n_draws][n_regions]
 *   latent_total[n][t][g] = sum_{i in g} weight_i * (double) z_{t,i}(n)       [n_draws][T][n_regions]
 * float64 on the host, NULL = skip (both NULL: BL_ERR_INVALID); a skipped output never changes the other one, and with latent_total
 * NULL no generator is touched.  A region without a site comes back 0.
 * Order.  Every product is formed in float64 and the sums run in float64 in one fixed order, no atomics: region g's sites in site order
 * are cut into runs of 64, the last run filled up with -0.0 (the identity of the sum: a region of one site returns its term's bits); a
 * run is summed as the tree (x_l + x_{l+32}), then lanes 16, 8, 4, 2, 1 apart, and the runs' sums are added in run order.  Row g is
 * therefore a function of region g's own sites in site order, their weights and the draws: it is the same bytes when the other sites
 * are relabelled, merged into other regions or left out with -1, however the draws are chunked, and two calls return the same bytes.
 * Workspace.  The device holds one double per (draw of a chunk, output row, run of 64) and per (draw of a chunk, output row, region),
 * 1 + T output rows a draw; the draws go through in chunks such that each of the two is at most BL_TOTALS_WORKSPACE_BYTES -- or one
 * draw's rows, should they alone be larger --, whatever n_draws is.  Next to it: the draws, and 16 bytes per run's 64 slots.  The padded
 * runs cost at most 63 idle lanes per region: one region per site is served, at one wave of 64 lanes per site, which is wasteful.
 * region or weight refused (BL_ERR_INVALID; the message holds the offending value): a label outside -1 .. n_regions - 1, a non-finite
 * weight; also n_regions < 1.  Both outputs are untouched on any refusal.  Serves what bl_predict, bl_predict_counts and
 * bl_predict_scores serve together -- occu, occu_cs, occu_cop, occu_rn, nmixture, with or without a false-positive rate / random
 * effects --; occu_comb, occu_dyn and a joint-species handle: BL_ERR_UNSUPPORTED, the message names the model.  BL_ERR_BUSY while a NUTS
 * launch is in flight on the handle.
 */
#define BL_TOTALS_WORKSPACE_BYTES (256u << 20)
int bl_regional_totals(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, int n_regions, const int32_t *region,
                       const double *weight, double *site_total, double *latent_total);

/*
 * The posterior of a covariate's average response curve (partial dependence, marginal standardisation), fused -- BUILDER-DEFINED (the
 * reference's users copy the data once per grid value, form predict()'s arrays and average them on the host): per posterior draw and
 * grid value, the weighted total over the sites of a deterministic site with ONE covariate set to the grid value at every site -- every
 * other covariate and every effect left as the site has it --, without an array [n_draws][n_values][N] ever being stored.  side 0
 * replaces site covariate `covariate` in 0 .. Ks - 1, side 1 observation covariate `covariate` in 0 .. Ko - 1 at every visit; the
 * replacement applies at every site, one whose own value was NaN included.  values holds n_values finite float32; weight[i] is finite
 * and may be zero or negative, NULL = 1.
 *   side 0:  v_i^(g)(n) = the float32 bl_deterministic gives for the first site (psi; occu_rn, nmixture: abundance) on the handle whose
 *            site covariate `covariate` is values[g] at every site, bit for bit
 *              curve_total[n][g] = sum_i weight_i * (double) v_i^(g)(n)
 *   side 1:  u_{v,i}^(g)(n) = the float32 bl_deterministic gives for the second site (prob_detection; occu_cop: rate_detection) at visit
 *            v = t J + j on the handle whose observation covariate `covariate` is values[g] at every visit, bit for bit
 *              s_i = sum_{v = 0 .. T J - 1} (double) u_{v,i}^(g)(n), float64 in ascending v, from the first term on
 *              curve_total[n][g] = sum_i weight_i * s_i
 *            Every cell counts, as bl_deterministic returns every cell.
 * curve_total is [n_draws][n_values] float64 on the host.
 * Order.  bl_regional_totals' for a single region: every product is formed in float64 and the sums run in float64 in one fixed order, no
 * atomics: the sites in site order are cut into runs of 64, the last run filled up with -0.0 (a single site returns its term's bits); a
 * run is summed as the tree (x_l + x_{l+32}), then lanes 16, 8, 4, 2, 1 apart, and the runs' sums are added in run order.  So side 0's
 * column g is, byte for byte, bl_regional_totals' site_total for one region on the modified handle.  Column g is a function of the
 * sites, the weights, the draws and values[g] alone: it is the same bytes whatever the other values and their number are, however the
 * draws are chunked, and two calls return the same bytes.
 * Workspace.  The device holds one double per (draw of a chunk, value, run of 64); the draws go through in chunks such that it is at
 * most BL_TOTALS_WORKSPACE_BYTES -- or one draw's rows, should they alone be larger --, whatever n_draws is.  Next to it: the draws, the
 * values and the weights.
 * Refused with BL_ERR_INVALID, the message holding the offending value: side not 0 or 1; covariate outside 0 .. Ks - 1 (side 1:
 * 0 .. Ko - 1), which is every covariate on a side without covariates; n_values < 1; a non-finite value or weight; values or
 * curve_total NULL.  curve_total is untouched on any refusal.  Serves what bl_regional_totals serves -- occu, occu_cs, occu_cop, occu_rn,
 * nmixture, with or without a false-positive rate / random effects --; occu_comb, occu_dyn and a joint-species handle:
 * BL_ERR_UNSUPPORTED, the message names the model.  BL_ERR_BUSY while a NUTS launch is in flight on the handle.
 */
int bl_response_curves(bl_dataset *ds, int n_draws, const float *draws, int side /* 0 site, 1 obs */, int covariate,
                       int n_values, const float *values, const double *weight /* [N], NULL = 1 */,
                       double *curve_total /* [n_draws][n_values] */);

/*
 * The posterior of the occupancy trajectory's totals over sets of sites, fused -- BUILDER-DEFINED, like the model (bl_dataset_create_dyn):
 * per posterior draw of an occu_dyn handle and region, the weighted totals of the occupancy over n_periods seasons WITHOUT the
 * observations (bl_path_posterior gives the path given them), without an array [n_draws][n_periods][N] ever being stored.  The kernel
 * reads the site covariates at the head of the handle's rows and no visit; n_periods = T is an argument of the call, not the handle's:
 * the model is homogeneous in time, so a T beyond the fitted seasons is the forecast.  region, weight and n_regions are
 * bl_regional_totals'.  A draw is [b_psi | b_col | b_ext (Ks + 1 each) | alpha], as the sampler lays it out.  Per draw n and site i, in
 * float64 throughout (covariates, NaN -> 0, and coefficients are promoted from float32):
 *   eta      = fma(x_K, b_K, .. fma(x_1, b_1, b_0)) in covariate order, the intercept first, for each of psi, gamma (colonisation), eps
 *   rates    e = exp(-|eta|), r = 1 / (1 + e), s = e r; (sigma(eta), sigma(-eta)) = eta > 0 ? (r, s) : (s, r): a rate and its complement
 *            each come from the sigmoid, no complement is formed as 1 - x
 *   pi_0 = psi, q_0 = 1 - psi;   col_t = q_t gamma, ext_t = pi_t eps;   pi_t+1 = fma(pi_t, 1 - eps, col_t), q_t+1 = fma(q_t, 1 - gamma, ext_t)
 *   the path: cell (n, t, i) takes the first uniform u of the generator of cell (n, t of T, i of N) -- csrc/pred_rng.hpp, n the absolute
 *            draw index, i the site's own index --: z_0 = (double)u < psi, z_t+1 = (double)u < (z_t ? 1 - eps : gamma)
 * and the outputs, float64 on the host, each a sum over the sites of region g of weight_i times
 *   occupancy    [n][T][g]      pi_t                          z            [n][T][g]      z_t
 *   colonised    [n][T - 1][g]  col_t                         z_colonised  [n][T - 1][g]  [z_t = 0, z_t+1 = 1]
 *   extinct      [n][T - 1][g]  ext_t                         z_extinct    [n][T - 1][g]  [z_t = 1, z_t+1 = 0]
 *   equilibrium  [n][g]         gamma / (gamma + eps)
 * NULL = skip (all seven NULL: BL_ERR_INVALID); a skipped output never changes another, with the three z outputs NULL no generator is
 * touched, and with T = 1 the per-pair outputs are empty and left alone.  A region without a site comes back 0.  The first T rows of
 * occupancy, colonised and extinct do not depend on n_periods; the path does (the cell's index holds T).
 * Order and workspace are bl_regional_totals': every product in float64, region g's sites in site order cut into runs of 64, the last
 * filled up with -0.0, a run summed as the tree (x_l + x_{l+32}), then lanes 16, 8, 4, 2, 1 apart, the runs' sums added in run order, no
 * atomics; row g is a function of region g's own sites, their weights and the draws, however the draws are chunked and whichever
 * outputs are asked for, and two calls return the same bytes.  The device holds one double per (draw of a chunk, output row, run of 64)
 * and per (draw of a chunk, output row, region), at most BL_TOTALS_WORKSPACE_BYTES each -- or one draw's rows --, whatever n_draws is.
 * Refused with BL_ERR_INVALID, the message holding the offending value: n_periods < 1; n_regions < 1; a label outside
 * -1 .. n_regions - 1; a non-finite weight; region NULL.  Every output is untouched on any refusal.  Serves handles of
 * bl_dataset_create_dyn -- one whose every visit is masked included --; every other handle: BL_ERR_UNSUPPORTED, the message names the
 * model.  BL_ERR_BUSY while a NUTS launch is in flight on the handle.
 */
int bl_trajectory_totals(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, int n_periods, int n_regions,
                         const int32_t *region, const double *weight /* [N], NULL = 1 */, double *occupancy, double *colonised,
                         double *extinct, double *equilibrium, double *z, double *z_colonised, double *z_extinct);

/*
 * The posterior of species richness -- how many of the species that were sampled under one chain a site holds --, fused --
 * BUILDER-DEFINED (the reference has no counterpart; its users would form predict()'s psi [n_draws][T][N][S] and run a recursion over
 * the species per draw and site on the host).  ds is ONE single-species occu handle; its site covariates are every species'.  draws is
 * stacked, [n_draws][n_species][D] float32 on the host, D the handle's: block s of draw n is species s's draw, laid out as the sampler
 * lays it out.  1 <= n_species <= BL_RICHNESS_MAX_SPECIES.  With psi[n][i][s] the float32 bl_deterministic gives at site i for block
 * s of draw n, bit for bit, the species' presences are independent Bernoulli(psi_s) given the draw and their number is
 * Poisson-binomial.  In float64, with S = n_species:
 *   p_s = (double) psi[n][i][s],  q_s = 1.0 - p_s
 *   pi  = [1, 0, .., 0] (S + 1 entries);  for s = 0 .. S - 1 in ascending order:  pi_new[r] = pi[r] * q_s + pi[r - 1] * p_s  (pi[-1] = 0)
 *         -- two products and one sum, each rounded once, nothing fused.  A species with p_s = 0 leaves every entry's bits unchanged.
 *   E[n][i] = sum_s p_s, in ascending s
 * Per site, over ALL n_draws draws, every sum one float64 accumulator in ascending draw order -- so the result depends neither on the
 * launch nor on how the draws are chunked -- and nothing of size [n_draws][N] stored:
 *   site_pmf          [i][r] = (sum_n pi[n][i][r]) / n_draws                                   [N][n_species + 1]
 *   site_expected_mean[i]    = (sum_n E[n][i]) / n_draws                                       [N]
 *   site_expected_sd  [i]    = sqrt(sum_n (E[n][i] - mean)^2 / (n_draws - 1)), a second pass; NaN for n_draws == 1      [N]
 * Per draw and region, the weighted area that holds exactly r species, r = 0 .. S; region, weight and n_regions are bl_regional_totals':
 *   area_total[n][r][g] = sum_{i in g} weight_i * pi[n][i][r]                                  [n_draws][n_species + 1][n_regions]
 * Order and workspace are bl_regional_totals': every product in float64, region g's sites in site order cut into runs of 64, the last
 * filled up with -0.0, a run summed as the tree (x_l + x_{l+32}), then lanes 16, 8, 4, 2, 1 apart, the runs' sums added in run order, no
 * atomics; region g's rows are a function of its own sites, their weights and the draws, however the draws are chunked, and two calls
 * return the same bytes.  A region without a site comes back 0.  The device holds one double per (draw of a chunk, row, run of 64) and
 * per (draw of a chunk, row, region), at most BL_TOTALS_WORKSPACE_BYTES each -- or one draw's rows --, whatever n_draws is; the site
 * side has no workspace.
 * float64 on the host, NULL = skip (all four NULL: BL_ERR_INVALID); a skipped output never changes another.  region is read only for
 * area_total and may be NULL iff area_total is.  Refused with BL_ERR_INVALID, the message holding the offending value: n_species < 1;
 * n_regions < 1; a label outside -1 .. n_regions - 1; a non-finite weight.  n_species > BL_RICHNESS_MAX_SPECIES: BL_ERR_UNSUPPORTED, the
 * message names the count and the cap.  Every output is untouched on any refusal.  Serves the occu family -- plain, with a
 * false-positive rate, with random effects --; every other model and a joint-species handle: BL_ERR_UNSUPPORTED, the message names the
 * model.  BL_ERR_BUSY while a NUTS launch is in flight on the handle.  Draws must be finite.
 */
#define BL_RICHNESS_MAX_SPECIES 32
int bl_species_richness(bl_dataset *ds, int n_species, int n_draws, const float *draws /* [n_draws][n_species][D] */, int n_regions,
                        const int32_t *region, const double *weight /* [N], NULL = 1 */, double *site_pmf, double *site_expected_mean,
                        double *site_expected_sd, double *area_total);

/*
 * Spatial autocorrelation of the residuals: per posterior draw and period, Moran's I of the occupancy and the site-level detection
 * residuals of Wright, Irvine and Higgs (2019) over a sparse neighbour graph, each next to the same statistic of a replicate drawn from
 * the model, and the residuals' means over the draws per site, fused -- BUILDER-DEFINED (the reference ships the residuals,
 * biolith/evaluation/residuals.py, and leaves the statistic to its users, who would form arrays [n_draws][J][T][N] on the host).  ds is
 * ONE single-species occu handle built WITH the observations, as for bl_site_posterior.  Per draw n, period t, site i, in float64
 * unless said otherwise:
 *   psi_i, p_ij   bl_deterministic's float32 psi and prob_detection, bit for bit
 *   z_i           bl_site_posterior's z for `seed`, bit for bit: the first uniform of the cell's generator against the conditional q
 *   z'_i, y'_ij   bl_predict's latent state and y for `seed_rep`, bit for bit
 *   seen          a visit whose record in the handle is unmasked: the observation, the visit's covariates and the site's covariates
 *                 are all present;  s_it the number of seen visits of the cell,  y_ij the handle's observation
 * Occupancy residual  o_i = z_i - psi_i, its replicate o'_i = z'_i - psi_i; mask m_i = 1 for every site.
 * Detection residual  d_i = (sum_{j seen} (y_ij - p_ij)) / s_it, the sum in visit order; mask m_i = [z_i = 1 and s_it > 0].  Its
 *                     replicate takes y' and z' over the SAME seen visits.  The residual is against prob_detection, as the reference's
 *                     residuals() forms it, also where the handle has a false-positive rate.
 * The neighbour graph is CSR: row i holds nbr_idx[e], nbr_w[e] for e = nbr_ptr[i] .. nbr_ptr[i + 1] - 1 (nbr_w NULL = 1); it need not be
 * symmetric.  Moran's I of a masked field (v, m):
 *   M = sum_i m_i,  mu = (sum_i m_i v_i) / M,  c_i = v_i - mu
 *   num = sum_i m_i c_i s_i,  s_i = sum_{e in row i} w_e m_j c_j  (j = nbr_idx[e]; the products w_e c_j summed in CSR order from +0)
 *   den = sum_i m_i c_i^2,    W = sum_i m_i W_i,  W_i = sum_{e in row i} w_e m_j
 *   I = (M / W) * num / den, evaluated left to right;  NaN where M < 2, where W == 0, or where the masked v are all equal -- tested as
 *   max == min, exact and order-free, not as den == 0.
 * Every product and sum is rounded once, nothing fused.  The sums over sites are bl_regional_totals': the sites in order cut into runs
 * of 64, the last filled up, a site outside the mask and a filler holding -0.0; a run summed as the tree (x_l + x_{l+32}), then lanes
 * 16, 8, 4, 2, 1 apart; the runs' sums added in run order.  No atomics: two calls return the same bytes, and a draw's values depend
 * neither on how the draws are chunked nor on the outputs asked for.
 *   moran_occ[n][t][0 / 1]  I of (o, 1) / of (o', 1)                                   [n_draws][T][2]
 *   moran_det[n][t][0 / 1]  I of (d, m) / of (d', m')                                  [n_draws][T][2]
 *   det_sites[n][t][0 / 1]  M of the detection field / of its replicate                [n_draws][T][2]
 * Per (period, site), over ALL n_draws draws, one float64 accumulator in ascending draw order:
 *   occ_mean  [t][i] = (sum_n o_i) / n_draws                                           [T][N]
 *   n_occupied[t][i] = the draws with m_i = 1 for the detection field                  [T][N]
 *   det_mean  [t][i] = (sum over those draws of d_i) / n_occupied; NaN where it is 0   [T][N]
 * NULL = skip (all six NULL: BL_ERR_INVALID); a skipped output never changes another.  The graph is read for moran_occ and moran_det
 * alone and may be NULL when neither is wanted.  The device holds 32 bytes per (draw of a chunk, period, site) -- the four fields'
 * values, what the gather reads of a neighbour --, at most BL_TOTALS_WORKSPACE_BYTES, whatever n_draws is; a single draw that needs
 * more (T N above 2^23): BL_ERR_UNSUPPORTED.  The site side has no workspace.
 * Refused with BL_ERR_INVALID before anything is launched, the message naming the index and the value: n_draws < 1; a Moran output
 * wanted with nbr_ptr or nbr_idx NULL; nnz < 0; nbr_ptr[0] != 0; a decreasing nbr_ptr; nbr_ptr[N] != nnz; an index outside 0 .. N - 1;
 * a self-loop; a non-finite weight.  Serves the one-species handles of bl_dataset_create, _fp, _re and _re_fp; every other model,
 * occu_comb and joint-species handles included: BL_ERR_UNSUPPORTED, the message names the model.  BL_ERR_BUSY while a NUTS launch is in
 * flight on the handle.  Every output is untouched on any refusal.  Draws must be finite.
 */
int bl_residual_moran(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, uint64_t seed_rep, int32_t nnz,
                      const int32_t *nbr_ptr /* [N + 1] */, const int32_t *nbr_idx /* [nnz] */, const double *nbr_w /* [nnz], NULL = 1 */,
                      double *moran_occ, double *moran_det, int32_t *det_sites, double *occ_mean, double *det_mean, int32_t *n_occupied);

/*
 * Posterior predictive draws of the discrete sites, one per posterior draw -- what
 * numpyro.infer.Predictive(model_fn, posterior_samples)(key, site_covs, obs_covs) samples in
 * biolith/utils/predict.py:66-92 (obs withheld, so no observation is masked):
 *   occu     latent = z   [n_draws][T][N]  ~ Bernoulli(psi)                         (occu.py:208-210)
 *            y            [n_draws][J][T][N] ~ Bernoulli(z * prob_detection)        (occu.py:229-241)
 *   occu_rn  latent = N_i [n_draws][T][N]  ~ truncated Poisson(abundance) on 0..max_abundance (occu_rn.py:194-198)
 *            y            ~ Bernoulli(1 - (1 - prob_detection)^N_i)                 (occu_rn.py:211-221)
 *   false-positive handles: y ~ Bernoulli(1 - (1 - z p)(1 - f_c)(1 - (1 - z) f_u))   (occu.py:229-241)
 * uint8 on the host (NULL = skip).  The sample is a function of (seed, draw, period, site) only; it is
 * distributionally, not bitwise, the reference's (JAX threefry keys are not reproduced).
 */
int bl_predict(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, uint8_t *latent, uint8_t *y);

/*
 * The same for the count models, whose sampled sites do not fit a byte (predict.py:66-92):
 *   occu_cop  latent = z,  y ~ Poisson(session_duration * (z rate_detection + (1 - z) f_u + f_c))   (occu_cop.py:222-255)
 *   nmixture  latent = N_i ~ Poisson(abundance) restricted to 0..max_abundance,  y ~ Binomial(N_i, prob_detection)
 *             (nmixture.py:183-220; with obs withheld there is no largest-count cut-off)
 * int32 on the host, shapes as in bl_predict.  Poisson draws by inversion (rate < 10) or Hoermann's PTRS.
 */
int bl_predict_counts(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, int32_t *latent, int32_t *y);
/* Same for occu_cs (occu_cs.py:196-232 with obs withheld): z[n][T][N], f[n][J][T][N] (which score distribution a replicate
 * drew from) as bytes, s[n][J][T][N] the scores; any of the three may be NULL. */
int bl_predict_scores(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, uint8_t *latent, uint8_t *f, float *s);

/*
 * Posterior predictive of occu_comb -- BUILDER-DEFINED: the reference's predict cannot withhold scores_obs from this model (a required
 * positional argument, models/occu_comb.py:19-24, 340-349), so under its Predictive the scores stay pinned to the data while y_pc / y_aru
 * are drawn.  Here all three observed sites are drawn, one replicate data set per posterior draw
 * [beta | alpha_PC | alpha_ARU | logit fc | logit fu | mu0 | log(mu1 - mu0) | log sigma0 | log sigma1]:
 *   z      [n_draws][T][N]       ~ Bernoulli(psi)
 *   y_pc   [n_draws][Jpc][T][N]  ~ Bernoulli(z p_pc)
 *   y_aru  [n_draws][Jaru][T][N] ~ Bernoulli(1 - (1 - z p_aru)(1 - fc)(1 - (1 - z) fu))
 *   scores [n_draws][Js][T][N]   ~ Normal(z ? mu1 : mu0, z ? sigma1 : sigma0)
 * bytes / float32 on the host, NULL = skip (all four NULL: BL_ERR_INVALID); a block without replicates is empty.  Covariates that are
 * NaN read as 0 and nothing is masked, as with the observations withheld.  The cell's generator is bl_predict's; it is consumed in one
 * fixed order (z, the point counts, the ARU visits, two uniforms per score), so the sample is a function of (seed, draw, period, site)
 * only and no output depends on which others are asked for.  Serves handles of bl_dataset_create_comb; every other handle:
 * BL_ERR_UNSUPPORTED, the message names the model.  BL_ERR_BUSY while a NUTS launch is in flight on the handle.
 */
int bl_predict_comb(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, uint8_t *z, uint8_t *y_pc, uint8_t *y_aru,
                    float *scores);
/* occu_comb's deterministic sites (occu_comb.py:224-331), as bl_deterministic forms the other models': psi [n_draws][T][N] (constant over
 * T), pc_prob [n_draws][Jpc][T][N] = sigmoid(alpha_PC . (1, w_pc)), aru_prob [n_draws][Jaru][T][N] = sigmoid(alpha_ARU . (1, w_aru));
 * host float32, NULL = skip.  Serves handles of bl_dataset_create_comb only (BL_ERR_UNSUPPORTED otherwise, the message names the model). */
int bl_deterministic_comb(bl_dataset *ds, int n_draws, const float *draws, float *psi, float *pc_prob, float *aru_prob);

/*
 * The posterior predictive check (biolith/evaluation/posterior_predictive_check.py:17-160), fused: per posterior draw the discrepancy of
 * the observed and of a replicate data set against E = psi * prob_detection, without the replicate-level arrays y and prob_detection
 * [n_draws][J][T][N] that the host check reduces.  The replicate is bl_predict's y for the same seed, bit for bit (the cell's generator,
 * consumed in its order, the same arithmetic); E is the float64 product of bl_deterministic's float32 psi and prob_detection, which is
 * exact; a visit counts where obs != 255 and by nothing else.  Float64 throughout:
 *   ft(o, e) = (sqrt o - sqrt e)^2,   chi(o, e) = (o - e)^2 / (e + 1e-10)
 *   by_site:    o, y and E summed over the site's seen visits (t, j), the statistic, summed over sites
 *   by_revisit: o, y and E of revisit (t, j) summed over its seen sites, the statistic, summed over (t, j)
 * obs is [J][T][N] bytes on the host: 0, 1, or 255 = not observed (anything else: BL_ERR_INVALID).  It is passed and not taken from the
 * handle, whose rows also fold in the covariate masks.  by_site / by_revisit are [n_draws][4] float64 on the host, a draw's four being
 * ft_obs, ft_rep, chi_obs, chi_rep; NULL = skip, and a skipped output never changes the other (both NULL: BL_ERR_INVALID).  Sums run in a
 * fixed order (registers, LDS, one partial per site block, the blocks in order; no floating-point atomics): two calls return the same
 * bits.  Serves the occupancy handles of bl_predict, one species each: bl_dataset_create, _fp, _re, _re_fp; every other handle:
 * BL_ERR_UNSUPPORTED, the message names the model.  BL_ERR_BUSY while a NUTS launch is in flight on the handle.
 */
int bl_predictive_check(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, const uint8_t *obs, double *by_site,
                        double *by_revisit);

/*
 * The same check for the abundance and count models -- BUILDER-DEFINED, the reference's check being occu's: per posterior draw the
 * discrepancy of the observed and of a replicate data set against the model's mean E of y with the latent state summed out.  The replicate
 * is bl_predict's (occu_rn) / bl_predict_counts' (nmixture, occu_cop) y for the same seed, bit for bit: the cell's generator, the latent
 * state first, then every visit in j order whether it is seen or not, the same arithmetic.  E is formed in float64 from the float32 sites
 * of bl_deterministic (lambda = abundance, p = prob_detection, psi, rate = rate_detection), K = max_abundance:
 *   nmixture  E = m p,  m = sum_n n w_n / sum_n w_n,  w_n = lambda^n / n!  over n = 0 .. K (the mean of the restricted Poisson)
 *   occu_rn   E = 1 - (1 - f) sum_n w_n (1 - p)^n / sum_n w_n
 *   occu_cop  E = session_duration (psi rate + (1 - psi) f_u + f_c)
 * f (f_c if BL_FP_CONSTANT, f_u if BL_FP_UNOCCUPIED; 0 without a rate) is the float32 site value of the draw's coordinate phi:
 * (float)(1 / (1 + exp(-(double)phi))) for occu_rn, (float)exp((double)phi) for occu_cop.  The sums are scaled as they run: finite for
 * any float32 lambda (an infinite one reads as FLT_MAX); exp(-lambda) cancels and is not formed.  Statistics, groupings, output layout,
 * fixed summation order (two calls return the same bits) and NULL handling are bl_predictive_check's; counts are summed in float64.
 * obs is [J][T][N] int32 on the host: the observed count, -1 = not observed; a visit counts where obs >= 0 and by nothing else.  A value
 * below -1, or above 1 on an occu_rn handle: BL_ERR_INVALID, the message holds the value.  Serves the one-species handles of
 * bl_dataset_create_rn, _rn_re, _rn_fp, _nmix, _nmix_re, _cop, _cop_re; every other handle: BL_ERR_UNSUPPORTED, the message names the
 * model (occu handles are pointed to bl_predictive_check).  BL_ERR_BUSY while a NUTS launch is in flight on the handle.
 */
int bl_predictive_check_counts(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, const int32_t *obs, double *by_site,
                               double *by_revisit);

/*
 * The information criteria's reductions of the pointwise log-likelihood (biolith/evaluation/log_likelihood.py:10-96 under lppd.py,
 * waic.py and deviance.py), fused: the log-likelihood ll of every observation under every posterior draw, [n_draws][J][T][N], is formed
 * on the device in float64 and reduced there -- over the points per draw, and over the draws per point -- without being stored.
 * With psi and r the float32 values of bl_deterministic and y the observation:
 *   marginal == 0 (log_likelihood): z = bl_predict's latent draw for the same seed, bit for bit (the first uniform of the (draw, period,
 *     site) generator); prob = z r, or with a false-positive rate f (f_c = f if BL_FP_CONSTANT, f_u = f if BL_FP_UNOCCUPIED)
 *     prob = 1 - (1 - z r)(1 - f_c)(1 - (1 - z) f_u) in float64, f = (float)(1 / (1 + exp(-(double)phi))) the float32 site value of the
 *     draw's coordinate phi; prob clamped to [FLT_MIN, 1 - FLT_EPSILON];  ll = y log(prob) + (1 - y) log1p(-prob)
 *   marginal != 0 (log_likelihood_manual): q = (double)psi (double)r;  ll = y log(clip(q, 1e-10, 1 - 1e-10)) + (1 - y) log(clip(1 - q,
 *     1e-10, 1 - 1e-10)); no generator, and a false-positive rate is ignored
 * obs is [J][T][N] bytes on the host: 0, 1, or 255 = not a point (anything else: BL_ERR_INVALID); the caller folds every mask into it
 * (the observation, the visit's and the site's covariates).  A cell that is no point contributes nothing and draws nothing.
 *   per_draw  [n_draws]    sum of ll over the points
 *   point_lse [J][T][N]    log mean_n exp(ll) over all n_draws draws; 0 where the cell is no point
 *   point_var [J][T][N]    variance of ll over the draws, ddof 1 (0 for n_draws == 1); 0 where the cell is no point
 * float64 on the host, NULL = skip, and a skipped output never changes another (all NULL: BL_ERR_INVALID).  Every sum, the streaming
 * log-sum-exp and the Welford / Chan variance run in a fixed order (no floating-point atomics): two calls return the same bits.  Device
 * workspace: at most 64 * 4 doubles per cell and one double per (draw, 256-site block); nothing grows with n_draws * J * T * N.
 * Serves what bl_predictive_check serves; every other handle: BL_ERR_UNSUPPORTED, the message names the model.  BL_ERR_BUSY while a NUTS
 * launch is in flight on the handle.
 */
int bl_predictive_density(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, const uint8_t *obs, int marginal,
                          double *per_draw, double *point_lse, double *point_var);

/*
 * PSIS-LOO -- BUILDER-DEFINED, NO REFERENCE COUNTERPART: Pareto-smoothed importance-sampling leave-one-out (Vehtari, Simpson, Gelman, Yao
 * and Gabry; the generalised-Pareto fit is Zhang and Stephens' profile posterior mean) of every cell of a log-likelihood matrix
 * log_lik [n_draws][cells], float32 on the host -- the log_lik any conditional posterior below returns, its trailing axes folded into the
 * cells.  The entry knows no model and takes no handle.  Per cell, in float64, with ll the cell's column:
 *   lr = -ll - max(-ll);  M = ceil(min(n / 5, 3 sqrt(n)));  cut = max((M+1)-th largest lr, log(DBL_MIN))  (n < 5: the smallest lr)
 *   the tail is {lr > cut}, M' draws.  M' <= 4: k = inf, lr stays.  Otherwise, with x_i = exp(lr_(i)) - exp(cut) ascending,
 *   m = 30 + floor(sqrt(M')), b_j = (1 - sqrt(m / (j - 0.5))) / (3 x[floor(M'/4 + 0.5) - 1]) + 1 / x_max  (j = 1 .. m),
 *   kk_j = mean_i log1p(-b_j x_i), L_j = M' (log(-b_j / kk_j) - kk_j - 1), w_j = 1 / sum_l exp(L_l - L_j), w_j < 10 DBL_EPSILON dropped
 *   and the rest renormalised, b = sum_j w_j b_j, kk = mean_i log1p(-b x_i), sigma = -kk / b, k = (M' kk + 5) / (M' + 10); if k is
 *   finite the i-th smallest tail draw gets lr = min(log(sigma q_i + exp(cut)), 0), q_i = expm1(-k log1p(-p_i)) / k, p_i = (i + 0.5) / M'
 *   (q_i = -log1p(-p_i) if |k| < 1e-15)
 *   lw = lr - logsumexp(lr):   elpd = logsumexp(lw + ll),   pareto_k = k,   lppd = logsumexp(ll) - log n
 * elpd, pareto_k and lppd are [cells] float64 on the host, NULL = skip (all three NULL: BL_ERR_INVALID).  A column that holds a
 * non-finite value gets NaN in all three and changes no other cell.  A cell's outputs are a function of its column alone: every sum runs
 * in a fixed order (no floating-point atomics), and neither the neighbouring cells nor cells_per_launch change a bit.  The cells go to the
 * device in ranges of cells_per_launch (0: as many as keep the device workspace -- the range, its transpose and the outputs -- within
 * 256 MB; a larger request is cut to that).  n_draws < 2, cells < 0, cells_per_launch < 0 or a NULL matrix: BL_ERR_INVALID; n_draws above
 * BL_PSIS_MAX_DRAWS: BL_ERR_UNSUPPORTED, the message names the cap; both before anything is launched.  cells == 0 succeeds.
 */
#define BL_PSIS_MAX_DRAWS 8192
int bl_psis_loo(int device, int n_draws, int64_t cells, const float *log_lik, int64_t cells_per_launch, double *elpd, double *pareto_k,
                double *lppd);

/*
 * Conditional occupancy -- BUILDER-DEFINED, NO REFERENCE COUNTERPART (biolith/utils/predict.py withholds the observations, so its z
 * is drawn from the prior).  Per posterior draw and (period, site), with the site-period's unmasked observations `obs`:
 *   A = log psi + log p(obs | z = 1),   B = log(1 - psi) + log p(obs | z = 0)         (the terms, clamps and masks of bl_logp_grad)
 *   log_lik [n_draws][T][N] = logaddexp(A, B) = log(psi p(obs | 1) + (1 - psi) p(obs | 0)):   sum over cells = the likelihood part of -U
 *   z_prob  [n_draws][T][N] = exp(A - log_lik) = P(z = 1 | obs, theta)
 *   z       [n_draws][T][N] ~ Bernoulli(z_prob), a function of (seed, draw, period, site) only (bl_predict's generator)
 * A cell with no unmasked observation has log_lik = 0 exactly and z_prob = psi.  Host memory, NULL = skip.  draws [n_draws][D] float32 as
 * for bl_predict.  Serves one-species handles of bl_dataset_create, _fp, _re, _re_fp and _comb (its three blocks; the scores through the
 * per-period count / mean / squared-deviation rows); every other handle: BL_ERR_UNSUPPORTED, the message names the model.
 */
int bl_site_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob, uint8_t *z);

/*
 * Conditional abundance -- BUILDER-DEFINED, NO REFERENCE COUNTERPART (biolith/utils/predict.py withholds the observations, so its N_i
 * is drawn from the prior Poisson).  Per posterior draw and (period, site), with l_n the log of the n-th addend of the model's own
 * marginal likelihood over the site-period's unmasked replicates and K = max_abundance:
 *   occu_rn   l_n = log Categorical(Poisson(lambda) pmf renormalised on 0..K)(n) + sum_j log Bernoulli(y_j; 1 - (1 - p_nj)(1 - f)),
 *             p_nj = 1 - (1 - r_j)^n, f the false-positive rate or 0, probabilities clamped to [tiny, 1 - eps] as bl_logp_grad clamps them
 *   nmixture  l_n = log Poisson(lambda)(n) + sum_j log Binomial(y_j; n, p_j) for max_j y_j <= n <= K, -inf below (the untruncated Poisson
 *             cut at K, as the model's N_i_trunc_norm factor leaves it)
 *   log_lik  [n_draws][T][N] = logsumexp_n l_n:   sum over cells = the likelihood part of -U of bl_logp_grad
 *   n_mean   [n_draws][T][N] = sum_n n exp(l_n - log_lik) = E[N | obs, theta]
 *   occ_prob [n_draws][T][N] = 1 - exp(l_0 - log_lik) = P(N > 0 | obs, theta)
 *   n_draw   [n_draws][T][N] ~ exp(l_n - log_lik) by inversion, a function of (seed, draw, period, site) only (bl_predict's generator)
 * A cell with no unmasked observation returns the prior: occu_rn log_lik = 0 exactly, nmixture log_lik = log P(N <= K).  Host memory,
 * NULL = skip.  draws [n_draws][D] float32 as for bl_predict / bl_predict_counts.  Serves one-species handles of bl_dataset_create_rn,
 * _rn_re, _rn_fp, _nmix and _nmix_re; every other handle: BL_ERR_UNSUPPORTED, the message names the model.
 */
int bl_abundance_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *n_mean, float *occ_prob,
                           int32_t *n_draw);

/*
 * Conditional dynamics -- BUILDER-DEFINED, like the model it serves (bl_dataset_create_dyn).  The seasons of a site are dependent, so
 * this is a forward filter, a backward smoother and, for the joint draw, forward filtering backward sampling; per posterior draw and
 * site, with a_t = log p(y_t | z_t = 1) over season t's unmasked visits and kb_t = n_detections log tiny (the terms, clamp and masks of
 * bl_logp_grad), pi_1 = psi:
 *   forward   A = log pi_t + a_t,  B = log(1 - pi_t) + kb_t,  phi_t = sigmoid(A - B) = P(z_t = 1 | y_1..t),
 *             pi_t+1 = phi_t (1 - eps) + (1 - phi_t) gamma,   1 - pi_t+1 = phi_t eps + (1 - phi_t)(1 - gamma)   (two positive sums)
 *   log_lik  [n_draws][N]      = sum_t logaddexp(A, B), the path-marginalised log-likelihood of the SITE (the level at which the dynamic
 *                                likelihood factorises):   sum over sites = the likelihood part of -U of bl_logp_grad
 *   z_prob   [n_draws][T][N]   = rho_t = P(z_t = 1 | y_1..T, theta), the smoothed marginal
 *   col_prob [n_draws][T-1][N] = xi_t(0,1) = P(z_t = 0, z_t+1 = 1 | y_1..T, theta)
 *   ext_prob [n_draws][T-1][N] = xi_t(1,0) = P(z_t = 1, z_t+1 = 0 | y_1..T, theta)
 *   z        [n_draws][T][N]   one JOINT draw of the path: z_T ~ Bernoulli(phi_T), z_t | z_t+1 = b ~ Bernoulli(phi_t P(b | 1) /
 *                                (phi_t P(b | 1) + (1 - phi_t) P(b | 0))); the uniform of cell (draw, t, site) is bl_site_posterior's, so z
 *                                is a function of (seed, draw, period, site) only
 * A site with no unmasked observation in any season has log_lik = 0 exactly and z_prob = the propagated prior (psi, then pi_t); a season
 * with an unmasked detection has z_prob = 1 and z = 1.  Host memory, NULL = skip.  draws [n_draws][D] float32 in the sampler's layout
 * [b_psi | b_col | b_ext (Ks + 1 each) | alpha (Ko + 1)].  Serves handles of bl_dataset_create_dyn; every other handle:
 * BL_ERR_UNSUPPORTED, the message names the model (the static models' conditionals are bl_site_posterior / bl_abundance_posterior, which
 * in turn refuse occu_dyn).
 */
int bl_path_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob, float *col_prob,
                      float *ext_prob, uint8_t *z);

/*
 * Conditional scores -- BUILDER-DEFINED, NO REFERENCE COUNTERPART (biolith/utils/predict.py withholds the scores, so the z and f of
 * bl_predict_scores are drawn from the prior).  occu_cs has two enumerated layers: the site-period state z and, per recording j,
 * f_j ~ Bernoulli(z p_j), whether the score s_j came from the true-positive Normal(mu1, sigma1) or the background Normal(mu0, sigma0).
 * Per posterior draw [beta | alpha | mu0 | log(mu1 - mu0) | log sigma0 | log sigma1] and (period, site), over the cell's unmasked
 * visits (score, observation covariates and site covariates all present), n0_j / n1_j = log Normal(s_j; mu0, sigma0) / (s_j; mu1, sigma1):
 *   mix_j = logaddexp(log p_j + n1_j, log(1 - p_j) + n0_j) = log p(s_j | z = 1)
 *   A = log psi + sum_j mix_j,   B = log(1 - psi) + sum_j n0_j                             (z = 0 forces every f_j = 0)
 *   log_lik [n_draws][T][N]    = logaddexp(A, B):   sum over cells = the likelihood part of -U of bl_logp_grad
 *   z_prob  [n_draws][T][N]    = exp(A - log_lik) = P(z = 1 | the cell's scores, theta)
 *   f_prob  [n_draws][J][T][N] = z_prob r_j = P(f_j = 1 | the cell's scores, theta),  r_j = exp(log p_j + n1_j - mix_j) = P(f_j = 1 | z = 1, s_j);
 *                                a masked visit has no score to condition on: r_j = p_j (NaN covariates read as 0, as the model reads them)
 *   z       [n_draws][T][N], f [n_draws][J][T][N]   one JOINT draw: z ~ Bernoulli(z_prob), f_j = z Bernoulli(r_j), so f_j <= z; a function of
 *                                (seed, draw, period, site) only -- the cell's generator is bl_site_posterior's, its first uniform draws z,
 *                                the next J draw f_0 .. f_J-1 in order, so z is the same whether or not f is asked for
 * log p, log(1 - p), log psi, log(1 - psi) are exact log-sigmoids (no probability clamp).  A cell with no unmasked visit has log_lik = 0
 * exactly and z_prob = psi.  Host memory, NULL = skip (all five NULL: BL_ERR_INVALID).  Serves handles of bl_dataset_create_cs; every other
 * handle: BL_ERR_UNSUPPORTED, the message names the model (bl_site_posterior, bl_abundance_posterior and bl_path_posterior in turn refuse
 * occu_cs).  BL_ERR_BUSY while a NUTS launch is in flight on the handle.
 */
int bl_score_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob, uint8_t *z,
                       float *f_prob, uint8_t *f);

/*
 * Conditional counts -- BUILDER-DEFINED, NO REFERENCE COUNTERPART (biolith/utils/predict.py withholds the counts, so the z of
 * bl_predict_counts is drawn from the prior: a site where the species was counted can come back unoccupied).  occu_cop
 * (occu_cop.py:150-255): y_j ~ Poisson(d_j (z lambda_j + (1 - z) f_u + f_c)).  Per posterior draw [beta | alpha | (phi = log rate) |
 * (log sds) | (effects)] and (period, site), over the cell's unmasked visits j (count, observation covariates and site covariates all
 * present), with nu_j = alpha . (1, w_j) + site_re_det + obs_re_j where the handle has them, lambda_j = exp(min(nu_j, 80)) (the
 * sampler's clamp), f the sampled rate (0 without one), f1 = f for BL_FP_CONSTANT else 0, f0 = f in either mode, and the
 * parameter-free c_j = y_j log d_j - lgamma(y_j + 1):
 *   A = log psi       + sum_j [ y_j log(lambda_j + f1) - d_j (lambda_j + f1) + c_j ]
 *   B = log(1 - psi)  + sum_j [ y_j log f0 - d_j f0 + c_j ]      (f0 = 0: log(1 - psi) + sum c_j if the counts sum to 0, else -inf)
 *   log_lik    [n_draws][T][N]    = logaddexp(A, B):   sum over cells = -U - log prior of bl_logp_grad (c_j included)
 *   z_prob     [n_draws][T][N]    = sigmoid(A - B) = P(z = 1 | the cell's counts, theta)
 *   true_mean  [n_draws][J][T][N] = z_prob y_j rho_j,  rho_j = lambda_j / (lambda_j + f1): given z = 1 the real detections among the y_j
 *                                   counted ones are Binomial(y_j, rho_j) (Poisson thinning; rho_j = 1 unless BL_FP_CONSTANT), given z = 0 none
 *   z          [n_draws][T][N], true_count [n_draws][J][T][N]   one JOINT draw: z ~ Bernoulli(z_prob), true_count_j = z Binomial(y_j, rho_j),
 *                                   so true_count_j <= z y_j; a function of (seed, draw, period, site) only -- the cell's generator is
 *                                   bl_site_posterior's, its first uniform draws z, the visits' follow in j order (how many depends on the
 *                                   data only), so z is the same whether or not a visit-level output is asked for
 * log psi and log(1 - psi) are exact log-sigmoids, with site_re_occ in the predictor where present.  A cell with no unmasked visit has
 * log_lik = 0 exactly and z_prob = psi; without a rate a cell with a positive count has z_prob = 1 exactly and log_lik = A; a masked
 * visit has no count: true_mean = true_count = 0.  Host memory, NULL = skip (all five NULL: BL_ERR_INVALID).  Serves one-species handles of
 * bl_dataset_create_cop (with or without a rate) and bl_dataset_create_cop_re; every other handle: BL_ERR_UNSUPPORTED, the message names
 * the model (bl_site_posterior, bl_abundance_posterior, bl_path_posterior and bl_score_posterior in turn refuse occu_cop).  BL_ERR_BUSY
 * while a NUTS launch is in flight on the handle.
 */
int bl_count_posterior(bl_dataset *ds, int n_draws, const float *draws, uint64_t seed, float *log_lik, float *z_prob, uint8_t *z,
                       float *true_mean, int32_t *true_count);

/*
 * Multi-GPU: chain-parallel sampling and the gather of the draws.
 *
 * The reference's only multi-device strategy is chain_method="parallel" (biolith/utils/fit.py:109-113: one chain per
 * local device under pmap); its gather is the implicit device->host copy of mcmc.get_samples() (fit.py:132).  Here rank
 * r runs its own chains (bl_nuts_config.chain_offset selects their RNG streams), nothing is exchanged while sampling, and
 * ONE collective over RCCL / xGMI follows: every rank contributes the result block of its chains (draws, diverging,
 * num_steps, accept_prob, potential_energy, step_size, inv_mass, n_leapfrog -- contiguous in device memory) and receives
 * everybody's.  librccl is loaded on first use (BL_ERR_COMM if it cannot be).
 *
 * Two ways to make the communicators:
 *   process per GPU   rank 0 calls bl_comm_unique_id and hands the 128 bytes to the other ranks by any side channel
 *                     (a file, a socket, torch.distributed's store); every rank calls bl_comm_init_rank.
 *   one process       bl_comm_init_all(ndev, devices, comms) -- the in-process fit(..., devices=[...]).
 */
#define BL_COMM_ID_BYTES 128
typedef struct bl_comm bl_comm;
int bl_comm_rccl_version(int *version);
int bl_comm_unique_id(uint8_t *id /*[BL_COMM_ID_BYTES]*/);
int bl_comm_init_rank(const uint8_t *id /*[BL_COMM_ID_BYTES]*/, int world, int rank, int device, bl_comm **out);
int bl_comm_init_all(int ndev, const int *devices /*[ndev], distinct*/, bl_comm **out /*[ndev]*/);
/* world size, this communicator's rank and device, wall time its creation took (reported, never inside a timed region) */
int bl_comm_info(const bl_comm *comm, int *world, int *rank, int *device, double *init_ms);
int bl_comm_destroy(bl_comm *comm);
/*
 * All-gather of the last finished launch of every local dataset (bl_nuts_wait first).  comms / datasets: the n_local
 * ranks this process drives (1 for process-per-GPU; all of them after bl_comm_init_all), dataset i on communicator i's
 * device.  chains_per_rank[world]: chains each rank ran -- every rank can compute it (chains are dealt in contiguous
 * blocks), so block sizes are never negotiated.  Equal counts: one ncclAllGather; unequal: its "v" form, one grouped
 * set of broadcasts.  out (host, caller-allocated for sum(chains_per_rank) chains, fields may be NULL; out itself may be
 * NULL on ranks that do not want the result) receives the chains in rank order.
 */
int bl_gather_draws(bl_comm *const *comms, bl_dataset *const *datasets, int n_local, const int32_t *chains_per_rank,
                    bl_nuts_output *out);
/*
 * The host-only half of the gather (no GPU, no RCCL needed; what a machine without GPUs can test of the N > 1 path).
 * bl_result_block_layout: byte offsets of {draws, diverging, num_steps, accept_prob, potential_energy, step_size, inv_mass,
 * n_leapfrog, end} inside ONE rank's result block for `chains` chains of `num_samples` draws of D coordinates.
 * bl_gather_unpack: scatters a gathered buffer -- the world blocks back to back in rank order, exactly what
 * bl_gather_draws receives on the device -- into the caller's arrays, the chains in rank order.
 */
int bl_result_block_layout(int chains, int num_samples, int D, uint64_t *offsets /*[9]*/);
int bl_gather_unpack(const void *gathered, uint64_t gathered_bytes, int world, const int32_t *chains_per_rank,
                     int num_samples, int D, bl_nuts_output *out);

/* The engine's xoshiro128++ streams (host-side; no GPU needed): out[nstreams][4]. */
int bl_rng_streams(uint64_t seed, int chain, int nstreams, uint32_t *out);
/* numpyro build_adaptation_schedule restatement used by the kernel: returns window count. */
int bl_adaptation_schedule(int num_warmup, int32_t *starts, int32_t *ends, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* BIOLITH_HIP_H */
