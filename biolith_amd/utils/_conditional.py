"""What ``conditional_occupancy``, ``conditional_abundance``, ``conditional_dynamics``, ``conditional_scores`` and ``conditional_counts``
share: the checks of the model and of the posterior against the data, the unmasked-observation counts, the coordinate layout, and the loop over one device handle per species."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .data import prepare_data, species_dataset
from .layout import Layout, draws_from_sites, layout_for
from .misc import time_limit

SERVED_BY = {"occu": "conditional_occupancy", "occu_comb": "conditional_occupancy", "occu_rn": "conditional_abundance",
             "nmixture": "conditional_abundance", "occu_dyn": "conditional_dynamics", "occu_cs": "conditional_scores",
             "occu_cop": "conditional_counts"}


def _unmasked(obs, covs, site_nan):
    """(S, N, T) count of a block's replicates that enter the likelihood: y, its covariates and the site's covariates all present."""
    ok = ~(np.isnan(obs) | np.isnan(covs).any(-1)[None] | site_nan[None, :, None, None])
    return ok.sum(-1)


def plate_last(n_obs):
    """(S, N, T) -> (T, N, S) int32, the species plate where the outputs carry it."""
    return np.ascontiguousarray(n_obs.transpose(2, 1, 0)).astype(np.int32)


@dataclass
class Conditional:
    spec: object
    posterior: dict
    coef: dict              # the checked site-coefficient blocks, (n, S, Ks + 1) float32
    X: np.ndarray           # site covariates (N, Ks) float32, NaN where missing
    site_nan: np.ndarray    # (N,)
    n_obs: np.ndarray       # (S, N, T): unmasked replicates of the model's ``obs`` block
    layout: Layout
    device: int

    def per_species(self, random_seed, timeout, body):
        """``body(ds, draws, sp, seed)`` -> a tuple of arrays, for every species' handle and (n, D) draws; ``seed`` separates the
        species' streams.  Returns the tuple with every entry stacked over the species, plate last."""
        parts = []
        with time_limit(timeout):
            for sp in range(self.spec.obs.shape[0]):
                ds, draws = species_dataset(self.spec, sp, self.device), draws_from_sites(self.layout, self.posterior, sp)
                parts.append(body(ds, draws, sp, (int(random_seed) + (sp << 32)) & (2 ** 64 - 1)))
                ds.close()
        return tuple(np.stack(a, axis=-1) for a in zip(*parts))


def prepare(fn, built, hint_for, model_fn, mcmc, site_covs, obs_covs, obs, kwargs, coef=("beta",), session_duration=None) -> Conditional:
    """The front of ``fn`` (one of ``SERVED_BY``'s values): refuse what it does not serve (``built`` says what it does; a model in
    ``hint_for`` is pointed to the function that serves it), build the model's spec from the data as ``fit`` does, and check the
    posterior's ``coef`` blocks and ``alpha`` against it.  ``session_duration`` (occu_cop) is normalised with the data and handed to the model."""
    served = [m for m, f in SERVED_BY.items() if f == fn]
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError(f"{fn}(): model_fn must be a biolith_amd model (biolith_amd.models.{' / '.join(served)})")
    if name not in served:
        hint = f"; use {SERVED_BY[name]}" if name in hint_for else ""
        raise NotImplementedError(f"{fn}(): not built for {name} (built: {built}){hint}")
    device = int(kwargs.pop("device", 0))
    site_covs, obs_covs, obs, session_duration, _, _ = prepare_data(site_covs, obs_covs, obs, session_duration)
    valid = {k: v for k, v in dict(site_covs=site_covs, obs_covs=obs_covs, obs=obs, session_duration=session_duration).items() if v is not None}
    spec = model_fn(**valid, **kwargs)
    posterior = mcmc.get_samples()
    blocks = {k: np.asarray(posterior[k], dtype=np.float32) for k in coef}     # (n, S, Ks+1)
    if any(c.shape[1] != spec.obs.shape[0] or c.shape[2] != spec.site_covs.shape[1] + 1 for c in blocks.values()):
        raise ValueError(f"{fn}(): the data differ from the fitted model's (species or site covariate count)")
    comb = spec.model == "occu_comb"   # (its detection blocks are alpha_PC / alpha_ARU)
    if not comb and np.asarray(posterior["alpha"]).shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError(f"{fn}(): covariate counts differ from the fitted model's coefficients")
    X = np.asarray(spec.site_covs, dtype=np.float32)
    site_nan = np.isnan(X).any(-1)
    N, T, J, Ko = spec.obs_covs.shape
    layout = layout_for(spec, N=N, T=T, J=J, Ks=X.shape[1], Ko=Ko, Ka=spec.extras["ARU_obs_covs"].shape[3] if comb else None)
    return Conditional(spec, posterior, blocks, X, site_nan, _unmasked(spec.obs, spec.obs_covs, site_nan), layout, device)
