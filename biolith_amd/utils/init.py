"""Initialisation strategies for ``fit(init_strategy=...)`` (biolith/utils/fit.py:29, 93: ``NUTS(model_fn, init_strategy=init_strategy or
init_to_uniform)``).  The reference hands NumPyro's ``numpyro.infer.init_to_*`` callables through; NumPyro is not part of this engine,
so these are small descriptors of the same names and meaning that ``fit`` resolves into the kernel's ``init_theta`` (one start position
per chain, in the unconstrained space the sampler works in):

* ``init_to_uniform(radius=2)`` -- Uniform(-radius, radius) per unconstrained coordinate (the default; with radius 2 the kernel draws
  it itself from the chain's own xoshiro streams, exactly as ``init_strategy=None``);
* ``init_to_feasible()`` -- every unconstrained coordinate 0;
* ``init_to_value(values={"beta": ..., "alpha": ...})`` -- the named sites at the given values, everything else as ``init_to_uniform``
  (NumPyro's rule);
* ``init_to_mean()`` / ``init_to_median(num_samples=15)`` / ``init_to_sample()`` -- from the coefficients' priors (Normal / Laplace:
  mean = median = loc; a draw; the median of ``num_samples`` draws): plain coefficient models only.

Objects with these names from NumPyro itself (``functools.partial`` of its ``init_to_*`` functions) are recognised by name and keyword
arguments, so a reference-style call keeps working.  Draw-level equality with NumPyro is impossible either way (its keys are threefry).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Any, Dict, Optional

import numpy as np

from .layout import layout_for


@dataclass(frozen=True)
class InitStrategy:
    kind: str
    radius: float = 2.0
    num_samples: int = 15
    values: Dict[str, Any] = field(default_factory=dict)


def init_to_uniform(site=None, radius: float = 2.0) -> InitStrategy:
    return InitStrategy("uniform", radius=float(radius))


def init_to_feasible(site=None) -> InitStrategy:
    return InitStrategy("feasible")


def init_to_value(site=None, values: Optional[Dict[str, Any]] = None) -> InitStrategy:
    return InitStrategy("value", values=dict(values or {}))


def init_to_mean(site=None) -> InitStrategy:
    return InitStrategy("mean")


def init_to_median(site=None, num_samples: int = 15) -> InitStrategy:
    return InitStrategy("median", num_samples=int(num_samples))


def init_to_sample(site=None) -> InitStrategy:
    return InitStrategy("sample")


_BY_NAME = dict(init_to_uniform=init_to_uniform, init_to_feasible=init_to_feasible, init_to_value=init_to_value,
                init_to_mean=init_to_mean, init_to_median=init_to_median, init_to_sample=init_to_sample)


def as_strategy(obj) -> Optional[InitStrategy]:
    """None, one of this module's descriptors (or the function itself, as ``fit(init_strategy=init_to_median)``), or NumPyro's
    ``init_to_*`` callables / their ``functools.partial`` forms, recognised by name."""
    if obj is None or isinstance(obj, InitStrategy):
        return obj
    func, kw = getattr(obj, "func", obj), dict(getattr(obj, "keywords", None) or {})
    name = getattr(func, "__name__", "")
    if name in _BY_NAME:
        kw.pop("site", None)
        return _BY_NAME[name](**kw)
    raise NotImplementedError(f"init_strategy={obj!r}: the HIP engine knows init_to_uniform / _feasible / _value / _mean / _median / _sample "
                              "(biolith_amd.utils.init, or NumPyro's callables of those names)")


def _prior_draws(rng, prior, shape):
    loc, scale = float(prior[0]), float(prior[1])
    if getattr(prior, "family", "normal") == "laplace":
        return rng.laplace(loc, scale, size=shape)
    return rng.normal(loc, scale, size=shape)


_COEFFICIENTS_ONLY = ("built for models whose coordinates are all regression coefficients "
                      "(no false-positive rate, random effects or score parameters); use init_to_uniform / _feasible / _value")


def _coordinates(block, v, sp, theta):
    """``init_to_value``: the value ``v`` given for ``block``'s site -> species ``sp``'s coordinates (``theta``: the chain's start so far)."""
    if block.width > 1 or len(block.shape) > 1:
        row = v if v.ndim == 1 else v[sp]   # (n_species, K + 1), the reference's site shape, or one row for all
        if row.shape != (block.width,):
            raise ValueError(f"init_to_value: {block.site} must have {block.width} coefficients per species, got shape {v.shape}")
        return row
    x = float(v.reshape(-1)[sp] if v.size > 1 else v.reshape(()))   # a scalar, or one value per species
    if block.transform == "sigmoid":
        if not 0.0 < x < 1.0:
            raise ValueError(f"init_to_value: {block.site} must lie in (0, 1)")
        return np.log(x) - np.log1p(-x)
    if block.transform == "gap":
        x -= theta[block.offset - 1]
        if not x > 0.0:
            raise ValueError(f"init_to_value: {block.site} must exceed mu0 (its prior is truncated below at mu0)")
    elif block.transform == "exp" and not x > 0.0:
        raise ValueError(f"init_to_value: {block.site} must be positive")
    return x if block.transform == "identity" else np.log(x)


def _start_positions(strategy, layout, *, D, priors, num_chains, first_chain, seed, species):
    """Start positions ``(num_chains, D)`` float64 of one launch, or None when the kernel's own draw applies (``init_to_uniform`` at
    radius 2).  ``layout`` names the blocks ``init_to_value`` may set (constrained values in, the engine's coordinates out);
    ``priors``: site -> coefficient prior when theta is nothing but those sites (``init_to_mean`` / ``_median`` / ``_sample``), else
    None.  Chain c of the fit gets its own generator (seed, c): what a chain starts from does not depend on how the chains are dealt
    to launches."""
    if strategy is None or (strategy.kind == "uniform" and strategy.radius == 2.0):
        return None
    vals = {k: np.asarray(v, dtype=np.float64) for k, v in strategy.values.items()}
    unknown = set(vals) - {b.site for b in layout.blocks}
    if unknown:
        raise NotImplementedError(f"init_to_value: sites {sorted(unknown)} are not sampled sites of {layout.model}")
    if strategy.kind in ("mean", "median", "sample") and priors is None:
        raise NotImplementedError(f"init_to_{strategy.kind}: {_COEFFICIENTS_ONLY}")
    radius = strategy.radius if strategy.kind == "uniform" else 2.0
    out = np.empty((num_chains, D), dtype=np.float64)
    for c in range(num_chains):
        rng = np.random.default_rng([int(seed) & 0x7FFFFFFF, first_chain + c, 0x1B1D])
        if strategy.kind == "feasible":
            out[c] = 0.0
            continue
        out[c] = rng.uniform(-radius, radius, size=D)
        if strategy.kind in ("uniform", "value"):
            for b, s in ((b, s) for b in layout.blocks if b.site in vals for s in range(layout.S)):
                out[c, b.offset + s * b.stride: b.offset + s * b.stride + b.width] = _coordinates(b, vals[b.site], species + s, out[c])
            continue
        n = 1 if strategy.kind == "sample" else strategy.num_samples
        for s in range(layout.S):
            for b in layout.blocks:
                prior = priors[b.site]
                col = np.full(b.width, float(prior[0])) if strategy.kind == "mean" else np.median(_prior_draws(rng, prior, (n, b.width)), axis=0)
                out[c, b.offset + s * b.stride: b.offset + s * b.stride + b.width] = col
    return out


def initial_positions(strategy: Optional[InitStrategy], *, D: int, Ks: int, Ko: int, n_species: int, plain: bool, blocks_first: bool = True, prior_beta, prior_alpha,
                      num_chains: int, first_chain: int, seed: int, species: int = 0):
    """Start positions for every model but occu_comb.  ``n_species`` species' coefficient blocks lie in THIS launch's theta of ``D``
    coordinates (one unless the species are sampled jointly), the launch's first species is ``species``; ``plain``: theta holds nothing
    but those coefficient blocks; ``blocks_first``: it starts with [beta, alpha] (all models but the dynamic one).  ``init_to_value``
    sets ``beta`` / ``alpha`` only."""
    if plain and not blocks_first:
        raise ValueError("initial_positions: the dynamic model's theta is not plain [beta, alpha] (plain=True needs blocks_first=True)")
    if strategy is not None and strategy.kind == "value":
        unknown = set(strategy.values) - {"beta", "alpha"}
        if unknown:
            raise NotImplementedError(f"init_to_value: sites {sorted(unknown)} are not coefficient sites of this engine (beta, alpha)")
        if not blocks_first and strategy.values:
            raise NotImplementedError("init_to_value: not built for the dynamic model's coefficient layout")
    coefficients = layout_for(SimpleNamespace(model="occu" if blocks_first else "occu_dyn", extras={}), N=0, T=0, J=0, Ks=Ks, Ko=Ko,
                              species_in_handle=n_species)
    return _start_positions(strategy, coefficients, D=D, priors=dict(beta=prior_beta, alpha=prior_alpha) if plain else None,
                            num_chains=num_chains, first_chain=first_chain, seed=seed, species=species)


def comb_initial_positions(strategy: Optional[InitStrategy], *, Ks: int, Kpc: int, Karu: int, num_chains: int, first_chain: int,
                           seed: int, species: int = 0):
    """Start positions for occu_comb (one species per launch).  ``init_to_value`` takes the reference's site names with constrained
    values (``ARU_prob_fp_constant``, ``ARU_fp_unoccupied``, ``mu0``, ``mu1``, ``sigma0``, ``sigma1``: a scalar, or one value per
    species; the coefficients as ``(n_species, K + 1)`` or one row); everything not named starts as ``init_to_uniform``."""
    layout = layout_for(SimpleNamespace(model="occu_comb", extras={}), N=0, T=0, J=0, Ks=Ks, Ko=Kpc, Ka=Karu)
    return _start_positions(strategy, layout, D=layout.D, priors=None, num_chains=num_chains, first_chain=first_chain, seed=seed, species=species)
