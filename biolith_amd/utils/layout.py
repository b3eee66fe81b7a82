"""The coordinate order of the engine's unconstrained vector ``theta`` -- stated once.

The sampler works on ``theta``; the reference's consumers read named sample sites.  ``layout_for`` lists, in order, the blocks of
``theta`` for one device handle, and three functions translate on top of it: ``sites_from_draws`` (draws -> sites, ``fit``),
``draws_from_sites`` (sites -> draws, ``predict`` / ``conditional_occupancy``) and ``species_block`` (a joint several-species draw ->
the one-species layout).  ``init`` takes its offsets from the same blocks.

==================================  ==========================================================================================
plain                               ``[beta, alpha]``
occu_fp / occu_cop with a rate      ``[beta, alpha, phi]``, phi = logit(prob_fp_<mode>) / log(rate_fp_<mode>)
occu_cs                             ``[beta, alpha, mu0, log(mu1 - mu0), log sigma0, log sigma1]``
random effects (occu, occu_rn,      ``[beta, alpha, (phi), (log site_re_sd), (log obs_re_sd), (site_re_occ | site_re_abu [N],
nmixture, occu_cop)                 site_re_det [N]), (obs_re [N][T][J])]``
occu_dyn                            ``[beta | beta_col | beta_ext | alpha]``
occu_comb                           ``[beta | alpha_PC | alpha_ARU | logit fc | logit fu | mu0 | log(mu1 - mu0) | log sigma0 |
                                    log sigma1]``
several species in one handle       ``[sp 0: beta, alpha | sp 1: ... | shared phi, log sds | site_re_occ [S][N] | site_re_det
(occu, occu_fp, occu_re)            [S][N] | obs_re [S][N][T][J]]``
==================================  ==========================================================================================

Transforms are evaluated in float64 and stored as float32.  On the way back a probability is clipped to [1e-300, 1 - 1e-16] before
the logit and a positive quantity to >= 1e-300 before the log.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

PLATE = -1   # stands for the species plate in ``Block.shape``


@dataclass(frozen=True)
class Block:
    """One named site's run of coordinates.  ``shape`` is the site's shape behind the draw axes, ``PLATE`` marking the species axis
    (absent: the site is shared across species); the columns hold one species' values in Fortran order of the remaining axes
    (``obs_re[j, t, n]`` lies at ``(n T + t) J + j``).  Species ``sp`` of the handle starts at ``offset + sp * stride``.
    ``transform`` maps a coordinate x to the site: ``identity``, ``exp``, ``sigmoid``, or ``gap`` = the previous coordinate + exp(x)
    (mu1 above mu0)."""

    site: str
    offset: int
    width: int
    stride: int
    shape: Tuple[int, ...]
    transform: str = "identity"

    @property
    def per_species(self) -> bool:
        return PLATE in self.shape


@dataclass(frozen=True)
class Layout:
    model: str
    blocks: Tuple[Block, ...]
    S: int                      # species in the handle
    fp_site: Optional[str]      # the sampled false-positive site (prob_fp_<mode> / rate_fp_<mode>), or None

    @property
    def D(self) -> int:
        return sum(b.width * (self.S if b.per_species else 1) for b in self.blocks)

    @property
    def plain(self) -> bool:
        """theta holds nothing but the species' [beta, alpha]."""
        return all(b.site in ("beta", "alpha") for b in self.blocks)

    def __getitem__(self, site) -> Block:
        for b in self.blocks:
            if b.site == site:
                return b
        raise KeyError(site)


def layout_for(spec, *, N, T, J, Ks, Ko, Ka=None, species_in_handle=1) -> Layout:
    """The blocks of ``theta`` for a handle of ``spec``'s model (``spec.model``, ``spec.extras``) holding ``species_in_handle`` species."""
    S, ex, model = int(species_in_handle), spec.extras, spec.model
    if S > 1 and model not in ("occu", "occu_fp", "occu_re"):
        raise NotImplementedError(f"{model}: one species per handle")
    blocks, at = [], 0

    def coefficients(*named):   # a species' coefficient vectors lie together: [sp 0: beta, alpha | sp 1: beta, alpha | ...]
        nonlocal at
        stride = sum(w for _, w in named)
        for name, w in named:
            blocks.append(Block(name, at, w, stride, (PLATE, w)))
            at += w
        at += (S - 1) * stride

    def shared(name, transform):   # one scalar outside the species plate
        nonlocal at
        blocks.append(Block(name, at, 1, 0, (), transform))
        at += 1

    def plated(name, shape=(), transform="identity"):   # [S][...]: one run per species
        nonlocal at
        w = int(np.prod(shape, dtype=np.int64))
        blocks.append(Block(name, at, w, w, tuple(shape) + (PLATE,), transform))
        at += S * w

    fp_site = None
    if model == "occu_dyn":
        coefficients(("beta", Ks + 1), ("beta_col", Ks + 1), ("beta_ext", Ks + 1), ("alpha", Ko + 1))
    elif model == "occu_comb":
        coefficients(("beta", Ks + 1), ("alpha_PC", Ko + 1), ("alpha_ARU", Ka + 1))
        for name, transform in (("ARU_prob_fp_constant", "sigmoid"), ("ARU_fp_unoccupied", "sigmoid"), ("mu0", "identity"),
                                ("mu1", "gap"), ("sigma0", "exp"), ("sigma1", "exp")):
            plated(name, (), transform)
    else:
        coefficients(("beta", Ks + 1), ("alpha", Ko + 1))
        if model == "occu_cop" and ex["fp_mode"] is not None:
            fp_site = f"rate_fp_{ex['fp_mode']}"
            shared(fp_site, "exp")
        mode = ex["fp_mode"] if model == "occu_fp" else ex.get("re_fp_mode")
        if mode is not None:
            fp_site = f"prob_fp_{mode}"
            shared(fp_site, "sigmoid")
        if model == "occu_cs":
            for name, transform in (("mu0", "identity"), ("mu1", "gap"), ("sigma0", "exp"), ("sigma1", "exp")):
                shared(name, transform)
        site_re, obs_re = bool(ex.get("site_random_effects")), bool(ex.get("obs_random_effects"))
        if site_re:
            shared("site_re_sd", "exp")
        if obs_re:
            shared("obs_re_sd", "exp")
        if site_re:   # (the abundance models name the first one after their predictor: nmixture.py:166-169, occu_rn.py:172-176)
            plated("site_re_abu" if model in ("nmixture", "occu_rn") else "site_re_occ", (N,))
            plated("site_re_det", (N,))
        if obs_re:
            plated("obs_re", (J, T, N))
    return Layout(model, tuple(blocks), S, fp_site)


def _forward(block, draws):
    """One handle's draws ``(C, S, D)`` -> the block's site values ``(C, S, width)``, float32."""
    x = draws[:, :, block.offset: block.offset + block.width]
    if block.transform == "identity":
        return x
    x = x.astype(np.float64)
    if block.transform == "exp":
        return np.exp(x).astype(np.float32)
    if block.transform == "sigmoid":
        return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)
    return (draws[:, :, block.offset - 1: block.offset].astype(np.float64) + np.exp(x)).astype(np.float32)   # gap: above the coordinate in front


def _constrained(block, posterior, sp):
    """Species ``sp``'s values of the block's site as (n, width) columns in theta's order: identity blocks as stored, the others in
    float64 and clipped for the inverse transform."""
    a = np.asarray(posterior[block.site])
    if block.per_species:
        a = a[(slice(None),) * (1 + block.shape.index(PLATE)) + (sp,)]
    if block.transform == "identity":
        return a.transpose((0,) + tuple(range(a.ndim - 1, 0, -1))).reshape(a.shape[0], block.width)   # Fortran order of the site's own axes
    a = a.astype(np.float64).reshape(-1, 1)
    if block.transform == "sigmoid":
        return np.clip(a, 1e-300, 1 - 1e-16)
    return np.maximum(a, 1e-300) if block.transform == "exp" else a


def sites_from_draws(layout, draws_per_species) -> dict:
    """Draws ``(C, S, D)`` of one-species handles, one per species -> the sampled sites grouped by chain, species plate as in
    ``Block.shape``.  A shared site is read from the first species' draws.  One copy per block, none of the whole matrix."""
    assert layout.S == 1
    first, nsp = draws_per_species[0], len(draws_per_species)
    lead, sites = first.shape[:2], {}
    for b in layout.blocks:
        if not b.per_species:   # (a scalar)
            sites[b.site] = _forward(b, first)[:, :, 0]
            continue
        p = b.shape.index(PLATE)
        own = b.shape[:p] + b.shape[p + 1:]
        out = np.empty(lead + b.shape[:p] + (nsp,) + b.shape[p + 1:], dtype=np.float32)
        for sp, d in enumerate(draws_per_species):
            v = _forward(b, d).reshape(lead + own[::-1])
            out[(slice(None),) * (2 + p) + (sp,)] = v.transpose((0, 1) + tuple(range(1 + len(own), 1, -1)))
        sites[b.site] = out
    return sites


def draws_from_sites(layout, posterior, sp) -> np.ndarray:
    """Posterior sites (draws flattened on axis 0) -> species ``sp``'s ``(n, D)`` float32 matrix in the one-species layout."""
    assert layout.S == 1
    cols, previous = [], None
    for b in layout.blocks:
        v = _constrained(b, posterior, sp)
        if b.transform == "sigmoid":
            x = np.log(v / (1.0 - v))
        elif b.transform == "exp":
            x = np.log(v)
        elif b.transform == "gap":
            x = np.log(np.maximum(v - previous, 1e-300))
        else:
            x = v
        cols.append(x.astype(np.float32, copy=False))
        previous = v
    return np.concatenate(cols, axis=1)


def fp_rate(layout, posterior):
    """Draws ``(n,)`` float64 of the sampled false-positive site ``layout.fp_site``, clipped as the engine's coordinate wants them."""
    return _constrained(layout[layout.fp_site], posterior, 0).reshape(-1)


def species_block(joint_layout, joint_draws, sp) -> np.ndarray:
    """Species ``sp``'s coordinates of a joint draw ``(C, S, D_joint)`` in the one-species layout (shared coordinates ride along)."""
    parts = [joint_draws[:, :, b.offset + sp * b.stride: b.offset + sp * b.stride + b.width] if b.per_species
             else joint_draws[:, :, b.offset: b.offset + b.width] for b in joint_layout.blocks]
    return np.ascontiguousarray(np.concatenate(parts, axis=2))
