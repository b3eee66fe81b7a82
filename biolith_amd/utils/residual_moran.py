"""``residual_moran`` -- is there spatial structure left in the residuals?  Moran's I of the occupancy and detection residuals per
posterior draw, against the same statistic of replicates drawn from the model, fused on the HIP engine.

No model of this engine has a spatial effect, so the first question an occupancy analyst asks of a map -- are the residuals
autocorrelated -- decides whether the fitted model can be trusted at all.  The residuals are those of Wright, Irvine and Higgs (2019),
who apply Moran's I to them: the occupancy residual ``z - psi`` with ``z`` drawn GIVEN the observations
(``conditional_occupancy``), and the detection residual ``y - p`` at the sites a draw has occupied (``evaluation.residuals``).  On the
host that is ``conditional_occupancy`` + ``predict`` + ``residuals`` and a sparse product per draw over arrays of size (n, J, T, N).
Here one C-ABI call per species -- ``bl_residual_moran`` (``include/biolith_hip.h``) -- regenerates every value in registers, gathers
over the neighbour graph and reduces in a fixed order.  BUILDER-DEFINED: the reference ships the residuals and leaves the statistic to
its users.  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from ._conditional import prepare


def neighbour_graph(coords, k: int = 8, weights: str = "row"):
    """The ``k`` nearest other sites of every site by Euclidean distance, as CSR ``(indptr int32, indices int32, data float64)``.

    ``coords`` is (N, d).  A row lists its neighbours by distance, ties by index -- also ties at the ``k``-th distance, so the graph
    is a function of the coordinates alone; duplicate coordinates are allowed (distance 0, never the site itself).  With
    ``N - 1 < k`` a row holds the ``N - 1`` neighbours there are.  ``weights``: ``"binary"`` 1, ``"row"`` one over the row's
    length (row-standardised: ``1 / k``).  The graph is in general not symmetric."""
    from scipy.spatial import cKDTree

    xy = np.asarray(coords, dtype=np.float64)
    if xy.ndim == 1:
        xy = xy[:, None]
    if xy.ndim != 2 or not np.isfinite(xy).all():
        raise ValueError("neighbour_graph(): coords must be a finite (N, d) array")
    if int(k) < 1:
        raise ValueError(f"neighbour_graph(): k={k}, at least 1")
    if weights not in ("row", "binary"):
        raise ValueError(f"neighbour_graph(): weights={weights!r}, 'row' or 'binary'")
    N, m = xy.shape[0], min(int(k), max(xy.shape[0] - 1, 0))
    indptr = (np.arange(N + 1, dtype=np.int64) * m).astype(np.int32)
    data = np.full(N * m, 1.0 / m if weights == "row" and m else 1.0)
    if m == 0:
        return indptr, np.zeros(0, dtype=np.int32), data[:0]
    tree = cKDTree(xy)
    kk = min(m + 2, N)   # the site itself, its m neighbours, and one more that shows a tie at the m-th distance
    _, j = tree.query(xy, k=kk)
    j = np.asarray(j).reshape(N, kk)
    dist = lambda a, b: np.sqrt(((a - b) ** 2).sum(-1))   # (one statement of the distance: ties compare as a brute-force search's)
    dd = dist(xy[:, None, :], xy[j])
    rows = np.arange(N)
    is_self = j == rows[:, None]
    dd[is_self] = -1.0   # the site itself first
    order = np.lexsort((j.ravel(), dd.ravel(), np.repeat(rows, kk))).reshape(N, kk) - rows[:, None] * kk
    j, dd = np.take_along_axis(j, order, 1), np.take_along_axis(dd, order, 1)
    indices = j[:, 1:m + 1].copy()
    # a row whose query missed the site itself (more duplicates than kk) or is tied at its last place: every site within that distance
    slow = ~is_self.any(1)
    if kk == m + 2:
        slow |= dd[:, m + 1] == dd[:, m]
    for i in np.flatnonzero(slow):
        near = np.asarray(tree.query_ball_point(xy[i], dd[i, -1] * (1.0 + 1e-12) + 1e-300), dtype=np.int64)
        near = near[near != i]
        d = dist(xy[i], xy[near])
        indices[i] = near[np.lexsort((near, d))][:m]
    return indptr, indices.reshape(-1).astype(np.int32), data


def _csr(neighbours, N):
    """``neighbours`` -- a CSR triple or a scipy.sparse matrix -- as (indptr int32, indices int32, data float64 or None)."""
    if hasattr(neighbours, "tocsr"):
        m = neighbours.tocsr()
        if m.shape != (N, N):
            raise ValueError(f"residual_moran(): neighbours is {m.shape}, the data hold {N} sites")
        neighbours = (m.indptr, m.indices, m.data)
    if not isinstance(neighbours, (tuple, list)) or len(neighbours) != 3:
        raise ValueError("residual_moran(): neighbours is a CSR triple (indptr, indices, data) or a scipy.sparse matrix")
    indptr = np.ascontiguousarray(np.asarray(neighbours[0]).reshape(-1), dtype=np.int32)
    indices = np.ascontiguousarray(np.asarray(neighbours[1]).reshape(-1), dtype=np.int32)
    data = None if neighbours[2] is None else np.ascontiguousarray(np.asarray(neighbours[2], dtype=np.float64).reshape(-1))
    if indptr.size != N + 1:
        raise ValueError(f"residual_moran(): neighbours' indptr holds {indptr.size} entries, the data hold {N} sites (N + 1 = {N + 1})")
    if data is not None and data.size != indices.size:
        raise ValueError("residual_moran(): neighbours' data and indices differ in length")
    return indptr, indices, data


def p_value(moran_obs, moran_rep):
    """Over the draws (axis 0) with both ``I`` finite: the share in which ``I_rep >= I_obs``, NaN where there is none, and their
    number."""
    obs, rep = np.asarray(moran_obs, dtype=np.float64), np.asarray(moran_rep, dtype=np.float64)
    ok = np.isfinite(obs) & np.isfinite(rep)
    n_finite = ok.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = (ok & (rep >= obs)).sum(axis=0) / np.where(n_finite > 0, n_finite, np.nan)
    return share, n_finite.astype(np.int64)


def residual_moran(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    coords=None,
    neighbours=None,
    k: int = 8,
    weights: str = "row",
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Moran's I of the occupancy and detection residuals of a fitted ``occu`` model per posterior draw and period, with the
    posterior predictive p-value of each against replicates drawn from the model.

    The data are passed exactly as to :func:`biolith_amd.utils.fit` -- the observations are needed --, the model's options and
    ``device=`` go through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of that fit.  Exactly one of ``coords`` -- an (N, d) array,
    from which :func:`neighbour_graph` makes the ``k``-nearest-neighbour graph with ``weights`` -- and ``neighbours`` -- a CSR triple
    ``(indptr, indices, data)`` or a ``scipy.sparse`` matrix, any graph without self-loops, symmetric or not -- is given.

    Per species, draw and period (``include/biolith_hip.h``: ``bl_residual_moran``), with ``seed`` the species' seed as
    ``conditional_occupancy`` derives it from ``random_seed`` and ``seed_rep = seed + 1``:

    * ``moran_obs`` is Moran's I of ``evaluation.residuals({**predict(seed_rep), "z": conditional_occupancy(seed)["z"]}, obs)``:
      the occupancy residual ``z - psi`` over every site; the detection residual averaged over a site's seen visits, over the sites
      the draw has occupied that have a seen visit;
    * ``moran_rep`` is the same of ``predict(seed_rep)``'s own ``z`` and ``y``, over the same seen visits.

    ``I = (M / W) sum_i c_i sum_j w_ij c_j / sum_i c_i^2`` over the ``M`` sites in the field, ``c`` centred on their mean, ``W`` the
    weights between them; NaN where ``M < 2``, ``W == 0`` or the values are all equal.  The detection residual is against
    ``prob_detection``, as the reference's ``residuals`` forms it, also with ``false_positives_*``.  A well-specified model gives
    ``p_value`` away from 0; spatial structure the model lacks raises ``I_obs`` above its replicates and drives ``p_value`` to 0.
    The same call returns the same bytes; nothing of size (n, J, T, N) is formed.

    Returns
    -------
    dict
        species plate last, n = posterior draws: ``occupancy``: ``{"moran_obs" (n, T, S), "moran_rep" (n, T, S), "p_value" (T, S)
        -- the share of the draws with both I finite in which I_rep >= I_obs, NaN if none --, "n_finite" (T, S), "mean" (T, N, S)
        the mean residual over the draws}``; ``detection``: the same keys and ``"n_sites_obs"``, ``"n_sites_rep"`` (n, T, S) int, the
        sites in the field (its ``mean`` is over the draws that have the site occupied, NaN where none has); ``n_occupied``
        (T, N, S) those draws' number; ``expected`` ``= -1 / (N - 1)``, I's expectation without autocorrelation; ``n_draws``,
        ``n_sites``, ``n_edges``.

    Raises
    ------
    TypeError
        ``model_fn`` is not a biolith_amd model.
    NotImplementedError
        every model but ``occu``.
    ValueError
        both or neither of ``coords`` and ``neighbours``; a graph for another number of sites, with a self-loop, an index outside
        the sites or a non-finite weight; data that differ from the fitted model's.

    Examples
    --------
    >>> from biolith_amd.models import simulate, occu
    >>> from biolith_amd.utils import fit, residual_moran
    >>> data, _ = simulate()
    >>> results = fit(occu, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> out = residual_moran(occu, results.mcmc, **data, coords=xy)
    >>> out["occupancy"]["p_value"]
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("residual_moran(): model_fn must be a biolith_amd model (biolith_amd.models.occu)")
    if name != "occu":
        raise NotImplementedError(f"residual_moran(): built for occu alone (with or without false positives / random effects), not for {name}")
    if (coords is None) == (neighbours is None):
        raise ValueError("residual_moran(): exactly one of coords and neighbours is given")
    c = prepare("conditional_occupancy", "occu", (), model_fn, mcmc, site_covs, obs_covs, obs, kwargs)
    N = int(c.X.shape[0])
    if coords is not None:
        xy = np.asarray(coords, dtype=np.float64)
        if xy.ndim == 1:
            xy = xy[:, None]
        if xy.ndim != 2 or xy.shape[0] != N:
            raise ValueError(f"residual_moran(): coords is {xy.shape}, the data hold {N} sites")
        graph = neighbour_graph(xy, k=k, weights=weights)
    else:
        graph = _csr(neighbours, N)
    mask = 2 ** 64 - 1

    def body(ds, draws, sp, seed):
        return ds.residual_moran(draws, graph, seed=seed, seed_rep=(seed + 1) & mask)

    m_occ, m_det, sites, o_mean, d_mean, n_occ = c.per_species(random_seed, timeout, body)   # (n, T, 2, S) and (T, N, S)
    out = {}
    for key, m, mean in (("occupancy", m_occ, o_mean), ("detection", m_det, d_mean)):
        obs_i, rep_i = np.ascontiguousarray(m[:, :, 0]), np.ascontiguousarray(m[:, :, 1])
        share, n_finite = p_value(obs_i, rep_i)
        out[key] = {"moran_obs": obs_i, "moran_rep": rep_i, "p_value": share, "n_finite": n_finite, "mean": mean}
    out["detection"]["n_sites_obs"] = np.ascontiguousarray(sites[:, :, 0])
    out["detection"]["n_sites_rep"] = np.ascontiguousarray(sites[:, :, 1])
    out["n_occupied"] = n_occ
    out["expected"] = -1.0 / (N - 1) if N > 1 else float("nan")
    out["n_draws"], out["n_sites"], out["n_edges"] = int(m_occ.shape[0]), N, int(graph[1].size)
    return out
