"""residual_moran on the GPU: the fused statistic (bl_residual_moran) against its definition in NumPy on predict()'s and
conditional_occupancy()'s arrays for the same seeds (tests/moran_ref.py) -- the geometry (one and two sites, sizes around a wave and a
block, a draw loop that strides past the grid rows, a chunk boundary), every graph shape (no edge, a ring, edges that cross waves and
blocks, an asymmetric kNN graph, a hub, isolated sites, weights that cancel), the exact identities (z, the counts, a rescaled graph),
the masks, every served handle kind, the same bytes twice, from each output alone and from the first draws, the separation of a
misspecified from a well-specified case, and the refusals at the C-ABI.

Posteriors are hand-made (random float32 coefficients in (-1, 1) behind a ``get_samples()`` stub, tests/test_gpu_regional_totals.py:
``_case``); observations are random.  Both sides evaluate the same float64 expressions in the same order, so the errors are usually 0;
the bounds are derived all the same (tests/moran_ref.py) and every compared case's bound is asserted to be below 1e-9.
Largest error seen: 0 of the bound for every Moran's I and mean (the two evaluations agree to the bit)."""
import ctypes as C

import numpy as np
import pytest

import moran_ref
from biolith_amd import _ffi, models
from biolith_amd.engine import OccuDataset
from biolith_amd.utils import conditional_occupancy, neighbour_graph, predict, residual_moran
from biolith_amd.utils._conditional import prepare
from biolith_amd.utils.data import species_dataset
from biolith_amd.utils.layout import draws_from_sites
from test_gpu_regional_totals import _case, _Posterior

pytestmark = pytest.mark.gpu

f32 = lambda a: np.asarray(a, dtype=np.float32)
VAL_BYTES, WORKSPACE = 32, 256 << 20   # residual_moran.hpp: the record of a (draw, period, site); run_over_draws' bound


def _with_obs(seed, rate=0.4, **shape):
    """``_case``'s covariates and posterior with random observations (S, N, T, J)."""
    data, posterior, opts = _case("occu", seed, **shape)
    N, T, J = data["obs_covs"].shape[:3]
    S = posterior.sites["beta"].shape[1]
    data["obs"] = f32(np.random.default_rng([seed, 1]).random((S, N, T, J)) < rate)
    return data, posterior, opts


def _handle(data, posterior, opts, sp=0):
    """Species ``sp``'s handle WITH its observations and its draw matrix, made as residual_moran makes them."""
    c = prepare("conditional_occupancy", "occu", (), models.occu, posterior, data["site_covs"], data["obs_covs"], data["obs"], dict(opts))
    return species_dataset(c.spec, sp, 0), draws_from_sites(c.layout, c.posterior, sp)


def _compare(data, posterior, opts, graph, seed=0, label=""):
    """The wrapper against the definition on predict(seed + 1)'s and conditional_occupancy(seed)'s arrays.  Returns the wrapper's result."""
    n = posterior.sites["beta"].shape[0]
    preds = predict(models.occu, posterior, data["site_covs"], data["obs_covs"], num_samples=n, random_seed=seed + 1, **opts)
    lat = conditional_occupancy(models.occu, posterior, **data, random_seed=seed, **opts)
    got = residual_moran(models.occu, posterior, **data, neighbours=graph, random_seed=seed, **opts)
    moran_ref.check(got, preds, lat, data, graph, label)
    N = data["site_covs"].shape[0]
    assert got["n_draws"] == n and got["n_sites"] == N and got["n_edges"] == len(graph[1])
    assert got["expected"] == -1.0 / (N - 1) if N > 1 else np.isnan(got["expected"])
    return got


# ------------------------------------------------------------------------------------------ graphs ----
def _csr(rows, weights=None):
    """Lists of neighbours per site -> CSR; ``weights``: lists alike, or None = unit (a NULL ``nbr_w``)."""
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.array([j for r in rows for j in r], dtype=np.int32)
    return ptr, idx, None if weights is None else np.array([w for r in weights for w in r], dtype=np.float64)


def _ring(N):
    return _csr([[(i - 1) % N, (i + 1) % N] for i in range(N)]) if N > 1 else _csr([[]])


def _crossing(N):
    """i -> (i + 64) % N and i -> (i + 256) % N: every edge leaves its wave, the second its block; arbitrary positive weights."""
    rows = [[j for j in ((i + 64) % N, (i + 256) % N) if j != i] for i in range(N)]
    rng = np.random.default_rng(N)
    return _csr(rows, [list(rng.uniform(0.5, 2.0, len(r))) for r in rows])


def _knn(N, k=4, seed=0):
    return neighbour_graph(np.random.default_rng([seed, 2]).normal(size=(N, 2)), k=k, weights="row")


def _hub(N):
    return _csr([list(range(1, N))] + [[0]] * (N - 1))


def _isolated(N):
    """A kNN graph among the first two thirds of the sites; the others have no edge and are nobody's neighbour."""
    m = 2 * N // 3
    ptr, idx, w = _knn(m, seed=5)
    return np.concatenate([ptr, np.full(N - m, ptr[-1], dtype=np.int32)]), idx, w


def _cancelling(N):
    rows = [[(i - 1) % N, (i + 1) % N] for i in range(N)]
    return _csr(rows, [[1.0, -1.0]] * N)


GRAPHS = {"ring": _ring, "crossing": _crossing, "knn": _knn, "hub": _hub, "isolated": _isolated}


# ------------------------------------------------------------------------------------------ geometry ----
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 300])
@pytest.mark.parametrize("n", [1, 3])
def test_geometry(N, n):
    T, J = (1, 3) if N % 2 else (2, 1)
    data, posterior, opts = _with_obs(N, N=N, n=n, T=T, J=J)
    graph = _crossing(N) if N > 256 else _ring(N)
    got = _compare(data, posterior, opts, graph, seed=N, label=f"N={N} n={n} T={T} J={J}")
    assert got["occupancy"]["moran_obs"].shape == (n, T, 1) and got["detection"]["n_sites_rep"].shape == (n, T, 1)
    assert got["occupancy"]["mean"].shape == (T, N, 1) and got["n_occupied"].shape == (T, N, 1)
    if N == 1:   # fewer than two sites: no I, the site outputs are served
        assert all(np.isnan(got[k][m]).all() for k in ("occupancy", "detection") for m in ("moran_obs", "moran_rep", "p_value"))
        assert np.isfinite(got["occupancy"]["mean"]).all()
    else:
        assert np.isfinite(got["occupancy"]["moran_obs"]).all() and np.isfinite(got["occupancy"]["moran_rep"]).all()
    if N == 257:
        _compare(data, posterior, opts, _ring(N), seed=N, label=f"N={N} n={n}, ring")


def test_the_draw_loop_strides_past_the_grid_rows():
    data, posterior, opts = _with_obs(12, N=3, n=1030, T=2, J=2)
    _compare(data, posterior, opts, _csr([[1, 2], [0], [1, 0]], [[0.5, 1.5], [1.0], [2.0, 0.25]]), seed=3, label="n=1030")


def test_a_chunk_boundary():
    """The workspace holds 32 bytes per (draw, period, site): at T N = 9000 a chunk is 256 MB / 288 000 = 932 draws, so 1000 draws go
    through in two.  The rows of the first chunk are those of the one-chunk call on the first 932 draws, byte for byte (a draw does not
    depend on the chunking); 64 draws before the boundary and the 68 behind it are compared with the definition."""
    N, T, n = 4500, 2, 1000
    chunk = WORKSPACE // (T * N * VAL_BYTES)
    assert chunk == 932 < n
    data, posterior, opts = _with_obs(13, N=N, n=n, T=T, J=1)
    ds, draws = _handle(data, posterior, opts)
    graph = _ring(N)
    m_occ, m_det, sites, _, _, _ = ds.residual_moran(draws, graph, seed=5, seed_rep=9, site=False)
    first = ds.residual_moran(np.ascontiguousarray(draws[:chunk]), graph, seed=5, seed_rep=9, site=False)
    for whole, part in zip((m_occ, m_det, sites), first):
        assert whole[:chunk].tobytes() == part.tobytes()
    sl = slice(chunk - 64, n)
    psi, p = (a[sl] for a in ds.deterministic(draws, psi=True, prob_detection=True))
    z = ds.site_posterior(draws, seed=5)[2][sl]
    z_rep, y_rep = (a[sl] for a in ds.predictive(draws, seed=9))
    ds.close()
    moran_ref.check_species((m_occ[sl], m_det[sl], sites[sl], None, None, None), psi, p, z, z_rep, y_rep, data["obs"][0],
                            data["obs_covs"], data["site_covs"], graph, "chunk boundary")


# ------------------------------------------------------------------------------------------ graphs ----
@pytest.mark.parametrize("kind", sorted(GRAPHS))
def test_graph_shapes(kind):
    N = 300
    data, posterior, opts = _with_obs(20, N=N, n=3, T=2, J=2)
    graph = GRAPHS[kind](N)
    if kind == "knn":   # row-standardised nearest neighbours are not mutual
        dense = np.zeros((N, N))
        dense[np.repeat(np.arange(N), 4), graph[1]] = 1
        assert not np.array_equal(dense, dense.T)
    got = _compare(data, posterior, opts, graph, seed=4, label=kind)
    assert np.isfinite(got["occupancy"]["moran_obs"]).all() and np.isfinite(got["detection"]["moran_obs"]).all()


def test_no_edge_and_weights_that_cancel():
    N = 130
    data, posterior, opts = _with_obs(21, N=N, n=3)
    empty = (np.zeros(N + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    got = _compare(data, posterior, opts, empty, seed=1, label="nnz = 0")
    assert all(np.isnan(got[k][m]).all() for k in ("occupancy", "detection") for m in ("moran_obs", "moran_rep"))
    assert np.isfinite(got["occupancy"]["mean"]).all() and got["n_occupied"].max() > 0 and got["n_edges"] == 0
    got = _compare(data, posterior, opts, _cancelling(N), seed=1, label="W == 0")
    assert np.isnan(got["occupancy"]["moran_obs"]).all() and np.isnan(got["occupancy"]["moran_rep"]).all()   # every site is in the field: W = 0
    assert got["occupancy"]["n_finite"].sum() == 0 and np.isnan(got["occupancy"]["p_value"]).all()


# ------------------------------------------------------------------------------------------ exactness ----
def test_one_draw_returns_conditional_occupancys_z():
    data, posterior, opts = _with_obs(30, N=300, n=1)
    ds, draws = _handle(data, posterior, opts)
    occ_mean = ds.residual_moran(draws, None, seed=7, seed_rep=8, moran=False)[3]
    psi = ds.deterministic(draws, psi=True, prob_detection=False)[0]
    z = ds.site_posterior(draws, seed=7)[2]
    ds.close()
    assert (occ_mean + psi[0].astype(np.float64)).tobytes() == z[0].astype(np.float64).tobytes()
    assert 0 < z.sum() < z.size


def test_the_counts_are_the_hosts():
    data, posterior, opts = _with_obs(31, N=300, n=40)
    data["obs"][0, ::7] = np.nan   # sites without a seen visit
    ds, draws = _handle(data, posterior, opts)
    graph = _knn(300)
    _, _, sites, _, _, n_occ = ds.residual_moran(draws, graph, seed=2, seed_rep=3)
    z = ds.site_posterior(draws, seed=2)[2]
    z_rep = ds.predictive(draws, seed=3, y=False)[0]
    ds.close()
    has = moran_ref.seen_visits(data["obs"][0], data["obs_covs"], data["site_covs"]).sum(-1).T > 0   # (T, N)
    assert np.array_equal(n_occ, ((z == 1) & has[None]).sum(0))
    assert np.array_equal(sites[..., 0], ((z == 1) & has[None]).sum(-1))
    assert np.array_equal(sites[..., 1], ((z_rep == 1) & has[None]).sum(-1))
    assert not has[:, ::7].any() and not n_occ[:, ::7].any()


def test_doubling_every_weight_changes_no_byte():
    data, posterior, opts = _with_obs(32, N=300, n=5)
    ds, draws = _handle(data, posterior, opts)
    ptr, idx, w = _crossing(300)
    a = ds.residual_moran(draws, (ptr, idx, w), seed=1, seed_rep=2, site=False)
    b = ds.residual_moran(draws, (ptr, idx, 2.0 * w), seed=1, seed_rep=2, site=False)
    ring = _ring(300)
    c = ds.residual_moran(draws, ring, seed=1, seed_rep=2, site=False)                                   # NULL weights ...
    d = ds.residual_moran(draws, (ring[0], ring[1], np.ones(600)), seed=1, seed_rep=2, site=False)     # ... are unit weights
    ds.close()
    assert np.isfinite(a[0]).all()
    for x, y in zip(a[:3] + c[:3], b[:3] + d[:3]):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------ masks ----
def test_masks():
    N = 130
    data, posterior, opts = _with_obs(40, N=N, n=3, T=2, J=3)
    rng = np.random.default_rng(41)
    data["obs"][0][rng.random((N, 2, 3)) < 0.2] = np.nan     # NaN observations
    data["obs"][0, 9] = np.nan                                # a site with every visit missing
    data["obs_covs"][rng.random((N, 2, 3)) < 0.1] = np.nan   # NaN visit covariates
    data["site_covs"][17, 0] = np.nan                         # a NaN site covariate: none of the site's visits is seen
    got = _compare(data, posterior, opts, _knn(N), seed=6, label="masks")
    assert not got["n_occupied"][:, [9, 17]].any() and np.isnan(got["detection"]["mean"][:, [9, 17]]).all()
    assert np.isfinite(got["occupancy"]["mean"]).all()        # the occupancy field holds every site


def test_no_occupied_site_and_a_constant_field():
    N = 130
    data, posterior, opts = _with_obs(42, N=N, n=3)
    data["obs"][:] = 0.0
    low = _Posterior({k: v.copy() for k, v in posterior.sites.items()})
    low.sites["beta"][..., 0] = -20.0                          # psi = 2e-9: no site is occupied in any draw
    got = _compare(data, low, opts, _ring(N), seed=1, label="intercept -20")
    assert not got["n_occupied"].any() and not got["detection"]["n_sites_obs"].any() and not got["detection"]["n_sites_rep"].any()
    assert np.isnan(got["detection"]["moran_obs"]).all() and np.isnan(got["detection"]["mean"]).all() and np.isnan(got["detection"]["p_value"]).all()
    high = _Posterior({k: v.copy() for k, v in posterior.sites.items()})
    high.sites["beta"][..., 0], high.sites["beta"][..., 1:] = 20.0, 0.0   # psi = 1 in float32 at every site: o = 0, max == min
    got = _compare(data, high, opts, _ring(N), seed=1, label="intercept +20")
    assert not got["occupancy"]["mean"].any()
    assert np.isnan(got["occupancy"]["moran_obs"]).all() and np.isnan(got["occupancy"]["moran_rep"]).all()
    assert (got["n_occupied"] == 3).all() and np.isfinite(got["detection"]["moran_obs"]).all()


# ------------------------------------------------------------------------------------------ every served handle kind ----
HANDLES = [{}, dict(fp="constant"), dict(fp="unoccupied"), dict(site_re=True), dict(obs_re=True), dict(site_re=True, obs_re=True)]
IDS = ["plain", "fp_constant", "fp_unoccupied", "site_re", "obs_re", "site_re-obs_re"]


@pytest.mark.parametrize("options", HANDLES, ids=IDS)
def test_every_served_handle(options):
    data, posterior, opts = _with_obs(50, N=70, T=2, J=2, n=3, **options)
    _compare(data, posterior, opts, _knn(70), seed=3, label=str(options))


def test_two_species():
    data, posterior, opts = _with_obs(51, N=70, S=2)
    graph = _knn(70)
    both = _compare(data, posterior, opts, graph, seed=4, label="S=2")
    assert both["occupancy"]["moran_obs"].shape == (3, 2, 2) and both["n_occupied"].shape == (2, 70, 2)   # the plate is last
    one = residual_moran(models.occu, _Posterior({k: v[:, :1] for k, v in posterior.sites.items()}), data["site_covs"], data["obs_covs"],
                         data["obs"][:1], neighbours=graph, random_seed=4)
    assert one["occupancy"]["moran_obs"].tobytes() == np.ascontiguousarray(both["occupancy"]["moran_obs"][..., :1]).tobytes()
    # coords in place of the graph: neighbour_graph's
    xy = np.random.default_rng(52).normal(size=(70, 2))
    a = residual_moran(models.occu, posterior, **data, coords=xy, k=5, weights="binary")
    b = residual_moran(models.occu, posterior, **data, neighbours=neighbour_graph(xy, k=5, weights="binary"))
    import scipy.sparse as sp
    ptr, idx, w = neighbour_graph(xy, k=5, weights="binary")
    c = residual_moran(models.occu, posterior, **data, neighbours=sp.csr_matrix((w, idx, ptr), shape=(70, 70)))
    for other in (b, c):
        assert a["detection"]["moran_rep"].tobytes() == other["detection"]["moran_rep"].tobytes() and a["n_edges"] == other["n_edges"] == 350


# ------------------------------------------------------------------------------------------ determinism and outputs ----
def _abi(ds, draws, graph, seed=0, seed_rep=1, which=range(6), nnz=None):
    """bl_residual_moran through ctypes with only the outputs ``which`` passed; the others stay untouched (-7)."""
    n = draws.shape[0]
    out = [np.full((n, ds.T, 2), -7.0), np.full((n, ds.T, 2), -7.0), np.full((n, ds.T, 2), -7, dtype=np.int32),
           np.full((ds.T, ds.N), -7.0), np.full((ds.T, ds.N), -7.0), np.full((ds.T, ds.N), -7, dtype=np.int32)]
    ptr = lambda a, t: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
    keep = [None if graph is None or a is None else np.ascontiguousarray(a, dtype=d)
            for a, d in zip(graph or (None,) * 3, (np.int32, np.int32, np.float64))]
    types = [C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_int32]
    rc = ds._lib.bl_residual_moran(ds._h, n, draws.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(seed), C.c_uint64(seed_rep),
                                   (0 if keep[1] is None else keep[1].size) if nnz is None else nnz,
                                   ptr(keep[0], C.c_int32), ptr(keep[1], C.c_int32), ptr(keep[2], C.c_double),
                                   *[ptr(a, t) if k in which else None for k, (a, t) in enumerate(zip(out, types))])
    return rc, out


def _untouched(out, but=()):
    return all((a == -7).all() for k, a in enumerate(out) if k not in but)


def test_same_bytes_twice_each_output_alone_and_the_first_draws():
    data, posterior, opts = _with_obs(60, N=300, n=40)
    ds, draws = _handle(data, posterior, opts)
    graph = _knn(300)
    rc, a = _abi(ds, draws, graph, 1, 2)
    assert rc == 0 and not any((x == -7).any() for x in a)
    rc, b = _abi(ds, draws, graph, 1, 2)
    assert rc == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for k in range(6):
        rc, alone = _abi(ds, draws, graph if k < 2 else None, 1, 2, which=[k])   # (the graph is read for I alone)
        assert rc == 0 and alone[k].tobytes() == a[k].tobytes() and _untouched(alone, but=[k]), k
    rc, few = _abi(ds, np.ascontiguousarray(draws[:7]), graph, 1, 2)
    assert rc == 0 and all(few[k].tobytes() == a[k][:7].tobytes() for k in range(3))
    rc, other = _abi(ds, draws, graph, 1, 3)                                      # another replicate: the observed side stays
    assert rc == 0 and other[0][..., 0].tobytes() == a[0][..., 0].tobytes() and not np.array_equal(other[0][..., 1], a[0][..., 1])
    assert other[3].tobytes() == a[3].tobytes() and other[5].tobytes() == a[5].tobytes()
    # the engine's method: the same arrays, None where not wanted
    m = ds.residual_moran(draws, graph, seed=1, seed_rep=2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(m, a))
    assert ds.residual_moran(draws, graph, moran=False)[:3] == (None, None, None)
    assert ds.residual_moran(draws, graph, site=False)[3:] == (None, None, None)
    ds.close()


# ------------------------------------------------------------------------------------------ separation ----
@pytest.mark.parametrize("gradient", [True, False])
def test_separation(gradient):
    """An omitted west-east gradient in the occupancy is found; a well-specified model is not accused (the cases and their p-values
    in NumPy alone: tests/test_residual_moran_cpu.py)."""
    data, sites, coords = moran_ref.separation_case(gradient)
    posterior = _Posterior(sites)
    graph = neighbour_graph(coords, k=8)
    got = _compare(data, posterior, {}, graph, seed=0, label="gradient" if gradient else "well specified")
    same = residual_moran(models.occu, posterior, **data, coords=coords, random_seed=0)
    assert same["occupancy"]["moran_obs"].tobytes() == got["occupancy"]["moran_obs"].tobytes()
    p = got["occupancy"]["p_value"][0, 0]
    print("p_value", p, "mean I_obs", got["occupancy"]["moran_obs"].mean(), "mean I_rep", got["occupancy"]["moran_rep"].mean())
    assert got["occupancy"]["n_finite"][0, 0] == 40
    assert p < 0.05 if gradient else 0.1 < p < 0.9
    if gradient:
        assert got["occupancy"]["moran_obs"].min() > got["expected"] + 0.1


# ------------------------------------------------------------------------------------------ the C-ABI's refusals ----
def test_refusals_at_the_abi():
    rng = np.random.default_rng(0)
    N = 20
    X, W = f32(rng.normal(size=(N, 1))), f32(rng.normal(size=(N, 2, 2, 1)))
    Y = f32(rng.random((1, N, 2, 2)) < 0.4)
    blank = lambda J: np.full((1, N, 2, J), np.nan, dtype=np.float32)
    ring = _ring(N)
    refused = {"occu_dyn": OccuDataset(X, W, Y, model="occu_dyn"),
               "occu_rn": OccuDataset(X, W, Y, model="occu_rn", max_abundance=5),
               "occu_comb": OccuDataset(X, W, blank(2), model="occu_comb", ARU_obs_covs=rng.normal(size=(N, 2, 3, 1)), ARU_obs=blank(3),
                                        scores_obs=blank(2)),
               "a joint-species handle": OccuDataset(X, W, np.concatenate([Y, Y]))}
    for name, ds in refused.items():
        dr = np.zeros((2, ds.D), dtype=np.float32)
        rc, out = _abi(ds, dr, ring)
        assert rc == _ffi.BL_ERR_UNSUPPORTED and b"bl_residual_moran: not built for " + name.encode() in ds._lib.bl_last_error(), name
        assert _untouched(out), name
        with pytest.raises(NotImplementedError):
            ds.residual_moran(dr, ring)
        ds.close()
    ds = OccuDataset(X, W, Y)
    dr = np.zeros((3, ds.D), dtype=np.float32)
    last = ds._lib.bl_last_error
    ptr, idx, _ = ring
    w = np.ones(idx.size)

    def refuses(graph, message, **more):
        rc, out = _abi(ds, dr, graph, **more)
        assert rc == _ffi.BL_ERR_INVALID and message in last() and _untouched(out), (message, rc, last())

    shifted = ptr.copy(); shifted[0] = 1
    refuses((shifted, idx, w), b"nbr_ptr[0]=1, not 0")
    falling = ptr.copy(); falling[6] = falling[5] - 1
    refuses((falling, idx, w), b"nbr_ptr[6]=9 below nbr_ptr[5]=10")
    refuses((ptr, idx, w), b"nbr_ptr[20]=40, not nnz=39", nnz=39)
    for bad in (N, -1):
        outside = idx.copy(); outside[11] = bad
        refuses((ptr, outside, w), b"nbr_idx[11]=%d outside 0 .. N - 1 = 19" % bad)
    loop = idx.copy(); loop[8] = 4
    refuses((ptr, loop, w), b"nbr_idx[8]=4 is a self-loop of site 4")
    for bad, text in ((np.nan, b"nan"), (np.inf, b"inf")):
        heavy = w.copy(); heavy[13] = bad
        refuses((ptr, idx, heavy), b"nbr_w[13]=" + text + b" is not finite")
    refuses(None, b"the neighbour graph is NULL")                                  # Moran's I wanted, no graph
    refuses(None, b"the neighbour graph is NULL", which=[1])
    rc, out = _abi(ds, dr, ring, which=())                                          # all six outputs NULL
    assert rc == _ffi.BL_ERR_INVALID and _untouched(out)
    rc, out = _abi(ds, dr[:0], ring)                                                # n_draws = 0
    assert rc == _ffi.BL_ERR_INVALID and b"n_draws=0" in last()
    rc, out = _abi(ds, dr, None, which=[2, 3, 4, 5])                                # no I wanted: the graph may be NULL
    assert rc == 0 and not any((out[k] == -7).any() for k in (2, 3, 4, 5)) and _untouched(out, but=[2, 3, 4, 5])
    with pytest.raises(ValueError):
        ds.residual_moran(dr, None)
    with pytest.raises(ValueError):
        ds.residual_moran(dr, ring, moran=False, site=False)
    with pytest.raises(ValueError):
        ds.residual_moran(dr, (ptr[:-1], idx, None))
    with pytest.raises(ValueError):
        ds.residual_moran(dr[:, :-1], ring)
    # a NUTS launch in flight
    ds.launch(num_warmup=200000, num_samples=200000, num_chains=2, seed=0)
    rc, out = _abi(ds, dr, ring)
    assert rc == _ffi.BL_ERR_BUSY and b"in flight" in last() and _untouched(out)
    ds.abort()
    with pytest.raises(Exception, match="aborted"):
        ds.wait()
    rc, out = _abi(ds, dr, ring)
    assert rc == 0 and not any((x == -7).any() for x in out)                        # the handle stays usable
    ds.close()
