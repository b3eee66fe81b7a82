"""residual_moran without a GPU: the exports; ``neighbour_graph`` against a brute-force distance matrix; the wrapper's refusals, which
come before any device call; the p-value rule; the definition (tests/moran_ref.py) on a field whose I is known in closed form; and
the two cases of the separation test, chosen here with the NumPy restatement alone."""
import numpy as np
import pytest

import moran_ref
from biolith_amd import _ffi, models, utils
from biolith_amd.utils.residual_moran import neighbour_graph, p_value, residual_moran


def test_exports():
    assert "residual_moran" in utils.__all__ and "neighbour_graph" in utils.__all__
    assert utils.residual_moran is residual_moran and utils.neighbour_graph is neighbour_graph
    assert "bl_residual_moran" in _ffi.EXPORTS


# ------------------------------------------------------------------------------------------ neighbour_graph ----
def _brute(xy, k):
    """Per row the k nearest other sites by (distance, index), from the full distance matrix."""
    N = xy.shape[0]
    d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
    m = min(k, N - 1)
    rows = []
    for i in range(N):
        others = np.array([j for j in range(N) if j != i], dtype=np.int64)
        rows.append(others[np.lexsort((others, d[i, others]))][:m])
    return np.array(rows, dtype=np.int64).reshape(N, m)


CLOUDS = {
    "one": np.array([[0.3, 0.7]]),
    "two": np.array([[0.0, 0.0], [1.0, 2.0]]),
    "nine": np.random.default_rng(0).normal(size=(9, 2)),
    "grid": np.stack(np.meshgrid(np.arange(5.0), np.arange(4.0), indexing="ij"), -1).reshape(-1, 2),   # ties at every distance
    "duplicates": np.repeat(np.random.default_rng(1).normal(size=(3, 2)), [5, 1, 3], axis=0),           # 9 sites at 3 places
    "all_equal": np.zeros((9, 3)),
    "line": np.arange(9.0)[:, None],
}


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
@pytest.mark.parametrize("k", [1, 2, 4, 8, 9, 20])
def test_neighbour_graph_against_brute_force(cloud, k):
    xy = CLOUDS[cloud]
    N = xy.shape[0]
    want = _brute(xy, k)
    m = want.shape[1]
    for weights in ("row", "binary"):
        indptr, indices, data = neighbour_graph(xy, k=k, weights=weights)
        assert indptr.dtype == np.int32 and indices.dtype == np.int32 and data.dtype == np.float64
        assert indptr.shape == (N + 1,) and indptr[0] == 0 and indptr[-1] == len(indices) == len(data) == N * m
        assert np.array_equal(np.diff(indptr), np.full(N, m))
        assert np.array_equal(indices.reshape(N, m), want), (cloud, k)
        assert not np.any(indices.reshape(N, m) == np.arange(N)[:, None])          # no self-loops
        assert np.all(data == (1.0 / m if weights == "row" and m else 1.0))
        if weights == "row" and m:
            assert np.allclose(np.add.reduceat(data, indptr[:-1]), 1.0)


def test_neighbour_graph_refusals():
    with pytest.raises(ValueError):
        neighbour_graph(np.zeros((4, 2)), k=0)
    with pytest.raises(ValueError):
        neighbour_graph(np.zeros((4, 2)), weights="kernel")
    with pytest.raises(ValueError):
        neighbour_graph(np.array([[0.0, np.nan]]))
    with pytest.raises(ValueError):
        neighbour_graph(np.zeros((2, 2, 2)))
    # the default: k = 8, row-standardised
    ptr, idx, w = neighbour_graph(np.random.default_rng(2).normal(size=(30, 2)))
    assert ptr[-1] == 240 and np.all(w == 0.125)


# ------------------------------------------------------------------------------------------ the wrapper's refusals ----
class _Posterior:
    def __init__(self, sites):
        self.sites = sites

    def get_samples(self):
        return self.sites


def _small(N=12, T=2, J=2, n=3):
    rng = np.random.default_rng(5)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    data = dict(site_covs=f32(rng.normal(size=(N, 1))), obs_covs=f32(rng.normal(size=(N, T, J, 1))), obs=f32(rng.random((1, N, T, J)) < 0.4))
    post = _Posterior(dict(beta=f32(rng.uniform(-1, 1, (n, 1, 2))), alpha=f32(rng.uniform(-1, 1, (n, 1, 2)))))
    return data, post


def test_the_wrapper_refuses_before_any_device_call(monkeypatch):
    data, post = _small()
    import biolith_amd.utils._conditional as cond

    def no_device(*a, **k):
        raise AssertionError("a device handle was asked for")

    monkeypatch.setattr(cond, "species_dataset", no_device)
    xy = np.random.default_rng(6).normal(size=(12, 2))
    graph = neighbour_graph(xy, k=3)
    with pytest.raises(ValueError, match="exactly one of coords and neighbours"):
        residual_moran(models.occu, post, **data)
    with pytest.raises(ValueError, match="exactly one of coords and neighbours"):
        residual_moran(models.occu, post, **data, coords=xy, neighbours=graph)
    with pytest.raises(ValueError, match="12 sites"):
        residual_moran(models.occu, post, **data, coords=xy[:11])
    with pytest.raises(ValueError, match="12 sites"):
        residual_moran(models.occu, post, **data, neighbours=neighbour_graph(xy[:11], k=3))
    import scipy.sparse as sp
    with pytest.raises(ValueError, match="12 sites"):
        residual_moran(models.occu, post, **data, neighbours=sp.csr_matrix((11, 11)))
    with pytest.raises(ValueError):
        residual_moran(models.occu, post, **data, neighbours=(graph[0], graph[1]))
    with pytest.raises(ValueError):
        residual_moran(models.occu, post, **data, neighbours=(graph[0], graph[1], graph[2][:-1]))
    for name in ("occu_rn", "nmixture", "occu_cop", "occu_cs", "occu_dyn", "occu_comb"):
        with pytest.raises(NotImplementedError, match="built for occu alone"):
            residual_moran(getattr(models, name), post, **data, coords=xy)
    with pytest.raises(TypeError):
        residual_moran("occu", post, **data, coords=xy)
    # ... and with everything in order the first thing it asks for is the device
    with pytest.raises(AssertionError, match="a device handle was asked for"):
        residual_moran(models.occu, post, **data, coords=xy)


# ------------------------------------------------------------------------------------------ the p-value rule ----
def test_the_p_value_rule():
    nan = np.nan
    obs = np.array([[0.1, nan, 0.3], [0.2, nan, nan], [0.0, nan, 0.1], [0.5, nan, nan]])   # (n = 4, 3 columns)
    rep = np.array([[0.2, 0.1, nan], [0.2, nan, 0.0], [-.1, 0.3, 0.1], [nan, 0.0, 0.0]])
    share, k = p_value(obs, rep)
    # column 0: draws 0, 1, 2 finite in both; rep >= obs in draws 0 and 1 (a tie counts).  column 1: none.  column 2: draw 2 alone, a tie.
    assert np.array_equal(k, [3, 0, 1]) and k.dtype == np.int64
    assert share[0] == 2 / 3 and np.isnan(share[1]) and share[2] == 1.0
    share, k = p_value(np.full((5, 2, 1), nan), np.zeros((5, 2, 1)))
    assert share.shape == (2, 1) and np.isnan(share).all() and not k.any()
    share, k = p_value(np.array([[np.inf], [0.0]]), np.array([[1.0], [1.0]]))                 # an infinite I is not finite
    assert share[0] == 1.0 and k[0] == 1
    want, kk = moran_ref.p_value(obs, rep)
    assert np.array_equal(want, p_value(obs, rep)[0], equal_nan=True) and np.array_equal(kk, [3, 0, 1])


# ------------------------------------------------------------------------------------------ the definition itself ----
def test_the_definition_on_fields_with_a_known_answer():
    # a ring of N sites with v alternating +1 / -1: every neighbour disagrees, I = -1; N even
    N = 130
    ring = (np.arange(N + 1) * 2, np.stack([(np.arange(N) - 1) % N, (np.arange(N) + 1) % N], 1).reshape(-1), None)
    v = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    I, M, bound = moran_ref.moran(v[None], ring)
    assert I[0] == -1.0 and M[0] == N and bound[0] < 1e-12
    # the first half +1, the second -1: all but four of the 2 N ordered pairs agree
    half = np.where(np.arange(N) < N // 2, 1.0, -1.0)
    I, _, _ = moran_ref.moran(half[None], ring)
    assert abs(I[0] - (2 * N - 8) / (2 * N)) < 1e-15
    # the undefined cases: fewer than two sites in the field, a constant field, no edge inside the field, weights that cancel
    one = np.full(N, np.nan)
    one[5] = 0.3
    assert np.isnan(moran_ref.moran(one[None], ring)[0][0]) and moran_ref.moran(one[None], ring)[1][0] == 1
    assert np.isnan(moran_ref.moran(np.full((1, N), 0.25), ring)[0][0])
    apart = np.full(N, np.nan)
    apart[[3, 50]] = [0.1, 0.9]
    assert np.isnan(moran_ref.moran(apart[None], ring)[0][0])
    cancel = (ring[0], ring[1], np.tile([1.0, -1.0], N))
    assert np.isnan(moran_ref.moran(v[None], cancel)[0][0])
    # a site outside the field takes no part: the statistic of the sites inside, on the graph between them
    rng = np.random.default_rng(3)
    xy = rng.normal(size=(90, 2))
    g = neighbour_graph(xy, k=4)
    f = rng.normal(size=90)
    inside = rng.random(90) < 0.7
    masked = np.where(inside, f, np.nan)
    I, M, _ = moran_ref.moran(masked[None], g)
    dense = np.zeros((90, 90))
    for i in range(90):
        dense[i, g[1][g[0][i]:g[0][i + 1]]] = g[2][g[0][i]:g[0][i + 1]]
    sub, c = dense[np.ix_(inside, inside)], f[inside] - f[inside].mean()
    assert M[0] == inside.sum() and abs(I[0] - inside.sum() / sub.sum() * (c @ sub @ c) / (c @ c)) < 1e-13
    # the sum's order: one run's tree, then the runs
    x = rng.normal(size=(2, 200))
    assert np.allclose(moran_ref.wave_sum(x), x.sum(-1), rtol=0, atol=1e-13) and moran_ref.wave_sum(x[:, :1]).tobytes() == x[:, 0].tobytes()


# ------------------------------------------------------------------------------------------ separation, on the CPU ----
@pytest.mark.parametrize("gradient", [True, False])
def test_the_separation_cases_separate_in_numpy_alone(gradient):
    """The omitted west-east gradient drives the occupancy field's p-value below 0.05; the well-specified case leaves it in (0.1, 0.9)."""
    data, sites, coords = moran_ref.separation_case(gradient)
    graph = neighbour_graph(coords, k=8, weights="row")
    obs = data["obs"][0]
    psi, p, z, z_rep, y_rep = moran_ref.restate_plain(data["site_covs"], data["obs_covs"], obs, sites["beta"][:, 0], sites["alpha"][:, 0], 0, 1)
    v, _ = moran_ref.fields(psi, p, z, z_rep, y_rep, obs, moran_ref.seen_visits(obs, data["obs_covs"], data["site_covs"]))
    I_obs, _, b_obs = moran_ref.moran(v[0], graph)
    I_rep, _, b_rep = moran_ref.moran(v[1], graph)
    assert max(b_obs.max(), b_rep.max()) < moran_ref.BOUND_CAP
    share, k = moran_ref.p_value(I_obs, I_rep)
    print("gradient" if gradient else "well specified", "p_value", share, "mean I_obs", I_obs.mean(), "mean I_rep", I_rep.mean())
    assert k[0] == 40
    assert share[0] < 0.05 if gradient else 0.1 < share[0] < 0.9
