"""tests/pred_rng_ref.py is right (no GPU): the vectorised generator against a scalar one written with Python integers and explicit
masks (nothing of it rests on NumPy's wrap-around), splitmix64's published values, the grid of the uniforms, and the reference
samplers against scipy's pmfs by chi-square tests at fixed seeds (both branches of the Poisson sampler, each side of rate 10)."""
import numpy as np
import pytest
from scipy import stats

import pred_rng_ref as R

M64, M32 = (1 << 64) - 1, (1 << 32) - 1


def _splitmix_int(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return x, z ^ (z >> 31)


def _rotl32(x, k):
    return ((x << k) | (x >> (32 - k))) & M32


def _scalar_uniforms(seed, index, count):
    """``count`` uniforms of BlPredRng(seed, index) as exact fractions of 2^24 (Python integers)."""
    x = (seed & M64) ^ ((index * 0xD1342543DE82EF95) & M64)
    x, a = _splitmix_int(x)
    x, b = _splitmix_int(x)
    s0, s1, s2, s3 = a & M32, a >> 32, b & M32, (b >> 32) | 1
    out = []
    for _ in range(count):
        r0 = (s0 + s3) & M32
        r = (_rotl32(r0, 7) + s0) & M32
        t = (s1 << 9) & M32
        s2 ^= s0
        s3 ^= s1
        s1 ^= s2
        s0 ^= s3
        s2 ^= t
        s3 = _rotl32(s3, 11)
        out.append(r >> 8)
    return out


def test_splitmix64_published_values():
    x = np.zeros(1, dtype=np.uint64)
    x, a = R.splitmix64(x)
    x, b = R.splitmix64(x)
    assert int(a[0]) == 0xE220A8397B1DCDAF and int(b[0]) == 0x6E789E6AA1B965F4
    s, a = _splitmix_int(0)
    assert a == 0xE220A8397B1DCDAF and _splitmix_int(s)[1] == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32, 2 ** 63 + 5, 2 ** 64 - 1])
def test_vectorised_generator_equals_scalar(seed):
    # indices 0, 1 and 2^40 + 3 as (n, t, i) of a (T, N) = (4, 2^20) grid: (n T + t) N + i
    T, N = 4, 2 ** 20
    cells = [(0, 0, 0), (0, 0, 1), (2 ** 18, 0, 3)]
    assert [(n * T + t) * N + i for n, t, i in cells] == [0, 1, 2 ** 40 + 3]
    n, t, i = (np.array(c) for c in zip(*cells))
    rng = R.CellRng(seed, n, T, t, N, i)
    got = np.stack([rng.uniform() for _ in range(40)], axis=1)
    for row, (cn, ct, ci) in zip(got, cells):
        want = _scalar_uniforms(seed, (cn * T + ct) * N + ci, 40)
        assert [int(v * 2 ** 24) for v in row] == want and all(v * 2 ** 24 == int(v * 2 ** 24) for v in row)
    assert (rng.taken == 40).all()


def test_seed_bits_above_32_matter():
    a, b = (R.cells(s, [0], 1, 8).uniform() for s in (5, 5 + (1 << 32)))
    assert not np.array_equal(a, b)


def test_partial_advance_matches_full():
    full, part = R.cells(7, range(3), 2, 5), R.cells(7, range(3), 2, 5)
    mask = (np.arange(30).reshape(3, 2, 5) % 3) == 0
    u1 = full.uniform()
    v1 = part.uniform(where=mask)
    assert np.array_equal(v1[mask], u1[mask]) and np.isnan(v1[~mask]).all()
    assert np.array_equal(part.uniform()[~mask], u1[~mask])          # the cells left behind are still at their first uniform
    assert np.array_equal(part.taken, np.where(mask, 2, 1))


def test_uniforms_on_the_grid():
    rng = R.cells(3, range(50), 2, 100)
    for _ in range(5):
        u = rng.uniform()
        assert (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)


def _chi_square(sample, pmf_of, lo, hi, min_expected=8.0):
    """p-value of the sample against the pmf on lo .. hi, tail bins merged until each expects ``min_expected``."""
    ks = np.arange(lo, hi + 1)
    e = pmf_of(ks) * sample.size
    o = np.bincount(np.clip(sample, lo, hi) - lo, minlength=ks.size).astype(float)
    e[0] += sample.size * pmf_of(np.arange(0, lo)).sum() if lo > 0 else 0.0
    e[-1] += sample.size - e.sum()                                   # the upper tail's mass
    bins_o, bins_e, ao, ae = [], [], 0.0, 0.0
    for oo, ee in zip(o, e):
        ao, ae = ao + oo, ae + ee
        if ae >= min_expected:
            bins_o.append(ao)
            bins_e.append(ae)
            ao = ae = 0.0
    bins_o[-1] += ao
    bins_e[-1] += ae
    bo, be = np.array(bins_o), np.array(bins_e)
    return float(stats.chi2.sf(((bo - be) ** 2 / be).sum(), bo.size - 1)), bo.size


@pytest.mark.parametrize("lam", [0.3, 9.99, 10.0, 40.0, 2000.0])
def test_poisson_follows_its_pmf(lam):
    rng = R.cells(2024, range(40), 1, 1000)
    k, took = R.poisson(rng, lam)
    assert np.array_equal(took, rng.taken)
    if lam < 10:
        assert np.array_equal(took, k + 1)                           # the sequential search: count + 1 uniforms
    else:
        assert (took % 2 == 0).all() and (took >= 2).all() and took.mean() < 3.0   # PTRS: two per round, ~1.1-1.3 rounds
    sd = np.sqrt(lam)
    p, nb = _chi_square(k.ravel(), lambda q: stats.poisson.pmf(q, lam), max(0, int(lam - 6 * sd)), int(lam + 6 * sd) + 1)
    assert nb >= 3 and p > 1e-3, (lam, p, nb)
    assert abs(k.mean() - lam) < 5 * sd / np.sqrt(k.size)


def test_poisson_branches_meet_at_ten_and_zero_rate_takes_nothing():
    rng = R.cells(1, [0], 1, 4)
    k, took = R.poisson(rng, np.array([0.0, -1.0, np.nan, 9.999999]).reshape(1, 1, 4))
    assert np.array_equal(took.ravel()[:3], [0, 0, 0]) and np.array_equal(k.ravel()[:3], [0, 0, 0])
    assert took.ravel()[3] == k.ravel()[3] + 1
    # the same uniforms, the two branches: 10 - ulp goes by products (count + 1 uniforms), 10 by PTRS (an even number)
    a, b = R.cells(9, range(200), 1, 1), R.cells(9, range(200), 1, 1)
    ka, ta = R.poisson(a, np.nextafter(10.0, 0.0))
    kb, tb = R.poisson(b, 10.0)
    assert np.array_equal(ta, ka + 1) and (tb % 2 == 0).all()


def test_binomial_follows_its_pmf_and_takes_n_uniforms():
    rng = R.cells(77, range(40), 1, 1000)
    n = np.broadcast_to(np.array([0, 1, 7, 12])[np.arange(1000) % 4], rng.shape)
    k = R.binomial(rng, n, 0.37)
    assert np.array_equal(rng.taken, n)
    for nn in (1, 7, 12):
        p, nb = _chi_square(k[n == nn], lambda q: stats.binom.pmf(q, nn, 0.37), 0, nn)
        assert p > 1e-3, (nn, p, nb)
    assert (k[n == 0] == 0).all()
    z = R.cells(77, range(2), 1, 10)
    assert np.array_equal(R.binomial(z, 5, 0.0), np.zeros(z.shape)) and (z.taken == 5).all()   # p = 0 still takes n


@pytest.mark.parametrize("eta,K", [(np.log(0.4), 1), (np.log(3.0), 6), (np.log(3.0), 127), (np.log(30.0), 20)])
def test_truncated_poisson_follows_its_pmf(eta, K):
    rng = R.cells(5, range(40), 1, 1000)
    k = R.truncated_poisson(rng, eta, K)
    assert (rng.taken == 1).all() and k.min() >= 0 and k.max() <= K
    norm = stats.poisson.cdf(K, np.exp(eta))
    p, nb = _chi_square(k.ravel(), lambda q: np.where(q <= K, stats.poisson.pmf(q, np.exp(eta)) / norm, 0.0), 0, K)
    assert p > 1e-3, (eta, K, p, nb)


def test_truncated_poisson_without_mass_is_K():
    rng = R.cells(0, range(2), 1, 5)
    assert (R.truncated_poisson(rng, 7.0, 6) == 6).all()            # exp(7) > 745: exp(-lambda) = 0, no m has mass
    assert (rng.taken == 1).all()


def test_normal_takes_two_uniforms_and_is_standard():
    rng = R.cells(8, range(40), 1, 1000)
    g = R.normal(rng)
    assert (rng.taken == 2).all() and np.isfinite(g).all()
    assert stats.kstest(g.ravel(), "norm").pvalue > 1e-3
    # the floor: the largest radius is sqrt(-2 log 2^-24)
    assert np.abs(g).max() <= np.sqrt(48 * np.log(2.0)) + 1e-12


def test_uniform_order_helper():
    assert R.uniform_order("predict", J=2) == ["latent", "y[0]", "y[1]"]
    assert R.uniform_order("predict_scores", J=1) == ["z", "f[0]", "s[0].radius", "s[0].angle"]
    assert R.uniform_order("predict_comb", Jpc=1, Jaru=2, Js=1) == ["z", "y_pc[0]", "y_aru[0]", "y_aru[1]", "scores[0].radius",
                                                                    "scores[0].angle"]
    assert R.uniform_order("score_posterior", J=2) == ["z", "f[0]", "f[1]"]
    with pytest.raises(KeyError):
        R.uniform_order("count_posterior")
    assert set(R.UNIFORM_ORDER) >= {"predict", "predict_counts/nmixture", "predict_counts/occu_cop", "predict_scores", "predict_comb",
                                    "site_posterior", "abundance_posterior", "score_posterior", "count_posterior", "path_posterior"}
