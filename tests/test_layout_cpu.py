"""utils/layout.py: the one statement of theta's coordinate order.  Closed-form widths, the meaning of every block pinned on literal
offsets, the round trip sites <-> draws, the joint split, and fit's three assemblers on stub handles.  Host only: no library, no GPU."""
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest

from biolith_amd.engine import NutsResult
from biolith_amd.utils.layout import PLATE, draws_from_sites, fp_rate, layout_for, sites_from_draws, species_block

fit_module = importlib.import_module("biolith_amd.utils.fit")   # (biolith_amd.utils exports the function ``fit`` under the module's name)

N, T, J, Ks, Ko, Ka = 4, 2, 3, 1, 2, 1
DIMS = dict(N=N, T=T, J=J, Ks=Ks, Ko=Ko, Ka=Ka)
P = Ks + Ko + 2   # one species' [beta, alpha]


def _re(site, obs, **kw):
    return dict(site_random_effects=site, obs_random_effects=obs, prior_site_re_sd=1.0, prior_obs_re_sd=1.0, **kw)


def _effects(site, obs, S=1):   # (tests/test_re_cpu.py, tests/test_gpu_re.py: the suite's closed formulas)
    return int(site) + int(obs) + S * ((2 * N if site else 0) + (N * T * J if obs else 0))


# name -> (model, extras, D of a one-species handle)
FORMS = {
    "occu": ("occu", {}, P),
    "occu_fp_constant": ("occu_fp", dict(fp_mode="constant"), P + 1),
    "occu_fp_unoccupied": ("occu_fp", dict(fp_mode="unoccupied"), P + 1),
    "occu_cop": ("occu_cop", dict(fp_mode=None), P),
    "occu_cop_rate": ("occu_cop", dict(fp_mode="constant"), P + 1),
    "occu_cop_rate_effects": ("occu_cop", _re(True, True, fp_mode="unoccupied"), P + 1 + _effects(True, True)),
    "occu_cop_effects": ("occu_cop", _re(False, True, fp_mode=None), P + _effects(False, True)),
    "occu_rn": ("occu_rn", dict(max_abundance=10), P),
    "occu_rn_rate_no_effects": ("occu_rn", _re(False, False, re_fp_mode="constant"), P + 1),
    "occu_rn_rate_effects": ("occu_rn", _re(True, True, re_fp_mode="constant"), P + 1 + _effects(True, True)),
    "occu_rn_effects": ("occu_rn", _re(True, False), P + _effects(True, False)),
    "nmixture": ("nmixture", dict(max_abundance=10), P),
    "nmixture_effects": ("nmixture", _re(True, True), P + _effects(True, True)),
    "occu_cs": ("occu_cs", {}, Ks + Ko + 6),
    "occu_re_site": ("occu_re", _re(True, False), P + _effects(True, False)),
    "occu_re_obs": ("occu_re", _re(False, True), P + _effects(False, True)),
    "occu_re_both": ("occu_re", _re(True, True), P + _effects(True, True)),
    "occu_re_both_rate": ("occu_re", _re(True, True, re_fp_mode="unoccupied"), P + 1 + _effects(True, True)),
    "occu_dyn": ("occu_dyn", {}, 3 * (Ks + 1) + Ko + 1),
    "occu_comb": ("occu_comb", {}, Ks + Ko + Ka + 9),
}
JOINT = ["occu", "occu_fp_constant", "occu_re_site", "occu_re_obs", "occu_re_both"]


def _spec(name):
    model, extras, _ = FORMS[name]
    return NS(model=model, extras=dict(extras), site_covs=np.zeros((N, Ks), np.float32), obs_covs=np.zeros((N, T, J, Ko), np.float32),
              shape=dict(S=1, N=N, T=T, J=J, Ks=Ks, Ko=Ko))


def _draws(rng, D, C=2, S=3):
    return rng.uniform(-4, 4, size=(C, S, D)).astype(np.float32)


@pytest.mark.parametrize("name", sorted(FORMS))
def test_width_is_the_closed_formula_and_blocks_tile_theta(name):
    lay = layout_for(_spec(name), **DIMS)
    assert lay.D == FORMS[name][2]
    at = 0
    for b in lay.blocks:   # one species: the blocks follow each other without gaps
        assert b.offset == at and b.width == int(np.prod([d for d in b.shape if d != PLATE], dtype=int))
        at += b.width
    assert at == lay.D


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("name", JOINT)
def test_joint_width_is_the_closed_formula(name, S):
    ex = FORMS[name][1]
    lay = layout_for(_spec(name), **DIMS, species_in_handle=S)
    assert lay.D == S * P + int(name.startswith("occu_fp")) + _effects(ex.get("site_random_effects", False), ex.get("obs_random_effects", False), S)
    with pytest.raises(NotImplementedError):
        layout_for(_spec("occu_rn"), **DIMS, species_in_handle=S)


def test_sites_are_the_expected_functions_of_literal_columns():
    """Ks = 1, Ko = 2: beta = columns 0-1, alpha = 2-4; everything behind that by hand."""
    rng = np.random.default_rng(1)
    sig, f64 = (lambda x: (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)), (lambda x: x.astype(np.float64))
    ex = lambda x: np.exp(f64(x)).astype(np.float32)

    # occu with a rate and both effects, two species' handles: [beta 0-1, alpha 2-4, phi 5, log site sd 6, log obs sd 7, occ 8-11, det 12-15, obs_re 16-39]
    lay = layout_for(_spec("occu_re_both_rate"), **DIMS)
    d = [_draws(rng, lay.D), _draws(rng, lay.D)]
    s = sites_from_draws(lay, d)
    assert list(s) == ["beta", "alpha", "prob_fp_unoccupied", "site_re_sd", "obs_re_sd", "site_re_occ", "site_re_det", "obs_re"]
    assert lay.fp_site == "prob_fp_unoccupied"
    for sp in range(2):
        assert np.array_equal(s["beta"][:, :, sp, :], d[sp][..., 0:2]) and np.array_equal(s["alpha"][:, :, sp, :], d[sp][..., 2:5])
        assert np.array_equal(s["site_re_occ"][..., sp], d[sp][..., 8:12]) and np.array_equal(s["site_re_det"][..., sp], d[sp][..., 12:16])
        for n in range(N):
            for t in range(T):
                for j in range(J):
                    assert np.array_equal(s["obs_re"][:, :, j, t, n, sp], d[sp][..., 16 + (n * T + t) * J + j])
    assert s["obs_re"].shape == (2, 3, J, T, N, 2) and s["obs_re"].flags["C_CONTIGUOUS"]
    # (shared sites: read from the first species' draws)
    assert np.array_equal(s["prob_fp_unoccupied"], sig(d[0][..., 5]))
    assert np.array_equal(s["site_re_sd"], ex(d[0][..., 6])) and np.array_equal(s["obs_re_sd"], ex(d[0][..., 7]))
    assert all(v.dtype == np.float32 for v in s.values())

    # the abundance models name the first site effect after their predictor; occu_cop's rate is exp(phi) and sits in front of the sds
    s = sites_from_draws(layout_for(_spec("nmixture_effects"), **DIMS), d[:1])
    assert "site_re_abu" in s and "site_re_occ" not in s and np.array_equal(s["site_re_abu"][..., 0], d[0][..., 7:11])   # (no phi: sds at 5, 6)
    lay = layout_for(_spec("occu_cop_rate_effects"), **DIMS)
    s = sites_from_draws(lay, d[:1])
    assert lay.fp_site == "rate_fp_unoccupied" and np.array_equal(s["rate_fp_unoccupied"], ex(d[0][..., 5]))
    assert np.array_equal(s["site_re_sd"], ex(d[0][..., 6])) and np.array_equal(s["site_re_occ"][..., 0], d[0][..., 8:12])
    s = sites_from_draws(layout_for(_spec("occu_fp_constant"), **DIMS), d[:1])
    assert np.array_equal(s["prob_fp_constant"], sig(d[0][..., 5])) and s["prob_fp_constant"].shape == (2, 3)

    # occu_cs: [beta, alpha, mu0 5, log(mu1 - mu0) 6, log sigma0 7, log sigma1 8], sites without a species axis
    s = sites_from_draws(layout_for(_spec("occu_cs"), **DIMS), d[:1])
    assert np.array_equal(s["mu0"], d[0][..., 5]) and np.array_equal(s["mu1"], (f64(d[0][..., 5]) + np.exp(f64(d[0][..., 6]))).astype(np.float32))
    assert np.array_equal(s["sigma0"], ex(d[0][..., 7])) and np.array_equal(s["sigma1"], ex(d[0][..., 8])) and np.all(s["mu1"] >= s["mu0"])

    # occu_dyn: [beta 0-1 | beta_col 2-3 | beta_ext 4-5 | alpha 6-8]
    s = sites_from_draws(layout_for(_spec("occu_dyn"), **DIMS), d[:1])
    assert [(k, v.shape) for k, v in s.items()] == [("beta", (2, 3, 1, 2)), ("beta_col", (2, 3, 1, 2)), ("beta_ext", (2, 3, 1, 2)), ("alpha", (2, 3, 1, 3))]
    assert np.array_equal(s["beta_col"][:, :, 0], d[0][..., 2:4]) and np.array_equal(s["beta_ext"][:, :, 0], d[0][..., 4:6]) and np.array_equal(s["alpha"][:, :, 0], d[0][..., 6:9])

    # occu_comb, Ka = 1: [beta 0-1 | alpha_PC 2-4 | alpha_ARU 5-6 | logit fc 7 | logit fu 8 | mu0 9 | log gap 10 | log sigma0 11 | log sigma1 12], per species
    s = sites_from_draws(layout_for(_spec("occu_comb"), **DIMS), d)
    for sp in range(2):
        assert np.array_equal(s["alpha_PC"][:, :, sp], d[sp][..., 2:5]) and np.array_equal(s["alpha_ARU"][:, :, sp], d[sp][..., 5:7])
        assert np.array_equal(s["ARU_prob_fp_constant"][..., sp], sig(d[sp][..., 7])) and np.array_equal(s["ARU_fp_unoccupied"][..., sp], sig(d[sp][..., 8]))
        assert np.array_equal(s["mu0"][..., sp], d[sp][..., 9])
        assert np.array_equal(s["mu1"][..., sp], (f64(d[sp][..., 9]) + np.exp(f64(d[sp][..., 10]))).astype(np.float32))
        assert np.array_equal(s["sigma0"][..., sp], ex(d[sp][..., 11])) and np.array_equal(s["sigma1"][..., sp], ex(d[sp][..., 12]))


def test_joint_blocks_sit_at_literal_offsets():
    """Two species, both effects: [sp 0: 0-4 | sp 1: 5-9 | log sds 10, 11 | occ [S][N] 12-19 | det [S][N] 20-27 | obs_re [S][N][T][J] 28-75]."""
    lay = layout_for(_spec("occu_re_both"), **DIMS, species_in_handle=2)
    jd = np.arange(lay.D, dtype=np.float32)[None, None, :]
    assert lay.D == 76
    one = species_block(lay, jd, 1)[0, 0]
    assert np.array_equal(one, np.r_[5:10, 10, 11, 16:20, 24:28, 52:76].astype(np.float32))
    assert np.array_equal(species_block(lay, jd, 0)[0, 0], np.r_[0:5, 10, 11, 12:16, 20:24, 28:52].astype(np.float32))
    # occu_fp: the shared rate rides along with every species
    lay = layout_for(_spec("occu_fp_constant"), **DIMS, species_in_handle=3)
    jd = np.arange(lay.D, dtype=np.float32)[None, None, :]
    assert np.array_equal(species_block(lay, jd, 2)[0, 0], np.r_[10:15, 15].astype(np.float32))


@pytest.mark.parametrize("name", sorted(FORMS))
def test_round_trip_draws_sites_draws(name):
    """draws -> sites -> draws: bit-equal on identity blocks; on transformed blocks within 1e-5 absolute for coordinates in [-4, 4] (the
    site is stored in float32, eps 6e-8, and the inverse logit amplifies by 1 / (p (1 - p)) <= 57 there: a 3x margin)."""
    rng = np.random.default_rng(2)
    lay = layout_for(_spec(name), **DIMS)
    nsp = 1 if name in ("occu_cs", "occu_dyn") else 2
    d = [_draws(rng, lay.D) for _ in range(nsp)]
    for b in lay.blocks:
        if not b.per_species:
            d[1:] = [np.concatenate([x[..., :b.offset], d[0][..., b.offset:b.offset + 1], x[..., b.offset + 1:]], axis=2) for x in d[1:]]   # shared across species
    sites = sites_from_draws(lay, d)
    posterior = {k: v.reshape((-1,) + v.shape[2:]) for k, v in sites.items()}
    for sp in range(nsp):
        back, x = draws_from_sites(lay, posterior, sp), d[sp].reshape(-1, lay.D)
        assert back.dtype == np.float32 and back.shape == x.shape and back.flags["C_CONTIGUOUS"]
        for b in lay.blocks:
            cols = slice(b.offset, b.offset + b.width)
            if b.transform == "identity":
                assert np.array_equal(back[:, cols], x[:, cols]), b.site
            else:
                assert np.max(np.abs(back[:, cols] - x[:, cols])) <= 1e-5, b.site
    if lay.fp_site:
        assert np.array_equal(fp_rate(lay, posterior).astype(np.float32), posterior[lay.fp_site])


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("name", JOINT)
def test_species_block_of_a_joint_draw_is_the_one_species_layout(name, S):
    """A joint draw assembled by hand from one-species draws (shared coordinates equal) splits back into exactly those."""
    rng = np.random.default_rng(3)
    one, joint = layout_for(_spec(name), **DIMS), layout_for(_spec(name), **DIMS, species_in_handle=S)
    assert [(b.site, b.width, b.shape, b.transform) for b in one.blocks] == [(b.site, b.width, b.shape, b.transform) for b in joint.blocks]
    d = [_draws(rng, one.D) for _ in range(S)]
    jd = np.full((2, 3, joint.D), np.nan, dtype=np.float32)
    for b1, bj in zip(one.blocks, joint.blocks):
        for sp in range(S if bj.per_species else 1):
            jd[..., bj.offset + sp * bj.stride: bj.offset + sp * bj.stride + bj.width] = d[sp][..., b1.offset: b1.offset + b1.width]
        if not bj.per_species:
            for x in d[1:]:
                x[..., b1.offset] = d[0][..., b1.offset]
    assert not np.isnan(jd).any()   # the joint blocks tile the joint theta
    for sp in range(S):
        assert np.array_equal(species_block(joint, jd, sp), d[sp])
    # two species jointly, site + obs effects: the sites of the split are the sites of the one-species handles
    a = sites_from_draws(one, [species_block(joint, jd, sp) for sp in range(S)])
    b = sites_from_draws(one, d)
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)


def _result(draws):
    C, S, D = draws.shape
    z = np.zeros
    return NutsResult(draws, z((C, S), bool), np.ones((C, S), np.int32), z((C, S), np.float32), z((C, S), np.float32), np.ones(C, np.float32),
                      np.ones((C, D), np.float32), z((C, 2), np.int64), 1.0, 4, 0, True)


@pytest.mark.parametrize("name", sorted(FORMS))
def test_assemblers_emit_the_layouts_sites(name):
    """fit's _assemble / _assemble_comb / _assemble_dyn on stub handles: the sampled sites are sites_from_draws', the deterministic ones
    stay lazy, and per-species results merge into one (draws side by side)."""
    rng = np.random.default_rng(4)
    spec, lay = _spec(name), layout_for(_spec(name), **DIMS)
    spec.extras.setdefault("ARU_obs_covs", np.zeros((N, T, 2, Ka), np.float32))
    ds = NS(**DIMS)
    nsp = 1 if name in ("occu_cs", "occu_dyn") else 2
    per = [(ds, _result(_draws(rng, lay.D))) for _ in range(nsp)]
    if name == "occu_dyn":
        mcmc = fit_module._assemble_dyn(per[0], spec, 5)
    elif name == "occu_comb":
        mcmc = fit_module._assemble_comb(per, spec, 5)
    else:
        mcmc = fit_module._assemble(per, spec, 5)
    want = sites_from_draws(lay, [r.draws for _, r in per])
    assert list(mcmc._latent) == list(want) and all(np.array_equal(mcmc._latent[k], want[k]) for k in want)
    assert mcmc._deterministic and all(callable(v) for v in mcmc._deterministic.values())
    assert mcmc.result.draws.shape == (2, 3, nsp * lay.D) and np.array_equal(mcmc.result.draws[..., :lay.D], per[0][1].draws)
    assert mcmc.result.inv_mass.shape == (2, nsp * lay.D)
