"""occu_dyn's three kernel forms (dyn_device.hpp) at their edges.  BUILDER-DEFINED MODEL, NO REFERENCE COUNTERPART: the ground truth is
the exact fixture tests/golden/dyn_exact.json (50-digit mpmath, tests/golden/make_dyn_exact.py) and the float64 oracle it certifies
(test_dyn_exact_cpu.py).

The host picks a form from the seasons T and the lanes per site pair G (dyn_lanes_per_pair: the largest power of two <= min(8, T) the
chain's lanes allow; BIOLITH_HIP_DYN_G forces it):
    two scans   bl_eval_sites_dyn_scan     T == G, T > 1          sampler tail ", true, 1, false>"  (", true, 2, false>" at 8 x 4 visits)
    scaled      bl_eval_sites_dyn_scaled   T <= 2 G otherwise     sampler tail ", true, -1, false>"
    first form  bl_eval_sites_dyn          T > 2 G                sampler tail ", false, -1, false>"
bl_logp_grad carries all three in one instantiation and branches on (T, G) at run time; the sampler has one instantiation per form and
compute-wave count.  Every case here states the form it is written for and asserts it: from (T, G) by the host's rule for bl_logp_grad,
from the launch's kernel_name for the sampler."""
import numpy as np
import pytest

import dyn_cases
import oracle
from biolith_amd.engine import OccuDataset
from parity import assert_potential_parity, describe_launch, potential_at_draws, potential_ratio, relative_excess
from test_gpu_sampler_density import RTOL

pytestmark = pytest.mark.gpu

KNOBS = ("BIOLITH_HIP_DYN_G", "BIOLITH_HIP_CWAVES", "BIOLITH_HIP_GENERAL")
TAILS = {", true, 1, false>": "scan", ", true, 2, false>": "scan", ", true, -1, false>": "scaled", ", false, -1, false>": "first"}

# rtol of the stored potential per form: |U_kernel - U_oracle| <= rtol |U_oracle| + ulp32 / 2 at every kept draw of the 60 + 60 runs
# below.  bl_logp_grad's bound is 1e-6; the measured maximum of (|dU| - ulp32 / 2) / |U| over the form's four cases (MI355X) stands beside it.
RTOL_FORM = {
    "scan": RTOL["dyn"],     # 1e-7; measured 8.98e-8 (4 compute waves, one workgroup: three rounds), 3.3e-8 on the host's three workgroups
    "scaled": RTOL["dyn"],   # 1e-7; measured 5.5e-8
    "first": RTOL["dyn"],    # 1e-7; measured 4.8e-8
}


def host_lanes_per_pair(N, T, chains=1):
    """dyn_lanes_per_pair (biolith_hip.hip) without the knob."""
    kmax = max(1, 32 // ((max(chains, 1) + 7) // 8))
    G = 1
    while 2 * G <= 8 and 2 * G <= T:
        G *= 2
    while G > 1 and ((N + 1) // 2) * G > kmax * 4 * 64:
        G //= 2
    return G


def form_of(T, G):
    return "scan" if (T == G and T > 1) else ("scaled" if T <= 2 * G else "first")


def launched(r):
    """(form, compute waves) of a sampler launch, from the instantiation it names."""
    name = r.kernel_name.rstrip()
    assert name.startswith("bl_nuts_kernel<") and name.split(",")[3].strip() == "8", name
    tail = [f for t, f in TAILS.items() if name.endswith(t)]
    assert len(tail) == 1, name
    return tail[0], int(name.split(",")[4])


def rounds_of(N, r):
    """Rounds of the site loop on the fullest workgroup of a launch, and its dead lane groups in the last one."""
    k, G, slots = r.wgs_per_chain, r.lane_group[0], (r.threads_per_wg // 64 - 1) * 64 // r.lane_group[0]
    npairs = ((N + k - 1) // k + 1) // 2
    rounds = (npairs + slots - 1) // slots
    return rounds, rounds * slots - npairs


def _clear(monkeypatch, **env):
    for var in KNOBS:
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, str(value))


def _assert_logp(label, Ug, Gg, U, G):
    """The project's bounds for this kernel: |dU| <= 1e-6 |U|, per theta row max |dgrad| <= 1e-5 max |grad|; everything finite."""
    assert np.all(np.isfinite(Ug)) and np.all(np.isfinite(Gg)), label
    dU = np.abs(Ug - U) / np.abs(U)
    dG = np.abs(Gg - G).max(1) / np.abs(G).max(1)
    print(f"\nDYNFORM {label} dU/|U|={dU.max():.3g} dgrad/max|grad|={dG.max():.3g}")
    assert np.all(dU <= 1e-6), (label, dU, Ug, U)
    assert np.all(dG <= 1e-5), (label, dG)


# ---------------------------------------------------------------- (a) bl_logp_grad against the exact fixture ----
@pytest.mark.parametrize("name", sorted(dyn_cases.SPECS))
def test_logp_grad_equals_the_exact_fixture(name, monkeypatch):
    """Every fixture case at the host's own G (eight sites: G = the largest power of two <= min(8, T)): two scans at T in {2, 4, 8},
    scaled at T in {1, 3, 5, 7, 9, 12, 15, 16}, first form at T = 17."""
    _clear(monkeypatch)
    X, W, Y, theta, kw, U, G = dyn_cases.load_exact(name)
    T = W.shape[1]
    lanes = host_lanes_per_pair(X.shape[0], T)
    assert form_of(T, lanes) == {1: "scaled", 2: "scan", 3: "scaled", 4: "scan", 5: "scaled", 7: "scaled", 8: "scan", 9: "scaled",
                                 12: "scaled", 15: "scaled", 16: "scaled", 17: "first"}[T]
    ds = OccuDataset(X, W, Y, model="occu_dyn", **kw)
    Ug, Gg = ds.logp_grad(theta.astype(np.float64))
    ds.close()
    _assert_logp(f"{name} T={T} G={lanes} {form_of(T, lanes)}", Ug, Gg, U, G)


FORCED = ([(T, T, "scan") for T in (2, 4, 8)]
          + [(T, G, "scaled") for T, G in ((1, 1), (1, 4), (2, 1), (3, 2), (3, 8), (7, 4), (8, 4), (9, 8), (15, 8), (16, 8))]
          + [(T, G, "first") for T, G in ((3, 1), (5, 2), (9, 4), (12, 4), (17, 8))])


@pytest.mark.parametrize("T,G,form", FORCED, ids=[f"T{T}-G{G}-{f}" for T, G, f in FORCED])
def test_logp_grad_equals_the_exact_fixture_at_forced_lanes(T, G, form, monkeypatch):
    """Each form at its boundaries, G forced: two scans at T = G; scaled at T = 2 G, at odd T (a lane's second period sub + G falls past
    T), at T < G (lanes without a period) and at one season; the first form from T = 2 G + 1 on.  Every fixture case of that T runs."""
    assert form_of(T, G) == form
    _clear(monkeypatch, BIOLITH_HIP_DYN_G=G)
    names = [n for n in sorted(dyn_cases.SPECS) if dyn_cases.SPECS[n][0] == T]
    assert names
    for name in names:
        X, W, Y, theta, kw, U, Gx = dyn_cases.load_exact(name)
        ds = OccuDataset(X, W, Y, model="occu_dyn", **kw)
        Ug, Gg = ds.logp_grad(theta.astype(np.float64))
        ds.close()
        _assert_logp(f"{name} T={T} G={G} {form}", Ug, Gg, U, Gx)


# ---------------------------------------------------------------- (b) more sites than one round ----
ROWS = ("bulk", "far", "sticky", "flip")
_tiled = {}


def tiled(N, T):
    """The fixture's data-edge pattern tiled to N sites (one visit per season, 1 + 1 covariates: 131 sites x 12 seasons fit one
    workgroup's LDS beside the model's scratch), the last site without data -- and the oracle's answers, computed once.  The oracle is
    certified on these inputs through the shared pattern and parameter rows (test_dyn_exact_cpu.py)."""
    if (N, T) not in _tiled:
        X, W, Y = dyn_cases.edge_dataset(100 * T + N, N, T, 1, 1, 1, last_site_empty=True)
        theta = dyn_cases.theta_rows(N + T, X, W, ROWS).astype(np.float64)
        od = oracle.OracleData(X, W, Y, model="occu_dyn")
        Uo, Go = od.potential_grad(theta)
        trees = oracle.nuts_run(od, 0, 4, num_chains=2, seed=N + T)
        _tiled[N, T] = (X, W, Y, theta, od, Uo, Go, trees)
    return _tiled[N, T]


# (T, G, form, whether one workgroup's LDS holds 131 sites' records beside the model's scratch)
ROUNDS = [(8, 8, "scan", True), (12, 8, "scaled", True), (17, 8, "first", False), (12, 4, "first", True)]


@pytest.mark.parametrize("N", [1, 2, 3, 49, 97, 131])
@pytest.mark.parametrize("T,G,form,one_wg", ROUNDS, ids=[f"T{T}-G{G}-{f}" for T, G, f, _ in ROUNDS])
def test_second_round_and_masked_groups(T, G, form, one_wg, N, monkeypatch):
    """Site loops with masked groups.  At G = 8 and three compute waves a workgroup has 24 slots: 97 sites on one workgroup are three
    rounds whose last holds ONE pair with a dummy second site beside 23 dead groups (which re-evaluate that pair with live = 0 and, in
    the two-scans form, still take part in the DPP steps); 49 sites are two rounds of the same kind; three workgroups give one round
    with dead groups.  bl_logp_grad (one round by construction) at the bounds of (a) against the oracle, then the sampler with
    wgs_per_chain 1 and 3: the first three trees are the oracle's and every stored potential is within bl_logp_grad's 1e-6.
    T = 17 at G = 8 cannot take a second round -- its lane-private columns leave room for 19 pairs' records, fewer than the 24
    slots, and the host raises the workgroups instead (choose_geometry) -- so the first form also runs at T = 12, G = 4 (48 slots:
    two rounds from 97 sites on)."""
    assert form_of(T, G) == form
    _clear(monkeypatch, BIOLITH_HIP_DYN_G=G)
    X, W, Y, theta, od, Uo, Go, o = tiled(N, T)
    ds = OccuDataset(X, W, Y, model="occu_dyn")
    Ug, Gg = ds.logp_grad(theta)
    _assert_logp(f"tiled N={N} T={T} G={G} {form}", Ug, Gg, Uo, Go)
    for k in (1, 3):
        r = ds.nuts(num_warmup=0, num_samples=4, num_chains=2, seed=N + T, wgs_per_chain=k)
        rounds, dead = rounds_of(N, r)
        print(f"DYNFORM rounds N={N} T={T} G={G} wgs_per_chain={k}->{r.wgs_per_chain} kernel={r.kernel_name!r} rounds={rounds} dead_groups={dead}")
        assert launched(r)[0] == form and r.lane_group[0] == G, (r.kernel_name, r.lane_group)
        if one_wg:
            assert r.wgs_per_chain == k and (k == 3 or N < 97 or rounds >= 2), (N, k, r.wgs_per_chain, rounds)
        assert np.array_equal(o["num_steps"][:, :3], r.num_steps[:, :3]), (k, o["num_steps"], r.num_steps)
        assert np.allclose(o["draws"][:, 0], r.draws[:, 0], atol=2e-3), k
        assert_potential_parity(r, potential_at_draws(od, r), 1e-6, f"tiled N={N} T={T} G={G} k={k}")
    ds.close()


# ---------------------------------------------------------------- (c) the sampler's instantiations ----
_sampler = {}


def sampler_case(form):
    """131 sites of the data-edge pattern at the host's own G = 8: T = 8 two scans, T = 12 scaled, T = 17 first form."""
    if form not in _sampler:
        T = {"scan": 8, "scaled": 12, "first": 17}[form]
        X, W, Y = dyn_cases.edge_dataset(40 + T, 131, T, 3, 2, 2, last_site_empty=True)
        od = oracle.OracleData(X, W, Y, model="occu_dyn")
        _sampler[form] = (X, W, Y, od, oracle.nuts_run(od, 0, 4, num_chains=2, seed=T))
    return _sampler[form]


@pytest.mark.parametrize("k", [1, 0])
@pytest.mark.parametrize("cw", [3, 4])
@pytest.mark.parametrize("form", ["scan", "scaled", "first"])
def test_sampler_instantiation(form, cw, k, monkeypatch):
    """Each form x {3, 4} compute waves x {one workgroup per chain as far as LDS allows, the host's choice}: the first three trees of
    two chains are the oracle's on the same streams, and over 60 + 60 transitions the potential stored at every kept draw equals the
    oracle's at that draw to RTOL_FORM."""
    _clear(monkeypatch, BIOLITH_HIP_CWAVES=cw)
    X, W, Y, od, o = sampler_case(form)
    T = W.shape[1]
    ds = OccuDataset(X, W, Y, model="occu_dyn")
    r = ds.nuts(num_warmup=0, num_samples=4, num_chains=2, seed=T, wgs_per_chain=k)
    assert launched(r) == (form, cw), r.kernel_name
    assert np.array_equal(o["num_steps"][:, :3], r.num_steps[:, :3]), (o["num_steps"], r.num_steps)
    assert np.allclose(o["draws"][:, 0], r.draws[:, 0], atol=2e-3)
    r = ds.nuts(num_warmup=60, num_samples=60, num_chains=2, seed=3, wgs_per_chain=k)
    f = describe_launch(ds)
    assert launched(r) == (form, cw) and f["kernel"] == r.kernel_name
    Uo = potential_at_draws(od, r)
    rtol = RTOL_FORM[form]
    print(f"\nDYNFORM sampler form={form} cw={cw} wgs_per_chain={k}->{r.wgs_per_chain} rtol={rtol:g} "
          f"worst_ratio={float(np.max(potential_ratio(r.potential_energy, Uo, rtol))):.3g} rel_excess={relative_excess(r.potential_energy, Uo):.3g} "
          f"kernel={r.kernel_name!r} lane_group={r.lane_group} rounds={rounds_of(131, r)}")
    assert_potential_parity(r, Uo, rtol, f"{form} cw={cw} k={k}")
    ds.close()


@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_same_trees_at_every_lanes_per_pair(G, monkeypatch):
    """One dataset (T = 8) and seed under G = 1, 2 (first form), 4 (scaled), 8 (two scans): the oracle's first three trees every time."""
    _clear(monkeypatch, BIOLITH_HIP_DYN_G=G)
    X, W, Y, od, o = sampler_case("scan")
    ds = OccuDataset(X, W, Y, model="occu_dyn")
    r = ds.nuts(num_warmup=0, num_samples=4, num_chains=2, seed=8)
    print(f"\nDYNFORM lanes G={G} kernel={r.kernel_name!r} wgs_per_chain={r.wgs_per_chain}")
    assert r.lane_group[0] == G and launched(r)[0] == {1: "first", 2: "first", 4: "scaled", 8: "scan"}[G], (r.kernel_name, r.lane_group)
    assert np.array_equal(o["num_steps"][:, :3], r.num_steps[:, :3]), (o["num_steps"], r.num_steps)
    assert np.allclose(o["draws"][:, 0], r.draws[:, 0], atol=2e-3)
    ds.close()
