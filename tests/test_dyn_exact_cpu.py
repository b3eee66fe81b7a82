"""The float64 oracle of occu_dyn (BUILDER-DEFINED, no reference counterpart) against an EXACT statement of the model: 50-digit mpmath,
the 2^T paths summed by brute force and by the linear-space forward product, the gradient by central differences at h = 1e-20
(tests/golden/make_dyn_exact.py -> tests/golden/dyn_exact.json).  test_dyn_cpu.py pins the oracle to a float64 literal, which itself
loses 2.5e-8 .. 6e-2 of U once the coefficients leave |theta| <= 2 (it takes log of a rounded sigmoid); this fixture reaches transition
probabilities of 1e-3 and 1 - 1e-3, seasons forced occupied by a detection, seventeen seasons and detection logits of +-12 -- under the
one condition that no site logit passes 16, where 1 - psi starts to round in float64 (dyn_cases.MAX_SITE_LOGIT)."""
import importlib.util
import json
import os

import numpy as np
import pytest

import dyn_cases
import oracle


def _oracle(X, W, Y, kw):
    return oracle.OracleData(X, W, Y, model="occu_dyn", **kw)


@pytest.mark.parametrize("name", sorted(dyn_cases.SPECS))
def test_oracle_equals_the_exact_fixture(name):
    """|dU| <= 1e-10 max(1, |U|), max |dgrad| <= 1e-9 max(1, max |grad|) per theta row (measured: 2e-15 for both)."""
    X, W, Y, theta, kw, U, G = dyn_cases.load_exact(name)
    od = _oracle(X, W, Y, kw)
    assert od.D == theta.shape[1]
    Uo, Go = od.potential_grad(theta.astype(np.float64))
    dU = np.abs(Uo - U) / np.maximum(1.0, np.abs(U))
    dG = np.abs(Go - G).max(1) / np.maximum(1.0, np.abs(G).max(1))
    print(f"\nEXACT {name} shape={X.shape[0], W.shape[1], W.shape[2], X.shape[1], W.shape[3]} dU={dU.max():.3g} dgrad={dG.max():.3g}")
    assert np.all(dU <= 1e-10), (name, dU)
    assert np.all(dG <= 1e-9), (name, dG)


def test_fixture_covers_the_matrix():
    """The shapes, capacities and parameter regimes the fixture is there for are in it, and every row is inside the certified range."""
    with open(dyn_cases.FIXTURE) as f:
        fx = json.load(f)
    assert sorted(fx["cases"]) == sorted(dyn_cases.SPECS)
    shapes = [tuple(c["shape"]) for c in fx["cases"].values()]
    assert {s[1] for s in shapes} >= {1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17}
    assert {s[2] for s in shapes} >= {1, 3, 4, 9}
    assert {s[3:] for s in shapes} >= {(0, 0), (1, 1), (3, 3), (4, 4), (5, 2), (8, 16), (2, 9)}
    rows = [r for c in fx["cases"].values() for r in c["rows"]]
    assert max(r["max_site_logit"] for r in rows) <= dyn_cases.MAX_SITE_LOGIT
    assert max(r["max_visit_logit"] for r in rows) >= 11.9          # the detection logits of +-12
    assert any(k.get("prior_beta") not in (None, (0.0, 1.0)) for *_, k in dyn_cases.SPECS.values())
    assert os.path.getsize(dyn_cases.FIXTURE) < 200 * 1024


def test_fixture_regenerates_to_the_committed_strings():
    """Three cases recomputed in mpmath equal the committed decimal strings (a machine without mpmath skips this one only)."""
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_dyn_exact", os.path.join(os.path.dirname(dyn_cases.FIXTURE), "make_dyn_exact.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(dyn_cases.FIXTURE) as f:
        fx = json.load(f)
    for name in dyn_cases.REGENERATED:
        assert json.loads(gen.dumps(gen.entry(name))) == fx["cases"][name], name
