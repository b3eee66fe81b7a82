"""Named occu_dyn cases shared by the exact fixture (tests/golden/make_dyn_exact.py -> tests/golden/dyn_exact.json), the CPU tests that
pin the oracle to it (test_dyn_exact_cpu.py) and the GPU tests of the kernel's three forms (test_gpu_dyn_forms.py) (TEST INFRASTRUCTURE).

Every array is float32 and comes from a seeded NumPy generator; the fixture stores the SHA-256 of their bytes, so a case that drifts
from what the fixture was computed for fails instead of being compared with numbers that belong to other data.

A case is (X (N, Ks), W (N, T, J, Ko), Y (1, N, T, J), theta rows (R, D), dataset kwargs), theta = [b_psi | b_gamma | b_eps | alpha]."""
import hashlib
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dyn_exact.json")
MAX_SITE_LOGIT = 16.0   # the condition under which the float64 oracle is certified against the exact statement
PATTERNS = 8            # the data-edge pattern repeats every eight sites


def edge_dataset(seed, N, T, J, Ks, Ko, last_site_empty=False):
    """Site i carries data edge i % 8:
    0 one visit missing (and one NaN observation covariate);  1 the first and the last season unobserved;  2 a middle season unobserved;
    3 no data at all;  4 a NaN site covariate (the site is masked);  5 detected at every visit of every season;  6 never detected;
    7 detections alternate season by season (a detection forces z = 1, so every path pays transitions)."""
    rng = np.random.default_rng(seed)
    scale = 0.7 if max(Ks, Ko) <= 4 else 0.35   # (many covariates: the linear predictors stay in range)
    X = (rng.normal(size=(N, Ks)) * scale).astype(np.float32)
    W = (rng.normal(size=(N, T, J, Ko)) * scale).astype(np.float32)
    Y = (rng.uniform(size=(N, T, J)) < 0.4).astype(np.float32)
    for i in range(N):
        e = i % PATTERNS
        if e == 0:
            Y[i, min(1, T - 1), J - 1] = np.nan
            if Ko:
                W[i, T - 1, 0, Ko - 1] = np.nan
        elif e == 1:
            Y[i, 0] = np.nan
            Y[i, T - 1] = np.nan
        elif e == 2:
            Y[i, T // 2] = np.nan
        elif e == 3:
            Y[i] = np.nan
        elif e == 4 and Ks:
            X[i, Ks - 1] = np.nan
        elif e == 5:
            Y[i] = 1.0
        elif e == 6:
            Y[i] = 0.0
        elif e == 7:
            Y[i, 0::2] = 1.0
            Y[i, 1::2] = 0.0
    if last_site_empty:
        Y[N - 1] = np.nan
    return X, W, Y[None]


def site_logits(X, theta):
    """|logit psi|, |logit gamma|, |logit eps| of every site: (R, 3, N), float64 of the float32 values (NaN covariates count as 0)."""
    Xc = np.nan_to_num(np.asarray(X, dtype=np.float64))
    B = X.shape[1] + 1
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    blocks = th[:, :3 * B].reshape(-1, 3, B)
    return np.abs(blocks[:, :, :1] + blocks[:, :, 1:] @ Xc.T)


def visit_logits(X, W, theta):
    """|logit p| of every visit: (R, N, T, J)."""
    Wc = np.nan_to_num(np.asarray(W, dtype=np.float64))
    al = np.atleast_2d(np.asarray(theta, dtype=np.float64))[:, 3 * (X.shape[1] + 1):]
    return np.abs(al[:, None, None, None, 0] + np.einsum("ntjk,rk->rntj", Wc, al[:, 1:]))


def theta_rows(seed, X, W, kinds):
    """One float32 row per kind:
    bulk    U(-1.5, 1.5);                         far     three times that;
    sticky  psi ~ 1, gamma ~ eps ~ 1e-3;          flip    psi ~ 1, gamma ~ eps ~ 1 - 1e-3;
    det12   bulk with detection logits out to +-12 (alpha_1 alone, sized by the largest first observation covariate).
    A row whose largest site logit would pass 15 has its site-side blocks scaled back to 15: MAX_SITE_LOGIT holds for every row."""
    rng = np.random.default_rng(seed)
    Ks, Ko = X.shape[1], W.shape[3]
    B = Ks + 1
    D = 3 * B + Ko + 1
    rows = []
    for kind in kinds:
        th = rng.uniform(-1.5, 1.5, size=D)
        if kind == "far":
            th *= 3.0
        elif kind in ("sticky", "flip"):
            th[:3 * B] *= 0.2
            th[[0, B, 2 * B]] = [6.0, -7.0, -7.0] if kind == "sticky" else [6.0, 7.0, 7.0]
        elif kind == "det12":
            assert Ko >= 1
            th[3 * B:] = 0.0
            th[3 * B + 1] = 12.0 / float(np.nanmax(np.abs(W[..., 0])))
        else:
            assert kind == "bulk", kind
        worst = float(site_logits(X, th).max())
        if worst > 15.0:
            th[:3 * B] *= 15.0 / worst
        rows.append(th)
    th = np.asarray(rows).astype(np.float32)
    assert site_logits(X, th).max() <= MAX_SITE_LOGIT
    return th


# name -> (T, J, Ks, Ko, theta kinds, dataset kwargs); eight sites each.  Every T, J and (Ks, Ko) of the matrix appears:
# T in {1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17}, J in {1, 3, 4, 9}, (Ks, Ko) in {(0, 0), (1, 1), (3, 3), (4, 4), (5, 2), (8, 16), (2, 9)}
ALL = ("bulk", "far", "sticky", "flip")
SPECS = {
    "t1": (1, 3, 1, 1, ALL, {}),
    "t2": (2, 4, 0, 0, ALL, {}),
    "t3": (3, 1, 3, 3, ALL, {}),
    "t4": (4, 9, 1, 1, ALL, {}),
    "t5": (5, 3, 4, 4, ALL, {}),
    "t7": (7, 4, 5, 2, ALL, {}),
    "t8": (8, 4, 3, 3, ALL + ("det12",), {}),
    "t9": (9, 3, 2, 9, ("bulk", "far", "sticky"), {}),
    "t12": (12, 1, 1, 1, ALL, {}),
    "t15": (15, 3, 3, 3, ("bulk", "far", "flip"), {}),
    "t16": (16, 4, 0, 0, ALL, {}),
    "t17": (17, 3, 1, 1, ALL, {}),
    "cap_8_16": (4, 3, 8, 16, ("bulk", "sticky"), {}),
    "cap_8_16_t9": (9, 1, 8, 16, ("bulk", "flip"), {}),
    "t3_k29": (3, 4, 2, 9, ("bulk", "far", "det12"), {}),
    "t5_k00_j9": (5, 9, 0, 0, ALL, {}),
    "t7_k33_j1": (7, 1, 3, 3, ALL, {}),
    "t8_k44_j9": (8, 9, 4, 4, ("bulk", "far", "sticky", "det12"), {}),
    "t8_k52": (8, 3, 5, 2, ALL, {}),
    "t9_k11_j4": (9, 4, 1, 1, ALL, {}),
    "t12_k33_j9": (12, 9, 3, 3, ("bulk", "far", "sticky"), {}),
    "t16_k52_j1": (16, 1, 5, 2, ("bulk", "flip"), {}),
    "t17_k44_j4": (17, 4, 4, 4, ("bulk", "far", "sticky"), {}),
    "priors": (5, 3, 1, 1, ("bulk", "far"), dict(prior_beta=(0.1, 1.5), prior_alpha=(-0.2, 0.7))),
}
REGENERATED = ("t2", "t5", "priors")   # the cases test_dyn_exact_cpu.py recomputes in mpmath where it is installed


def build(name):
    T, J, Ks, Ko, kinds, kw = SPECS[name]
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)   # (its own name: adding a case leaves the others' arrays alone)
    X, W, Y = edge_dataset(seed, 8, T, J, Ks, Ko)
    return X, W, Y, theta_rows(seed + 500, X, W, kinds), dict(kw)


def digests(X, W, Y, theta):
    """SHA-256 of the float32 bytes of each array (NaNs are the generator's own quiet NaN: one bit pattern)."""
    out = {}
    for key, a in (("X", X), ("W", W), ("Y", Y), ("theta", theta)):
        a = np.ascontiguousarray(a)
        assert a.dtype == np.float32, (key, a.dtype)
        out[key] = hashlib.sha256(a.tobytes()).hexdigest()
    return out


def load_exact(name):
    """The fixture's rows of a case as float64 arrays (U (R,), grad (R, D)), after checking that the case is the one they were computed for.
    A mismatch is an error, never a skip."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    X, W, Y, theta, kw = build(name)
    entry = fx["cases"][name]
    assert entry["sha256"] == digests(X, W, Y, theta), f"{name}: the case's arrays are not the ones dyn_exact.json was computed for"
    U = np.array([float(r["U"]) for r in entry["rows"]])
    G = np.array([[float(g) for g in r["grad"]] for r in entry["rows"]])
    assert U.shape == (theta.shape[0],) and G.shape == theta.shape
    return X, W, Y, theta, kw, U, G
