"""site_summary's definition in NumPy on predict()'s arrays, the host's rank and interpolation rule restated, and the bounds of the
comparison -- shared by tests/test_site_summary_cpu.py and tests/test_gpu_site_summary.py.

The definition, for a float32 array ``v32`` with the draws on axis 0 and ``v = v32.astype(float64)``:
    mean = v.mean(0);   sd = v.std(0, ddof=1) (NaN for one draw);   quantiles = np.quantile(v, probs, axis=0)   (method "linear")
    order[r] = np.sort(v32, axis=0)[ranks[r]], bit for bit

Bounds (derived, not tuned; the inputs are bit-equal to predict()'s float32 values):
    mean       rtol 1e-12: the order of at most ~1100 float64 additions, (n - 1) 2^-53 ~ 1.2e-13, with a margin of 8
    sd         |got - want| <= 1e-10 want + 1e-14 max(1, |mean|): the two-pass M2 has relative error ~ n 2^-52, the mean's error enters
               at second order; the absolute term covers cells whose n values are all equal
    order      exact
    quantiles  |got - want| <= 2e-15 max(1, |want|): NumPy's lerp and a + (b - a) g differ by one rounding
"""
import warnings

import numpy as np

WORST = {"mean": 0.0, "sd": 0.0, "quantiles": 0.0}   # the largest error seen, as a fraction of its bound (printed by every check)


def reference(v32, probs):
    """mean, sd, quantiles of the definition; ``v32`` (n, ...) float32."""
    v32 = np.asarray(v32)
    assert v32.dtype == np.float32
    v = v32.astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (one draw: ddof = 1 divides 0 by 0, which is the definition's NaN)
        sd = v.std(0, ddof=1)
    return v.mean(0), sd, np.quantile(v, np.asarray(probs, dtype=np.float64), axis=0)


def order_reference(v32, ranks):
    """The float32 values of ``ranks`` in the sorted order of every cell's draws -> (len(ranks), ...)."""
    v32 = np.asarray(v32)
    assert v32.dtype == np.float32
    return np.sort(v32, axis=0)[np.asarray(ranks, dtype=np.int64)]


def host_ranks(probs, n):
    """The host's rule, restated: lo = floor((n - 1) q), hi = min(lo + 1, n - 1), the weight g = (n - 1) q - lo, and the distinct ranks."""
    lo, hi, g = [], [], []
    for q in np.asarray(probs, dtype=np.float64).reshape(-1):
        pos = (n - 1) * float(q)
        a = min(int(np.floor(pos)), n - 1)
        lo.append(a); hi.append(min(a + 1, n - 1)); g.append(pos - a)
    return np.array(lo), np.array(hi), np.array(g), np.array(sorted(set(lo) | set(hi)))


def host_quantiles(v32, probs):
    """The quantiles as the host forms them: the two order statistics of the float32 values, a + (b - a) g in float64."""
    s = np.sort(np.asarray(v32), axis=0).astype(np.float64)
    lo, hi, g, _ = host_ranks(probs, s.shape[0])
    return np.stack([s[a] + (s[b] - s[a]) * w for a, b, w in zip(lo, hi, g)])


def check(got, v32, probs, label=""):
    """One site's ``{"mean", "sd", "quantiles"}`` (any shape that broadcasts from the definition's) against the definition at the bounds
    of the module's docstring; prints the largest errors as fractions of their bounds."""
    mean, sd, quant = reference(v32, probs)
    n = np.asarray(v32).shape[0]
    for k, want in (("mean", mean), ("sd", sd), ("quantiles", quant)):
        assert got[k].dtype == np.float64 and got[k].shape == want.shape, (label, k, got[k].shape, want.shape)
    e_mean = np.abs(got["mean"] - mean)
    b_mean = 1e-12 * np.abs(mean)
    e_q = np.abs(got["quantiles"] - quant)
    b_q = 2e-15 * np.maximum(1.0, np.abs(quant))
    if n > 1:
        e_sd = np.abs(got["sd"] - sd)
        b_sd = 1e-10 * sd + 1e-14 * np.maximum(1.0, np.abs(mean))
    else:
        assert np.isnan(got["sd"]).all(), label
        e_sd, b_sd = np.zeros(1), np.ones(1)
    frac = {"mean": float(np.max(e_mean / np.where(b_mean > 0, b_mean, 1.0), initial=0.0)), "sd": float(np.max(e_sd / b_sd, initial=0.0)),
            "quantiles": float(np.max(e_q / b_q, initial=0.0))}
    for k, f in frac.items():
        WORST[k] = max(WORST[k], f)
    print(f"{label:44s} n {n:5d} cells {mean.size:7d}  of its bound: mean {frac['mean']:.2e}  sd {frac['sd']:.2e}  quantiles {frac['quantiles']:.2e}"
          f"   (worst so far {WORST['mean']:.2e} {WORST['sd']:.2e} {WORST['quantiles']:.2e})")
    assert np.all(e_mean <= b_mean), f"mean {label}"
    assert np.all(e_sd <= b_sd), f"sd {label}"
    assert np.all(e_q <= b_q), f"quantiles {label}"
