"""The ORDER of ``response_curves``' reduction in NumPy -- not the model: given the per-site float64 terms, the sum as the device
forms it (``bl_response_curves`` in include/biolith_hip.h, ``bl_regional_totals``' order for a single region).

The sites in site order are cut into runs of 64, the last run filled up with -0.0 (the identity of the float64 sum); a run is summed as
the tree ``a[:, :32] + a[:, 32:]``, then halves down to one column; the runs' sums are added left to right.  Every step is one IEEE
float64 addition on both sides, so together with the terms --

    site side   w_i * (double) v_i                      v_i the float32 of ``deterministic`` on the modified covariates
    obs side    w_i * (sequential float64 sum over the visits v = t J + j of (double) u_{v,i}, from the first term on)

-- it predicts the output byte for byte: no tolerance."""
import numpy as np

U = 2.0 ** -53


def ordered_sum(terms):
    """``terms`` (..., N) float64 -> (...,) float64: the device's sum over the last axis, addition by addition."""
    t = np.asarray(terms, dtype=np.float64)
    lead, N = t.shape[:-1], t.shape[-1]
    assert N >= 1
    runs = (N + 63) // 64
    a = np.full(lead + (runs * 64,), -0.0)
    a[..., :N] = t
    a = a.reshape(lead + (runs, 64))
    width = 64
    while width > 1:
        width //= 2
        a = a[..., :width] + a[..., width:]
    a = a[..., 0]                      # (..., runs)
    out = a[..., 0].copy()
    for r in range(1, runs):
        out = out + a[..., r]
    return out


def site_terms(v, weight=None):
    """``v`` (..., N) float32 -> the site side's terms ``w_i * (double) v_i``."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    w = np.ones(v.shape[-1]) if weight is None else np.asarray(weight, dtype=np.float64)
    return w * v.astype(np.float64)


def obs_terms(u, weight=None):
    """``u`` (n, J, T, N) float32, ``deterministic``'s layout -> the obs side's terms (n, N): the weight times the float64 sum over the
    visits in ascending v = t J + j, one addition at a time from the first term on."""
    u = np.asarray(u)
    assert u.dtype == np.float32 and u.ndim == 4
    n, J, T, N = u.shape
    by_visit = np.transpose(u, (0, 2, 1, 3)).reshape(n, T * J, N).astype(np.float64)
    s = by_visit[:, 0].copy()
    for v in range(1, T * J):
        s = s + by_visit[:, v]
    w = np.ones(N) if weight is None else np.asarray(weight, dtype=np.float64)
    return w * s


def bound(terms):
    """Within which two float64 sums of the same N terms agree, each in an order of its own: ``2 (N - 1) 2^-53 sum |terms|``
    (derived in tests/totals_ref.py)."""
    t = np.asarray(terms, dtype=np.float64)
    return 2.0 * max(t.shape[-1] - 1, 0) * U * np.sum(np.abs(t), axis=-1)
