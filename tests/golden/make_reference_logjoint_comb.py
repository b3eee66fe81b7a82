#!/usr/bin/env python3
"""Generate tests/golden/reference_logjoint_comb_<case>.json by EXECUTING the reference's occu_comb (build container only).

The model text that runs is the reference's own ``biolith.models.occu_comb`` (occu_comb.py:150-349), under the functional NumPy shim of
make_reference_logjoint.py (imported, not copied), which this script extends by the two distributions occu_comb needs beyond it:

* ``Gamma(concentration, rate)`` on the positive reals (sampled on the log scale, log-Jacobian u);
* ``TruncatedDistribution(base, low=l)`` of a Normal base: log_prob = base.log_prob(v) - log(1 - Phi((l - loc) / scale)) on (l, inf),
  sampled as v = l + exp(u) (numpyro's ``biject_to(greater_than(l))``), log-Jacobian u.

Assumptions (1)-(6) of make_reference_logjoint.py apply unchanged.  The potential is cross-checked by a second contraction that runs
the model body once per VALUE of z and ``logsumexp``s the per-(site, period) sums of EVERY observed site inside z's plates (y_pc,
y_aru, scores) afterwards.  Only DATA is written: the simulator's kwargs (the data are simulate_comb's, bit-identical to the
reference's), the SHA-256 of the data arrays, the priors, flat parameter vectors in the engine's order
[beta | alpha_PC | alpha_ARU | logit fc | logit fu | mu0 | log(mu1 - mu0) | log sigma0 | log sigma1], the potential U at each and a
central-difference gradient of U.  The case index is reference_logjoint_comb_index.json (the occu index is left as it is).

Run:  python tests/golden/make_reference_logjoint_comb.py      (needs the reference; never run on the GPU box)
"""
import contextlib
import io
import json
import math
import os
import sys
from collections import OrderedDict

import numpy as np
from scipy import special as sps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_reference_logjoint as mrl  # noqa: E402


class Gamma(mrl.Distribution):
    support = "positive"

    def __init__(self, concentration, rate=1.0):
        self.a, self.b = mrl._f(concentration), mrl._f(rate)
        self.batch_shape = np.broadcast_shapes(self.a.shape, self.b.shape)

    def log_prob(self, v):
        return self.a * np.log(self.b) - sps.gammaln(self.a) + (self.a - 1.0) * np.log(v) - self.b * v


class TruncatedDistribution(mrl.Distribution):
    def __init__(self, base, low=None, high=None):
        assert isinstance(base, mrl.Normal) and type(base) is mrl.Normal and high is None and low is not None
        self.base, self.low = base, mrl._f(low)
        self.support = ("greater_than", self.low)
        self.batch_shape = np.broadcast_shapes(base.batch_shape, self.low.shape)

    def log_prob(self, v):
        z = (self.low - self.base.loc) / self.base.scale
        lp = self.base.log_prob(v) - np.log(0.5 * sps.erfc(z / math.sqrt(2.0)))
        return np.where(v > self.low, lp, -np.inf)


_constrain0 = mrl._constrain


def _constrain(fn, u):
    if isinstance(fn.support, tuple) and fn.support[0] == "greater_than":
        u = np.asarray(u, dtype=np.float64)
        return fn.support[1] + np.exp(u), float(np.sum(u))
    return _constrain0(fn, u)


mrl._constrain = _constrain
_modules0 = mrl._functional_modules


def _functional_modules():
    mods = _modules0()
    mods["numpyro.distributions"].__dict__.update(Gamma=Gamma, TruncatedDistribution=TruncatedDistribution)
    return mods


mrl._functional_modules = _functional_modules
PRIORS = dict(Normal=mrl.Normal, Laplace=mrl.Laplace, Beta=mrl.Beta, Gamma=Gamma)

# case -> (simulate_comb kwargs, model priors as [family, parameters...] or pairs of them, theta regime)
CASES = OrderedDict([
    ("comb_default", (dict(), dict(), "uniform")),
    ("comb_missing", (dict(simulate_missing=True), dict(), "uniform")),
    ("comb_missing_3periods", (dict(simulate_missing=True, n_periods=3, n_sites=60), dict(), "uniform")),
    # point-count detections at sites of tiny psi: the z = 0 branch pays log(tiny) per detection (numpyro's clamp_probs)
    ("comb_clamp", (dict(n_sites=50, ARU_prob_fp_constant=0.05, ARU_prob_fp_unoccupied=0.1, random_seed=4), dict(), "low_psi")),
    ("comb_laplace", (dict(n_sites=60, n_site_covs=2, n_PC_covs=2, n_ARU_covs=3, simulate_missing=True, random_seed=6),
                      dict(prior_beta=["Laplace", 0.2, 1.5], prior_alpha=["Laplace", -0.1, 0.8],
                           prior_ARU_prob_fp_constant=["Beta", 3.0, 4.0], prior_ARU_prob_fp_unoccupied=["Beta", 1.5, 6.0],
                           prior_mu=[["Normal", -1.0, 4.0], ["Normal", 2.0, 6.0]], prior_sigma=[["Gamma", 4.0, 1.5], ["Gamma", 6.0, 2.0]]),
                      "uniform")),
])


def materialise(pri):
    def one(v):
        return PRIORS[v[0]](*v[1:])
    out = {}
    for k, v in pri.items():
        out[k] = tuple(one(x) for x in v) if isinstance(v[0], list) else one(v)
    return out


def model_args(data, pri):
    a = {k: mrl.f32(data[k]) for k in ("site_covs", "PC_obs_covs", "ARU_obs_covs", "scores_obs", "PC_obs", "ARU_obs")}
    a.update(materialise(pri))
    return a


def unconstrained(th, Ks, Kp, Ka):
    o = Ks + Kp + Ka + 3
    return OrderedDict(beta=th[None, :Ks + 1], alpha_PC=th[None, Ks + 1: Ks + Kp + 2], alpha_ARU=th[None, Ks + Kp + 2: o],
                       ARU_prob_fp_constant=th[o: o + 1], ARU_fp_unoccupied=th[o + 1: o + 2], mu0=th[o + 2: o + 3],
                       mu1=th[o + 3: o + 4], sigma0=th[o + 4: o + 5], sigma1=th[o + 5: o + 6])


def log_joint_by_value(model_fn, args, u):
    """No enumeration axis: the body once per value of z, the observed sites inside z's plates summed over their other plates."""
    per_value, fixed_total, jac = [], None, None
    for v in (0, 1):
        t = mrl.run_model(model_fn, args, u, enum=("fixed", v))
        zp = t["z"]["plates"]
        acc, fixed, j = 0.0, 0.0, 0.0
        for name, s in t.items():
            if s["kind"] != "sample":
                continue
            j += s["log_jac"]
            lp = s["log_prob"]
            if name == "z" or (s.get("observed") and set(zp) <= set(s["plates"])):
                extra = tuple(d for d in s["plates"] if d not in zp)
                acc = acc + (lp.sum(axis=extra) if extra else lp)
            else:
                fixed += float(np.sum(lp))
        per_value.append(acc)
        if fixed_total is None:
            fixed_total, jac = fixed, j
        else:
            assert abs(fixed - fixed_total) <= 1e-9 * max(1.0, abs(fixed_total)), (fixed, fixed_total)
    return fixed_total + float(np.sum(sps.logsumexp(np.stack(per_value), axis=0))), jac


def main():
    mrl.load_reference()
    model_fn = sys.modules["biolith.models.occu_comb"].occu_comb
    from biolith_amd.models import simulate_comb

    index = OrderedDict()
    for case, (skw, pri, regime) in CASES.items():
        with contextlib.redirect_stdout(io.StringIO()):
            data, truth = simulate_comb(**skw)
        args = model_args(data, pri)
        Ks, Kp, Ka = data["site_covs"].shape[1], data["PC_obs_covs"].shape[3], data["ARU_obs_covs"].shape[3]
        D = Ks + Kp + Ka + 9
        rng = np.random.default_rng(len(index) + 100)
        points = []
        for p in range(3):
            th = np.empty(D)
            th[:D - 6] = rng.uniform(-1.0, 1.0, size=D - 6)
            th[D - 6:] = np.array([-1.2, -1.5, -2.0, math.log(5.0), math.log(4.5), math.log(3.0)]) + rng.uniform(-0.4, 0.4, size=6)
            if regime == "low_psi":
                th[0] = -9.0 - p
            th = th.astype(np.float32).astype(np.float64)

            def U(x):
                return mrl.potential(model_fn, args, unconstrained(x, Ks, Kp, Ka))

            u0 = U(th)
            lj, jac = log_joint_by_value(model_fn, args, unconstrained(th, Ks, Kp, Ka))
            assert abs(-(lj + jac) - u0) <= 1e-9 * abs(u0), (case, u0, -(lj + jac))
            h, g = 1e-5, np.empty(D)
            for d in range(D):
                e = np.zeros(D)
                e[d] = h
                g[d] = (8 * (U(th + e) - U(th - e)) - (U(th + 2 * e) - U(th - 2 * e))) / (12 * h)
            points.append(dict(theta=th.tolist(), U=u0, grad_U_central_difference=g.tolist()))
        entry = dict(case=case, simulate_kwargs=skw, priors=pri, D=D,
                     data_sha={k: mrl.sha(data[k]) for k in ("site_covs", "PC_obs_covs", "ARU_obs_covs", "PC_obs", "ARU_obs", "scores_obs")},
                     points=points)
        with open(os.path.join(HERE, f"reference_logjoint_{case}.json"), "w") as f:
            json.dump(entry, f)
        index[case] = dict(file=f"reference_logjoint_{case}.json", D=D)
        print(case, [round(p["U"], 6) for p in points])
    with open(os.path.join(HERE, "reference_logjoint_comb_index.json"), "w") as f:
        json.dump(index, f, indent=1)


if __name__ == "__main__":
    main()
