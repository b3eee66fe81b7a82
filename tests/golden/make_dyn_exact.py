"""Writes tests/golden/dyn_exact.json: occu_dyn's potential U = -log p(theta, y) and its gradient at the cases of tests/dyn_cases.py,
stated in mpmath at 50 digits (TEST INFRASTRUCTURE; BUILDER-DEFINED MODEL, NO REFERENCE COUNTERPART -- this is its ground truth).

    python tests/golden/make_dyn_exact.py            # every case
    python tests/golden/make_dyn_exact.py t2 t5      # prints these cases' entries instead of writing the file

The statement, per site i (masking as in occu: a visit counts when y is finite and no covariate of the visit or the site is NaN; NaN
covariates enter the linear predictors as 0):
    psi, gamma, eps = sigma(x_i b_psi), sigma(x_i b_gamma), sigma(x_i b_eps),   u_tj = w_itj alpha
    a1_t = sum_j log sigma(+-u_tj) = -sum_j log1p(exp(-+u_tj))                     log P(y_t | z_t = 1)
    a0_t = sum_j (y_tj ? log tiny_f32 : log1p(-tiny_f32))                          log P(y_t | z_t = 0)   (numpyro's clamp, as in occu)
    P(y_i) = sum over the 2^T paths z of P(z_1) prod P(z_t+1 | z_t) prod_t exp(a_{z_t, t})
computed two ways -- brute force over the paths (T <= 10) and the unnormalised linear-space forward product pi X_0 ... X_T-1 1
(every T; mpmath has no exponent limit, so nothing is rescaled) -- which must agree to 1e-40; Normal priors on every coefficient.
The gradient of every coordinate is a central difference of that statement at h = 1e-20 (truncation ~1e-40, rounding ~1e-30).
Every row must keep the largest site logit <= 16 (dyn_cases.MAX_SITE_LOGIT): beyond it 1 - psi rounds in float64 and the oracle
this fixture certifies can no longer be held to 1e-10."""
import itertools
import json
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dyn_cases  # noqa: E402

mp.mp.dps = 50
H = mp.mpf(10) ** -20
TINY = mp.mpf(float(np.finfo(np.float32).tiny))
BRUTE_MAX_T = 10


def _sigma(v):
    return 1 / (1 + mp.exp(-v))


class Exact:
    def __init__(self, X, W, Y, prior_beta=(0.0, 1.0), prior_alpha=(0.0, 1.0)):
        X, W, Y = np.asarray(X, np.float32), np.asarray(W, np.float32), np.asarray(Y, np.float32)
        Y = Y[0] if Y.ndim == 4 else Y
        self.N, self.Ks = X.shape
        _, self.T, self.J, self.Ko = W.shape
        self.mask = np.isfinite(Y) & ~np.isnan(W).any(-1) & ~np.isnan(X).any(-1)[:, None, None]
        self.X = [[mp.mpf(float(v)) for v in row] for row in np.nan_to_num(X)]
        self.W = [[[[mp.mpf(float(v)) for v in np.nan_to_num(W[i, t, j])] for j in range(self.J)] for t in range(self.T)] for i in range(self.N)]
        self.det = Y != 0
        self.prior_beta = tuple(mp.mpf(float(v)) for v in prior_beta)
        self.prior_alpha = tuple(mp.mpf(float(v)) for v in prior_alpha)
        self._visits_key, self._visits = None, None

    def visits(self, alpha):
        """(L0, L1)[i][t] = exp(a0_t), exp(a1_t); kept for the last alpha (a difference in a site-side coordinate leaves it alone)."""
        key = tuple(alpha)
        if key != self._visits_key:
            out = []
            for i in range(self.N):
                site = []
                for t in range(self.T):
                    a1 = a0 = mp.mpf(0)
                    for j in range(self.J):
                        if not self.mask[i, t, j]:
                            continue
                        u = alpha[0] + mp.fsum(w * a for w, a in zip(self.W[i][t][j], alpha[1:]))
                        if self.det[i, t, j]:
                            a1 -= mp.log1p(mp.exp(-u)); a0 += mp.log(TINY)
                        else:
                            a1 -= mp.log1p(mp.exp(u)); a0 += mp.log1p(-TINY)
                    site.append((mp.exp(a0), mp.exp(a1)))
                out.append(site)
            self._visits_key, self._visits = key, out
        return self._visits

    def site_terms(self, th):
        B = self.Ks + 1
        L = self.visits(th[3 * B:])
        for i in range(self.N):
            psi, gam, eps = (_sigma(th[b * B] + mp.fsum(x * c for x, c in zip(self.X[i], th[b * B + 1:(b + 1) * B]))) for b in range(3))
            yield L[i], psi, gam, eps

    def log_prior(self, th):
        B = self.Ks + 1

        def normal(v, loc, scale):
            return -((v - loc) / scale) ** 2 / 2 - mp.log(scale) - mp.log(2 * mp.pi) / 2

        return mp.fsum(normal(v, *self.prior_beta) for v in th[:3 * B]) + mp.fsum(normal(v, *self.prior_alpha) for v in th[3 * B:])

    def log_joint(self, th):
        """Forward product, linear space, unnormalised."""
        total = self.log_prior(th)
        for L, psi, gam, eps in self.site_terms(th):
            v0, v1 = (1 - psi) * L[0][0], psi * L[0][1]
            for t in range(1, self.T):
                v0, v1 = (v0 * (1 - gam) + v1 * eps) * L[t][0], (v0 * gam + v1 * (1 - eps)) * L[t][1]
            total += mp.log(v0 + v1)
        return total

    def log_joint_brute(self, th):
        """Every one of the 2^T paths, summed."""
        total = self.log_prior(th)
        for L, psi, gam, eps in self.site_terms(th):
            init = (1 - psi, psi)
            step = ((1 - gam, gam), (eps, 1 - eps))
            lik = mp.mpf(0)
            for z in itertools.product((0, 1), repeat=self.T):
                p = init[z[0]] * L[0][z[0]]
                for t in range(1, self.T):
                    p *= step[z[t - 1]][z[t]] * L[t][z[t]]
                lik += p
            total += mp.log(lik)
        return total

    def potential_grad(self, theta32):
        th = [mp.mpf(float(v)) for v in np.asarray(theta32, np.float32)]
        U = -self.log_joint(th)
        if self.T <= BRUTE_MAX_T:
            Ub = -self.log_joint_brute(th)
            assert abs(U - Ub) <= mp.mpf(10) ** -40 * max(1, abs(U)), (U, Ub)
        grad = []
        for k in range(len(th)):
            up, dn = list(th), list(th)
            up[k] += H; dn[k] -= H
            grad.append((self.log_joint(dn) - self.log_joint(up)) / (2 * H))
        return U, grad


def entry(name):
    X, W, Y, theta, kw = dyn_cases.build(name)
    site, visit = dyn_cases.site_logits(X, theta).reshape(len(theta), -1).max(1), dyn_cases.visit_logits(X, W, theta).reshape(len(theta), -1).max(1)
    assert site.max() <= dyn_cases.MAX_SITE_LOGIT, (name, site)
    ex = Exact(X, W, Y, **kw)
    rows = []
    for r, th in enumerate(theta):
        U, grad = ex.potential_grad(th)
        rows.append(dict(U=repr(float(U)), grad=[repr(float(g)) for g in grad],
                         max_site_logit=round(float(site[r]), 3), max_visit_logit=round(float(visit[r]), 3)))
    return dict(shape=[int(v) for v in (X.shape[0], W.shape[1], W.shape[2], X.shape[1], W.shape[3])],
                sha256=dyn_cases.digests(X, W, Y, theta), rows=rows)


def dumps(obj):
    return json.dumps(obj, indent=0, separators=(",", ":"), sort_keys=True) + "\n"


if __name__ == "__main__":
    names = sys.argv[1:]
    if names:
        sys.stdout.write(dumps({n: entry(n) for n in names}))
    else:
        out = dict(dps=mp.mp.dps, h="1e-20", tiny_f32=repr(float(TINY)), max_site_logit=dyn_cases.MAX_SITE_LOGIT, cases={})
        for n in sorted(dyn_cases.SPECS):
            out["cases"][n] = entry(n)
            print(n, "done", flush=True)
        with open(dyn_cases.FIXTURE, "w") as f:
            f.write(dumps(out))
