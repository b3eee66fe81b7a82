"""The generator of the post-fit kernels in NumPy (TEST INFRASTRUCTURE): an exact restatement of csrc/pred_rng.hpp and of the samplers
of csrc/predict_math.hpp, vectorised over cells, independent of the library.

A cell is one (draw n, period t of T, site i of N), n the ABSOLUTE draw index.  Its generator is xoshiro128++ on four 32-bit words:

    index = (n T + t) N + i                      (uint64)
    x     = seed ^ index * 0xD1342543DE82EF95    (uint64, wrapping)
    a, b  = splitmix64(x), splitmix64(x)         (two steps of the one stream)
    s0, s1, s2, s3 = lo(a), hi(a), lo(b), hi(b) | 1
    uniform: r = rotl(s0 + s3, 7) + s0; the xoshiro128 state step; u = (r >> 8) 2^-24, a multiple of 2^-24 in [0, 1)

Everything is integer arithmetic, so ``CellRng.uniform`` equals the device's float32 uniform exactly (returned as float64).  The
samplers take their uniforms from a ``CellRng`` in the kernels' order and do the kernels' float64 arithmetic; cells that take a
data-dependent number of uniforms advance on their own (``uniform(where=...)``), and ``rng.taken`` counts the uniforms per cell.

``UNIFORM_ORDER`` writes out the order in which each kernel consumes a cell's uniforms, taken from its source.
"""
import numpy as np
from scipy.special import gammaln

M64 = (1 << 64) - 1
KEY_MULT = 0xD1342543DE82EF95
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
TWO_PI_F32 = float(np.float32(6.2831853))   # the kernel's float32 constant
U_FLOOR = 2.0 ** -24

# kernel -> the uniforms of one cell, in order.  "xN" = N uniforms; a name in <> is data the count depends on.
UNIFORM_ORDER = {
    # predict.hip: bl_predict_kernel (occu, occu_fp, occu_re, occu_rn: the latent state is z or N, one uniform either way)
    "predict": "latent, then y[j] for j = 0 .. J-1 (one each)",
    # predict.hip: bl_predict_counts_kernel
    "predict_counts/nmixture": "N (one), then per visit j = 0 .. J-1: <N> uniforms (Binomial(N, p_j), whatever p_j is)",
    "predict_counts/occu_cop": "z (one), then per visit j = 0 .. J-1: Poisson(rate_j): none at rate <= 0; rate < 10: count + 1 "
                               "(sequential products); else two per PTRS round",
    # predict.hip: bl_predict_scores_kernel
    "predict_scores": "z, then per visit j = 0 .. J-1: f[j] (one), then the score's normal (two: radius, angle)",
    # comb_predict.hip: the generator advances whether or not an output is wanted
    "predict_comb": "z, then y_pc[j] (one each, Jpc), then y_aru[j] (one each, Jaru), then two per score (Js)",
    # the conditional posteriors
    "site_posterior": "z (one)",
    "abundance_posterior": "n_draw (one: inversion of the conditional pmf)",
    "score_posterior": "z, then f[j] for j = 0 .. J-1 (one each, masked visits included, whatever z is)",
    "count_posterior": "z, then per visit j = 0 .. J-1: <y_j> uniforms in constant mode (Binomial(y_j, rho_j), whatever z is), none "
                       "in the other modes",
    "path_posterior": "one generator per (n, t, i), its first uniform only: t = T-1 decides z_T-1 ~ Bernoulli(z_prob[T-1]); then "
                      "t = T-2 .. 0: z_t ~ Bernoulli(b_1 or b_0 given z_t+1)",
}


def uniform_order(kernel, J=0, Jpc=0, Jaru=0, Js=0):
    """The labels of a cell's uniforms, in order, for the kernels that take a fixed number of them."""
    if kernel == "predict":
        return ["latent"] + [f"y[{j}]" for j in range(J)]
    if kernel == "predict_scores":
        return ["z"] + [lab for j in range(J) for lab in (f"f[{j}]", f"s[{j}].radius", f"s[{j}].angle")]
    if kernel == "predict_comb":
        return (["z"] + [f"y_pc[{j}]" for j in range(Jpc)] + [f"y_aru[{j}]" for j in range(Jaru)]
                + [lab for j in range(Js) for lab in (f"scores[{j}].radius", f"scores[{j}].angle")])
    if kernel in ("site_posterior", "abundance_posterior"):
        return ["z" if kernel == "site_posterior" else "n_draw"]
    if kernel == "score_posterior":
        return ["z"] + [f"f[{j}]" for j in range(J)]
    raise KeyError(f"{kernel}: the number of uniforms depends on the data (UNIFORM_ORDER)")


def _u64(a):
    return np.atleast_1d(np.asarray(a)).astype(np.uint64)


def splitmix64(x):
    """One step on a uint64 array: (new state, output)."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(GOLDEN)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        return x, z ^ (z >> np.uint64(31))


def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


class CellRng:
    """bl_cell_rng(seed, n, T, t, N, i) for arrays n, t, i (broadcast against each other)."""

    def __init__(self, seed, n, T, t, N, i):
        n, t, i = np.broadcast_arrays(_u64(n), _u64(t), _u64(i))
        with np.errstate(over="ignore"):
            index = (n * np.uint64(T) + t) * np.uint64(N) + i
            x = np.uint64(int(seed) & M64) ^ (index * np.uint64(KEY_MULT))
        x, a = splitmix64(x)
        x, b = splitmix64(x)
        lo, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
        self.s = [(a & lo).astype(np.uint32), (a >> sh).astype(np.uint32), (b & lo).astype(np.uint32),
                  (b >> sh).astype(np.uint32) | np.uint32(1)]
        self.shape = index.shape
        self.taken = np.zeros(self.shape, dtype=np.int64)

    def copy(self):
        """An independent generator at the same point of every cell's stream."""
        other = object.__new__(CellRng)
        other.s, other.shape, other.taken = [a.copy() for a in self.s], self.shape, self.taken.copy()
        return other

    def uniform(self, where=None):
        """The next uniform of every cell (float64, exact); with ``where`` only those cells advance (NaN elsewhere)."""
        s0, s1, s2, s3 = self.s
        with np.errstate(over="ignore"):
            r0 = s0 + s3
            r = _rotl(r0, 7) + s0
        t = s1 << np.uint32(9)
        s2 = s2 ^ s0
        s3 = s3 ^ s1
        s1 = s1 ^ s2
        s0 = s0 ^ s3
        s2 = s2 ^ t
        s3 = _rotl(s3, 11)
        u = (r >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        new = [s0, s1, s2, s3]
        if where is None:
            self.s = new
            self.taken += 1
            return u
        where = np.broadcast_to(where, self.shape)
        self.s = [np.where(where, a, b) for a, b in zip(new, self.s)]
        self.taken += where
        return np.where(where, u, np.nan)


def bernoulli(rng, p):
    """[u < p], one uniform (pm_draw_z and every visit's detection)."""
    return rng.uniform() < p


def binomial(rng, n, p):
    """bl_binomial: n Bernoulli(p) trials, one uniform each: a cell takes n uniforms whatever p is."""
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), rng.shape)
    cnt = np.zeros(rng.shape, dtype=np.int64)
    for m in range(int(n.max(initial=0))):
        on = m < n
        u = rng.uniform(where=on)
        cnt += on & (u < p)
    return cnt


def poisson(rng, lam):
    """bl_poisson in float64: (the draw, the uniforms it took), per cell.  lam <= 0 (or NaN): 0 without a uniform; lam < 10:
    sequential products against exp(-lam), at most 1000 factors; else Hoermann's PTRS, at most 1000 rounds of two uniforms, then
    (int)lam."""
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), rng.shape)
    start = rng.taken.copy()
    out = np.zeros(rng.shape, dtype=np.int64)
    small, big = (lam > 0.0) & (lam < 10.0), lam >= 10.0
    if small.any():
        enlam = np.exp(-np.where(small, lam, 1.0))
        prod = np.where(small, rng.uniform(where=small), 0.0)
        k = np.zeros(rng.shape, dtype=np.int64)
        on = small & (prod > enlam)
        while on.any():
            prod = np.where(on, prod * rng.uniform(where=on), prod)
            k += on
            on = on & (prod > enlam) & (k < 1000)
        out = np.where(small, k, out)
    if big.any():
        L = np.where(big, lam, 10.0)
        slam, loglam = np.sqrt(L), np.log(L)
        b = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * b
        invalpha, vr = 1.1239 + 1.1328 / (b - 3.4), 0.9277 - 3.6224 / (b - 2.0)
        on = big.copy()
        res = np.where(big, L.astype(np.int64), 0)              # what 1000 rejected rounds leave
        for _ in range(1000):
            if not on.any():
                break
            U, V = rng.uniform(where=on) - 0.5, rng.uniform(where=on)
            with np.errstate(invalid="ignore", divide="ignore"):
                us = 0.5 - np.abs(U)
                kf = np.floor((2.0 * a / us + b) * U + L + 0.43)
                fast = (us >= 0.07) & (V <= vr)
                skip = ~fast & ((kf < 0.0) | ((us < 0.013) & (V > us)))
                slow = ~fast & ~skip & (np.log(V) + np.log(invalpha) - np.log(a / (us * us) + b) <= -L + kf * loglam - gammaln(kf + 1.0))
            acc = on & (fast | slow)
            res = np.where(acc, np.nan_to_num(kf).astype(np.int64), res)
            on = on & ~acc
        out = np.where(big, res, out)
    return out, rng.taken - start


def truncated_poisson(rng, eta, K):
    """pm_draw_abundance: N ~ Poisson(exp(eta)) restricted to 0 .. K by inversion over the renormalised pmf, the float64 recursion
    p_m+1 = p_m lambda / (m + 1); one uniform.  exp(-lambda) = 0 (lambda > 745) leaves no mass anywhere: the draw is K."""
    eta = np.broadcast_to(np.asarray(eta, dtype=np.float64), rng.shape)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        lam = np.exp(eta)
        p, tot = np.exp(-lam), np.zeros(rng.shape)
        for m in range(K + 1):
            tot = tot + p
            p = p * (lam / (m + 1.0))
        target = rng.uniform() * tot
        p, cum = np.exp(-lam), np.zeros(rng.shape)
        out = np.full(rng.shape, K, dtype=np.int64)
        found = np.zeros(rng.shape, dtype=bool)
        for m in range(K + 1):
            cum = cum + p
            hit = ~found & (target < cum)
            out = np.where(hit, m, out)
            found |= hit
            p = p * (lam / (m + 1.0))
    return out


def normal(rng):
    """pm_normal in float64: Box-Muller, two uniforms, the first floored at 2^-24; the angle is u2 times the kernel's float32 2 pi."""
    u1, u2 = np.maximum(rng.uniform(), U_FLOOR), rng.uniform()
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI_F32 * u2)


def cells(seed, draws, T, N, sites=None):
    """A ``CellRng`` over the grid (len(draws), T, len(sites)): absolute draw indices ``draws``, every period, ``sites`` (default all)."""
    sites = np.arange(N) if sites is None else np.asarray(sites)
    n, t, i = np.meshgrid(np.asarray(draws), np.arange(T), sites, indexing="ij")
    return CellRng(seed, n, T, t, N, i)
