"""Python handle over the HIP engine's C-ABI: dataset upload, log-density hook, NUTS driver.

This is the host-side counterpart of what ``mcmc.run`` did in the reference
(biolith/utils/fit.py:105-130).  It only marshals NumPy buffers through ``ctypes``; all arithmetic
of the hot path runs in the gfx950 kernels under ``csrc/``.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _ffi


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


class _PinnedPool:
    """Page-locked host buffers for the large deterministic sites (psi at the headline size: 160 MB).  Copying into page-locked
    memory runs at PCIe rate (3 ms instead of 10 for those 160 MB), but pinning it is slow (60 ms), so: the FIRST request of a size
    class gets ordinary pages at once while a buffer of that class is pinned in the background; later requests take a pooled
    buffer, which returns to the pool when the array that used it is gone.  At most ``cap`` bytes stay pooled."""

    def __init__(self, cap=1 << 30):
        import threading

        self.free, self.cap, self.held, self.pending, self.wanted, self.lock = {}, cap, 0, set(), set(), threading.Lock()

    def empty(self, lib, shape, dtype):
        import weakref

        count = int(np.prod(shape))
        size = 1 << max(23, (count * np.dtype(dtype).itemsize - 1).bit_length())   # power-of-two size classes
        with self.lock:
            bucket = self.free.get(size)
            ptr = bucket.pop() if bucket else None
            if ptr is not None:
                self.held -= size
            elif size not in self.pending and size not in self.wanted and self.held + size <= self.cap:
                self.wanted.add(size)   # (pinned once the copy that is about to run is over: kick())
        if ptr is None:
            return np.empty(shape, dtype=dtype)
        buf = (C.c_char * size).from_address(ptr)
        arr = np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)
        weakref.finalize(buf, self._give_back, lib, size, ptr)       # (the array keeps ``buf`` alive through its base chain)
        return arr

    def kick(self, lib):
        """Start pinning the size classes asked for since the last call (after the device copy: the two would contend)."""
        import threading

        with self.lock:
            todo, self.wanted = self.wanted, set()
            self.pending |= todo
        for size in todo:
            threading.Thread(target=self._warm, args=(lib, size)).start()   # (not a daemon: never killed inside a driver call at exit)

    def _warm(self, lib, size):
        p = C.c_void_p()
        ok = lib.bl_host_alloc(size, C.byref(p)) == 0
        with self.lock:
            self.pending.discard(size)
        if ok:
            self._give_back(lib, size, p.value)

    def _give_back(self, lib, size, ptr):
        with self.lock:
            keep = self.held + size <= self.cap
            if keep:
                self.free.setdefault(size, []).append(ptr)
                self.held += size
        if not keep:
            lib.bl_host_free(C.c_void_p(ptr))


_PINNED = _PinnedPool()
_CTYPE = {np.float32: C.c_float, np.uint8: C.c_uint8, np.int32: C.c_int32, np.float64: C.c_double}   # the per-draw entries' output types


@dataclass
class NutsResult:
    draws: np.ndarray             # (C, S, D) float32
    diverging: np.ndarray         # (C, S) bool
    num_steps: np.ndarray         # (C, S) int32
    accept_prob: np.ndarray       # (C, S) float32
    potential_energy: np.ndarray  # (C, S) float32
    step_size: np.ndarray         # (C,)
    inv_mass: np.ndarray          # (C, D)
    n_leapfrog: np.ndarray        # (C, 2) int64: warmup, sampling gradient evaluations
    kernel_ms: float              # HIP-event time of the persistent kernel
    wgs_per_chain: int
    lds_bytes: int
    lds_staged: bool
    chains_l2_local: int = 0      # chains that ran the verified same-XCD (L2-local) exchange
    threads_per_wg: int = 0       # 64 x (compute waves + 1 control wave)
    lds_vector_tier: int = 0      # random-effects / occu_cs kernels: sampler vectors kept in LDS (0 none, 1 the leaf in flight, 2 all a leapfrog touches)
    comm_init_ms: float = 0.0     # fit(devices=[...]): wall time of ncclCommInitAll (outside the sampling clock)
    lane_group: tuple = (1, 1)    # lanes that shared one site pair: (period lanes, visit lanes); (1, 1) = one pair per lane
    kernel_name: str = ""         # the sampler instantiation that ran, as rocprofv3 names it
    env_overrides: str = ""       # BIOLITH_HIP_* knobs set at the launch ("" = none: the engine's own geometry and kernel form)
    record_bytes: int = 0         # bytes of a workgroup's exchange record: 64 = compact records, 128 / 256 / 512 = 16 / 32 / 64 granules


class OccuDataset:
    """Device-resident occupancy dataset (one species).

    Parameters mirror ``occu``'s data arguments (biolith/models/occu.py:19-40):
    ``site_covs (N, Ks)``, ``obs_covs (N, T, J, Ko)``, ``obs (S=1, N, T, J)``; NaN = missing.
    """

    def __init__(self, site_covs, obs_covs, obs, prior_beta=(0.0, 1.0), prior_alpha=(0.0, 1.0), device: int = 0,
                 model: str = "occu", max_abundance: int = 100, fp_mode: Optional[str] = "constant", prior_fp=(2.0, 5.0),
                 session_duration=None, prior_fp_rate: float = 1.0, site_random_effects: bool = False,
                 obs_random_effects: bool = False, prior_site_re_sd: float = 1.0, prior_obs_re_sd: float = 1.0,
                 prior_mu=((0.0, 10.0), (0.0, 10.0)), prior_sigma=((5.0, 1.0), (5.0, 1.0)), re_fp_mode: Optional[str] = None,
                 ARU_obs_covs=None, ARU_obs=None, scores_obs=None, prior_fc=(2.0, 5.0), prior_fu=(2.0, 5.0)):
        lib = _ffi.load()
        if model not in ("occu", "occu_rn", "occu_fp", "occu_cop", "nmixture", "occu_re", "occu_cs", "occu_dyn", "occu_comb"):
            raise ValueError(f"unknown model {model!r}")
        if fp_mode not in ("constant", "unoccupied") and not (model == "occu_cop" and fp_mode is None):
            raise ValueError(f"unknown fp_mode {fp_mode!r}")
        self.model, self.max_abundance = model, int(max_abundance)
        self.fp_mode, self.prior_fp = fp_mode, (float(prior_fp[0]), float(prior_fp[1]))
        X = np.ascontiguousarray(site_covs, dtype=np.float32)
        W = np.ascontiguousarray(obs_covs, dtype=np.float32)
        Y = np.ascontiguousarray(obs, dtype=np.float32)
        if X.ndim != 2:
            raise ValueError("site_covs must be of shape (n_sites, n_site_covs)")
        if W.ndim != 4:
            raise ValueError("obs_covs must be of shape (n_sites, n_periods, n_replicates, n_obs_covs)")
        if Y.ndim != 4:
            raise ValueError("obs must be of shape (n_species, n_sites, n_periods, n_replicates)")
        N, Ks = X.shape
        _, T, J, Ko = W.shape
        if W.shape[0] != N:
            raise ValueError("site_covs and obs_covs must have the same number of sites")
        if Y.shape[1:] != (N, T, J):
            raise ValueError("obs must have shape (n_species, n_sites, n_periods, n_replicates) matching obs_covs")
        self.dims = _ffi.bl_dims(Y.shape[0], N, T, J, Ks, Ko)
        self.N, self.T, self.J, self.Ks, self.Ko, self.S = N, T, J, Ks, Ko, Y.shape[0]
        # occu_fp: trailing phi = logit(false-positive rate); occu_cop with a false-positive rate: phi = log(rate)
        self.D = Ks + Ko + 2 + (1 if model == "occu_fp" or (model == "occu_cop" and fp_mode is not None) else 0)
        if self.S > 1:
            # several species in one handle: ONE chain over theta = [species 0: beta, alpha | species 1: ... | (shared phi)]
            # (the species plate of occu.py:182-186 under one NUTS); occu with or without false positives, or with random
            # effects: theta = [... | log sds | site_re_occ [S][N] | site_re_det [S][N] | obs_re [S][N][T][J]], the sds shared
            if model not in ("occu", "occu_fp", "occu_re"):
                raise NotImplementedError(f"{model}: one species per dataset (joint sampling is built for occu / occu_fp / occu_re)")
            self.D += (self.S - 1) * (Ks + Ko + 2)
        self.device = device
        pb = _ffi.bl_normal_prior(float(prior_beta[0]), float(prior_beta[1]))
        pa = _ffi.bl_normal_prior(float(prior_alpha[0]), float(prior_alpha[1]))
        h = C.c_void_p()
        if model == "occu_comb":
            # obs_covs / obs are the point counts' (one species); theta = [beta | alpha_PC | alpha_ARU | logit fc | logit fu | mu0 |
            # log(mu1 - mu0) | log sigma0 | log sigma1] (include/biolith_hip.h: bl_dataset_create_comb)
            if self.S != 1:
                raise NotImplementedError("occu_comb: one species per dataset")
            Wa = np.ascontiguousarray(ARU_obs_covs, dtype=np.float32)
            Ya = np.ascontiguousarray(ARU_obs, dtype=np.float32)
            Sc = np.ascontiguousarray(scores_obs, dtype=np.float32)
            if Wa.ndim != 4 or Wa.shape[:2] != (N, T):
                raise ValueError("ARU_obs_covs must be of shape (n_sites, n_periods, ARU_replicates, n_ARU_obs_covs)")
            if Ya.shape != (1, N, T, Wa.shape[2]):
                raise ValueError("ARU_obs must have shape (1, n_sites, n_periods, ARU_replicates)")
            if Sc.ndim != 4 or Sc.shape[:3] != (1, N, T):
                raise ValueError("scores_obs must have shape (1, n_sites, n_periods, scores_replicates)")
            self.dims_comb = _ffi.bl_comb_dims(N, T, J, Wa.shape[2], Sc.shape[3], Ks, Ko, Wa.shape[3])
            self.Ka, self.Ja, self.Js = Wa.shape[3], Wa.shape[2], Sc.shape[3]
            pfc, pfu = _ffi.bl_beta_prior(*map(float, prior_fc)), _ffi.bl_beta_prior(*map(float, prior_fu))
            pm = np.ascontiguousarray(np.asarray(prior_mu, dtype=np.float64).reshape(4))
            ps = np.ascontiguousarray(np.asarray(prior_sigma, dtype=np.float64).reshape(4))
            _ffi.check(lib.bl_dataset_create_comb(C.byref(self.dims_comb), _fp(X), _fp(W), _fp(Y), _fp(Wa), _fp(Ya), _fp(Sc),
                                                  C.byref(pfc), C.byref(pfu), _dp(pm), _dp(ps), C.byref(pb), C.byref(pa), device, C.byref(h)))
            self.D = Ks + Ko + Wa.shape[3] + 9
        elif model == "occu_dyn":
            # builder-defined dynamic occupancy (no reference counterpart): theta = [b_psi | b_gamma | b_eps (Ks+1 each) | alpha (Ko+1)]
            if self.S != 1:
                raise NotImplementedError("occu_dyn: one species per dataset")
            _ffi.check(lib.bl_dataset_create_dyn(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), C.byref(pb), C.byref(pa), device, C.byref(h)))
            self.D = 3 * (Ks + 1) + Ko + 1
        elif model == "occu_rn" and re_fp_mode is not None:
            # Royle-Nichols with a false-positive rate (with or without random effects): theta = [beta, alpha, phi = logit(rate), (log sds), (effects)]
            if re_fp_mode != "constant":
                raise ValueError("occu_rn: the false-positive rate acts on every site (re_fp_mode='constant')")
            pf = _ffi.bl_beta_prior(*self.prior_fp)
            _ffi.check(lib.bl_dataset_create_rn_fp(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), int(max_abundance),
                                                   int(bool(site_random_effects)), int(bool(obs_random_effects)),
                                                   float(prior_site_re_sd), float(prior_obs_re_sd), C.byref(pf), C.byref(pb), C.byref(pa),
                                                   device, C.byref(h)))
            d = C.c_int()
            _ffi.check(lib.bl_dataset_param_dim(h, C.byref(d)))
            self.D = int(d.value)
        elif model == "occu_rn" and (site_random_effects or obs_random_effects):
            # theta = [beta, alpha, (log site_re_sd), (log obs_re_sd), (site_re_abu[N], site_re_det[N]), (obs_re[N][T][J])]
            _ffi.check(lib.bl_dataset_create_rn_re(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), int(max_abundance),
                                                   int(bool(site_random_effects)), int(bool(obs_random_effects)),
                                                   float(prior_site_re_sd), float(prior_obs_re_sd), C.byref(pb), C.byref(pa),
                                                   device, C.byref(h)))
            d = C.c_int()
            _ffi.check(lib.bl_dataset_param_dim(h, C.byref(d)))
            self.D = int(d.value)
        elif model == "occu_rn":
            _ffi.check(lib.bl_dataset_create_rn(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), int(max_abundance),
                                                C.byref(pb), C.byref(pa), device, C.byref(h)))
        elif model == "nmixture":
            with np.errstate(invalid="ignore"):
                if np.isfinite(Y).any() and np.nanmax(Y) > max_abundance:
                    raise ValueError(f"max_abundance={max_abundance} is below the largest count {np.nanmax(Y):g}")
            if site_random_effects or obs_random_effects:
                # theta = [beta, alpha, (log site_re_sd), (log obs_re_sd), (site_re_abu[N], site_re_det[N]), (obs_re[N][T][J])]
                _ffi.check(lib.bl_dataset_create_nmix_re(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), int(max_abundance),
                                                         int(bool(site_random_effects)), int(bool(obs_random_effects)),
                                                         float(prior_site_re_sd), float(prior_obs_re_sd), C.byref(pb), C.byref(pa),
                                                         device, C.byref(h)))
                d = C.c_int()
                _ffi.check(lib.bl_dataset_param_dim(h, C.byref(d)))
                self.D = int(d.value)
            else:
                _ffi.check(lib.bl_dataset_create_nmix(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), int(max_abundance),
                                                      C.byref(pb), C.byref(pa), device, C.byref(h)))
        elif model == "occu_cop":
            if session_duration is None:
                raise ValueError("occu_cop needs session_duration (n_sites, n_periods, n_replicates)")
            Dur = np.ascontiguousarray(session_duration, dtype=np.float32)
            if Dur.shape != (N, T, J):
                raise ValueError("session_duration must have shape (n_sites, n_periods, n_replicates)")
            mode = {None: 0, "constant": _ffi.FP_CONSTANT, "unoccupied": _ffi.FP_UNOCCUPIED}[fp_mode]
            if site_random_effects or obs_random_effects:
                # theta = [beta, alpha, (log site_re_sd), (log obs_re_sd), (site_re_occ[N], site_re_det[N]), (obs_re[N][T][J])]
                # (+ phi = log rate_fp right behind the coefficients with a false-positive rate)
                _ffi.check(lib.bl_dataset_create_cop_re(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), _fp(Dur), mode, float(prior_fp_rate),
                                                        int(bool(site_random_effects)), int(bool(obs_random_effects)),
                                                        float(prior_site_re_sd), float(prior_obs_re_sd), C.byref(pb), C.byref(pa), device, C.byref(h)))
                d = C.c_int()
                _ffi.check(lib.bl_dataset_param_dim(h, C.byref(d)))
                self.D = int(d.value)
            else:
                _ffi.check(lib.bl_dataset_create_cop(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), _fp(Dur), mode,
                                                     float(prior_fp_rate), C.byref(pb), C.byref(pa), device, C.byref(h)))
        elif model == "occu_cs":
            # obs holds the scores; theta = [beta, alpha, mu0, log(mu1 - mu0), log sigma0, log sigma1]
            pm = np.ascontiguousarray(np.asarray(prior_mu, dtype=np.float64).reshape(4))
            ps = np.ascontiguousarray(np.asarray(prior_sigma, dtype=np.float64).reshape(4))
            _ffi.check(lib.bl_dataset_create_cs(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), _dp(pm), _dp(ps),
                                                C.byref(pb), C.byref(pa), device, C.byref(h)))
            self.D = Ks + Ko + 6
        elif model == "occu_re":
            # theta = [beta, alpha, (log site_re_sd), (log obs_re_sd), (site_re_occ[N], site_re_det[N]), (obs_re[N][T][J])]
            if not (site_random_effects or obs_random_effects):
                raise ValueError("occu_re needs site_random_effects and / or obs_random_effects")
            if re_fp_mode is not None:
                # ... together with a false-positive rate (occu.py:146-157): theta = [beta, alpha, phi = logit(rate), log sds, effects]
                if re_fp_mode not in ("constant", "unoccupied"):
                    raise ValueError(f"unknown re_fp_mode {re_fp_mode!r}")
                pf = _ffi.bl_beta_prior(*self.prior_fp)
                _ffi.check(lib.bl_dataset_create_re_fp(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), int(bool(site_random_effects)),
                                                       int(bool(obs_random_effects)), float(prior_site_re_sd), float(prior_obs_re_sd),
                                                       _ffi.FP_CONSTANT if re_fp_mode == "constant" else _ffi.FP_UNOCCUPIED, C.byref(pf),
                                                       C.byref(pb), C.byref(pa), device, C.byref(h)))
            else:
                _ffi.check(lib.bl_dataset_create_re(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), int(bool(site_random_effects)),
                                                    int(bool(obs_random_effects)), float(prior_site_re_sd), float(prior_obs_re_sd),
                                                    C.byref(pb), C.byref(pa), device, C.byref(h)))
            d = C.c_int()
            _ffi.check(lib.bl_dataset_param_dim(h, C.byref(d)))
            self.D = int(d.value)
        elif model == "occu_fp":
            pf = _ffi.bl_beta_prior(*self.prior_fp)
            mode = _ffi.FP_CONSTANT if fp_mode == "constant" else _ffi.FP_UNOCCUPIED
            _ffi.check(lib.bl_dataset_create_fp(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), mode, C.byref(pf),
                                                C.byref(pb), C.byref(pa), device, C.byref(h)))
        else:
            _ffi.check(lib.bl_dataset_create(C.byref(self.dims), _fp(X), _fp(W), _fp(Y), C.byref(pb), C.byref(pa),
                                             device, C.byref(h)))
        self._h = h
        self._lib = lib
        # Laplace instead of Normal coefficient priors (distributions.LocScale.family; utils/grid_search.py:366-371)
        fam = [getattr(p, "family", "normal") for p in (prior_beta, prior_alpha)]
        if any(f not in ("normal", "laplace") for f in fam):
            raise ValueError(f"unknown prior family {fam}")
        if "laplace" in fam:
            _ffi.check(lib.bl_dataset_set_prior_family(h, int(fam[0] == "laplace"), int(fam[1] == "laplace")))
        self.site_re, self.obs_re = bool(site_random_effects), bool(obs_random_effects)
        self.re_fp_mode = re_fp_mode if model in ("occu_re", "occu_rn") else None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bl_dataset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ K1 parity hook ----
    def logp_grad(self, theta, staged: bool = True):
        """U(theta) = -log p(theta, y) and dU/dtheta; theta (D,) or (B, D)."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        single = th.ndim == 1
        th2 = th.reshape(1, -1) if single else th
        if th2.shape[1] != self.D:
            raise ValueError(f"theta must have {self.D} columns")
        B = th2.shape[0]
        U = np.empty(B)
        G = np.empty((B, self.D))
        _ffi.check(self._lib.bl_logp_grad(self._h, B, _dp(th2), _dp(U), _dp(G), int(staged)))
        return (U[0], G[0]) if single else (U, G)

    # --------------------------------------------------------------------------- NUTS ----
    def _config(self, num_warmup, num_samples, num_chains, seed, chain_offset, max_tree_depth, target_accept,
                wgs_per_chain, init_theta):
        cfg = _ffi.bl_nuts_config()
        cfg.num_warmup, cfg.num_samples, cfg.num_chains = int(num_warmup), int(num_samples), int(num_chains)
        cfg.chain_offset, cfg.seed = int(chain_offset), int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.max_tree_depth, cfg.wgs_per_chain = int(max_tree_depth), int(wgs_per_chain)
        cfg.target_accept = float(target_accept)
        keep = None
        if init_theta is not None:
            keep = np.ascontiguousarray(init_theta, dtype=np.float64)
            if keep.shape != (num_chains, self.D):
                raise ValueError("init_theta must have shape (num_chains, D)")
            cfg.init_theta = _dp(keep)
        return cfg, keep

    def launch(self, num_warmup=1000, num_samples=1000, num_chains=1, seed=0, chain_offset=0, max_tree_depth=10,
               target_accept=0.8, wgs_per_chain=0, init_theta=None, stream: Optional[int] = None):
        """Asynchronous launch of the persistent kernel (returns immediately)."""
        cfg, keep = self._config(num_warmup, num_samples, num_chains, seed, chain_offset, max_tree_depth,
                                 target_accept, wgs_per_chain, init_theta)
        _ffi.check(self._lib.bl_nuts_launch(self._h, C.byref(cfg), C.c_void_p(stream or 0)))
        self._shape = (int(num_chains), int(num_samples))

    def done(self) -> bool:
        d = C.c_int(0)
        _ffi.check(self._lib.bl_nuts_poll(self._h, C.byref(d)))
        return bool(d.value)

    def abort(self):
        self._lib.bl_nuts_abort(self._h)

    def wait(self):
        _ffi.check(self._lib.bl_nuts_wait(self._h))

    def wgs_per_chain(self) -> int:
        """Workgroups per chain of the last launch (bl_nuts_geometry)."""
        k, thr, lds, staged, loc = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _ffi.check(self._lib.bl_nuts_geometry(self._h, C.byref(k), C.byref(thr), C.byref(lds), C.byref(staged), C.byref(loc)))
        return int(k.value)

    def _kernel_name(self) -> str:
        buf = C.create_string_buffer(192)
        _ffi.check(self._lib.bl_nuts_kernel_name(self._h, buf, 192))
        return buf.value.decode()

    def env_overrides(self) -> str:
        """BIOLITH_HIP_* knobs that were set when the last launch read the environment ("" = none; bl_nuts_env_overrides)."""
        if not hasattr(self._lib, "bl_nuts_env_overrides"):   # (a library built before round 6, loaded by name for an A/B)
            return ""
        buf = C.create_string_buffer(512)
        _ffi.check(self._lib.bl_nuts_env_overrides(self._h, buf, 512))
        return buf.value.decode()

    def record_bytes(self) -> int:
        """Bytes of one workgroup's exchange record in the last finished launch (bl_nuts_record_bytes; 0: the library has no such call)."""
        if not hasattr(self._lib, "bl_nuts_record_bytes"):   # (a library built before the compact records, loaded by name for an A/B)
            return 0
        n = C.c_int(0)
        _ffi.check(self._lib.bl_nuts_record_bytes(self._h, C.byref(n)))
        return int(n.value)

    def elapsed_ms(self) -> float:
        ms = C.c_float(0)
        _ffi.check(self._lib.bl_nuts_elapsed_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def debug_counters(self, n: int = 32):
        """In-kernel phase cycle counters (zeros unless a BL_STAMPS diagnostic library is loaded)."""
        out = np.zeros(n, dtype=np.int64)
        _ffi.check(self._lib.bl_nuts_debug_counters(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), n))
        return out

    def device_draws(self):
        """(device pointer, bytes) of the last launch's draws [C][S][D] float32."""
        p, n = C.c_void_p(), C.c_size_t()
        _ffi.check(self._lib.bl_nuts_device_draws(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def _output(self, Cn: int, S: int):
        """Host arrays for ``Cn`` chains x ``S`` draws and the ``bl_nuts_output`` that points at them."""
        D = self.D
        a = dict(draws=np.empty((Cn, S, D), dtype=np.float32), diverging=np.empty((Cn, S), dtype=np.uint8),
                 num_steps=np.empty((Cn, S), dtype=np.int32), accept_prob=np.empty((Cn, S), dtype=np.float32),
                 potential_energy=np.empty((Cn, S), dtype=np.float32), step_size=np.empty(Cn, dtype=np.float32),
                 inv_mass=np.empty((Cn, D), dtype=np.float32), n_leapfrog=np.empty((Cn, 2), dtype=np.int64))
        out = _ffi.bl_nuts_output(
            _fp(a["draws"]), a["diverging"].ctypes.data_as(C.POINTER(C.c_uint8)), a["num_steps"].ctypes.data_as(C.POINTER(C.c_int32)),
            _fp(a["accept_prob"]), _fp(a["potential_energy"]), _fp(a["step_size"]), _fp(a["inv_mass"]),
            a["n_leapfrog"].ctypes.data_as(C.POINTER(C.c_int64)),
        )
        return a, out

    def _result(self, a) -> NutsResult:
        k, thr, lds, staged, loc = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _ffi.check(self._lib.bl_nuts_geometry(self._h, C.byref(k), C.byref(thr), C.byref(lds), C.byref(staged), C.byref(loc)))
        gt, gj = C.c_int(1), C.c_int(1)
        _ffi.check(self._lib.bl_nuts_lane_group(self._h, C.byref(gt), C.byref(gj)))
        return NutsResult(a["draws"], a["diverging"].astype(bool), a["num_steps"], a["accept_prob"], a["potential_energy"],
                          a["step_size"], a["inv_mass"], a["n_leapfrog"], self.elapsed_ms(),
                          k.value, lds.value, bool(staged.value & 1), loc.value, thr.value, staged.value >> 1,
                          lane_group=(int(gt.value), int(gj.value)), kernel_name=self._kernel_name(), env_overrides=self.env_overrides(),
                          record_bytes=self.record_bytes())

    def fetch(self) -> NutsResult:
        Cn, S = self._shape
        a, out = self._output(Cn, S)
        _ffi.check(self._lib.bl_nuts_fetch(self._h, C.byref(out)))
        return self._result(a)

    def nuts(self, timeout: Optional[float] = None, **kw) -> NutsResult:
        """launch + wait + fetch.  With ``timeout`` (seconds) the kernel is aborted through its
        host-mapped flag and ``TimeoutError`` raised (fit(timeout=...), biolith/utils/fit.py:124-128)."""
        self.launch(**kw)
        if timeout is not None:
            t_end = time.monotonic() + float(timeout)
            try:
                while not self.done():
                    if time.monotonic() > t_end:
                        raise TimeoutError("Timed out")
                    time.sleep(0.0005)
            except BaseException:
                # also reached for the reference-style SIGALRM TimeoutException or Ctrl-C
                self.abort()
                try:
                    self.wait()
                except Exception:
                    pass
                raise
        self.wait()
        return self.fetch()

    # ------------------------------------------------------------ deterministic sites ----
    def _draw_matrix(self, draws):
        """draws (..., D) -> contiguous float32 (n, D); a different trailing size (e.g. a random-effects posterior of
        another number of sites) is rejected instead of being silently re-shaped."""
        d = np.asarray(draws, dtype=np.float32)
        if d.ndim == 0 or d.shape[-1] != self.D:
            raise ValueError(f"draws must have {self.D} coordinates on the last axis for this dataset, got shape {d.shape}")
        return np.ascontiguousarray(d).reshape(-1, self.D)

    def _big_empty(self, shape, dtype=np.float32):
        """Output array for a device -> host copy: page-locked (pooled, see ``_PinnedPool``) from 8 MB on."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if nbytes < (8 << 20):
            return np.empty(shape, dtype=dtype)
        return _PINNED.empty(self._lib, shape, dtype)

    def deterministic(self, draws, psi: bool = True, prob_detection: bool = False):
        """psi -- or, for occu_rn, abundance -- (n, T, N) and/or prob_detection (n, J, T, N) for draws (n, D)
        (occu.py:207,221-228; occu_rn.py:192,209-218)."""
        d = self._draw_matrix(draws)
        n = d.shape[0]
        out_psi = self._big_empty((n, self.T, self.N)) if psi else None
        out_pd = self._big_empty((n, self.J, self.T, self.N)) if prob_detection else None
        _ffi.check(self._lib.bl_deterministic(self._h, n, _fp(d), _fp(out_psi), _fp(out_pd)))
        _PINNED.kick(self._lib)
        return out_psi, out_pd

    def site_summary(self, draws, ranks=(), psi: bool = True, prob_detection: bool = True):
        """The deterministic sites' summary over draws (n, D), fused on the device (BUILDER-DEFINED): ``psi_mean, psi_sd, psi_order,
        prob_mean, prob_sd, prob_order``.  The first site (``psi``; occu_rn, nmixture: ``abundance``) is constant over the periods and
        comes back per site: mean and sd (N,) float64, order (len(ranks), N) float32; the second (``prob_detection``; occu_cop:
        ``rate_detection``): (J, T, N) and (len(ranks), J, T, N).  ``order[r]`` is the value of rank ``ranks[r]`` (0 = smallest) among
        the cell's n float32 values of ``deterministic``, bit for bit; mean and sd (ddof 1, NaN for one draw) are float64 sums over them
        in draw order.  ``None`` for a site that is not wanted, and for the order statistics without ranks.  Nothing of size (n, T, N)
        or (n, J, T, N) exists on the device or the host.  Draws must be finite (include/biolith_hip.h: bl_site_summary)."""
        d = self._draw_matrix(draws)
        n = d.shape[0]
        r = np.ascontiguousarray(np.asarray(ranks, dtype=np.int64).reshape(-1))
        if not (psi or prob_detection):
            raise ValueError("site_summary(): neither site is wanted")
        if n == 0:
            raise ValueError("site_summary(): no draws")
        if r.size > _ffi.SUMMARY_MAX_RANKS:
            raise NotImplementedError(f"site_summary(): {r.size} ranks, at most {_ffi.SUMMARY_MAX_RANKS} (BL_SUMMARY_MAX_RANKS)")
        if r.size and (r.min() < 0 or r.max() >= n):
            raise ValueError(f"site_summary(): ranks must lie in 0 .. n_draws - 1 = {n - 1}")
        r32 = r.astype(np.int32)
        out = []
        for want, shape in ((psi, (self.N,)), (prob_detection, (self.J, self.T, self.N))):
            out += [np.empty(shape) if want else None, np.empty(shape) if want else None,
                    np.empty((r.size,) + shape, dtype=np.float32) if want and r.size else None]
        ptrs = [None if a is None else a.ctypes.data_as(C.POINTER(_CTYPE[a.dtype.type])) for a in out]
        _ffi.check(self._lib.bl_site_summary(self._h, n, _fp(d), int(r.size), r32.ctypes.data_as(C.POINTER(C.c_int32)), *ptrs))
        return tuple(out)

    def site_diagnostics(self, draws, n_chains: int, psi: bool = True, prob_detection: bool = True):
        """The deterministic sites' convergence diagnostics over draws (C n, D) of ``n_chains`` = C chains, chain-major, fused on the
        device (BUILDER-DEFINED): ``psi_n_eff, psi_r_hat, psi_mean, psi_sd, prob_n_eff, prob_r_hat, prob_mean, prob_sd``, float64.  The
        first site (``psi``; occu_rn, nmixture: ``abundance``) is constant over the periods and comes back per site, (N,); the second
        (``prob_detection``; occu_cop: ``rate_detection``) (J, T, N).  ``n_eff`` and ``r_hat`` are numpyro's effective sample size and
        split R-hat of the cell's float32 values of ``deterministic``, by direct lagged sums in float64 (include/biolith_hip.h:
        bl_site_diagnostics); ``mean`` and ``sd`` are ``site_summary``'s.  ``None`` for a site that is not wanted.  Nothing of size
        (C n, T, N) or (C n, J, T, N) exists on the device or the host.  Draws must be finite."""
        d = self._draw_matrix(draws)
        total, C_ = d.shape[0], int(n_chains)
        if not (psi or prob_detection):
            raise ValueError("site_diagnostics(): neither site is wanted")
        if C_ < 1 or total == 0 or total % C_:
            raise ValueError(f"site_diagnostics(): {total} draws are not {C_} chains of equal length")
        if total // C_ < 2:
            raise ValueError(f"site_diagnostics(): {total // C_} draws per chain, at least 2")
        out = []
        for want, shape in ((psi, (self.N,)), (prob_detection, (self.J, self.T, self.N))):
            out += [np.empty(shape) if want else None for _ in range(4)]
        _ffi.check(self._lib.bl_site_diagnostics(self._h, total, _fp(d), C_, *[_dp(a) for a in out]))
        return tuple(out)

    def regional_totals(self, draws, region, n_regions: int, weight=None, seed: int = 0, site: bool = True, latent: bool = True):
        """Per draw of draws (n, D) and region, the weighted totals of the first deterministic site and of the latent state, fused on
        the device (BUILDER-DEFINED): ``site_total`` (n, n_regions) and ``latent_total`` (n, T, n_regions), float64, ``None`` where not
        wanted.  ``region`` (N,) holds 0 .. n_regions - 1, -1 = in no region; ``weight`` (N,) finite float64, ``None`` = 1.  The terms
        are ``deterministic``'s float32 first site and ``predictive``'s / ``predictive_scores``' latent state for the same ``seed``,
        bit for bit, times the weight in float64, summed in one fixed order (include/biolith_hip.h: bl_regional_totals).  Nothing of
        size (n, T, N) exists on the device or the host."""
        d = self._draw_matrix(draws)
        n = d.shape[0]
        r = np.ascontiguousarray(np.asarray(region).reshape(-1), dtype=np.int32)
        w = None if weight is None else np.ascontiguousarray(np.asarray(weight, dtype=np.float64).reshape(-1))
        if not (site or latent):
            raise ValueError("regional_totals(): neither total is wanted")
        if n == 0:
            raise ValueError("regional_totals(): no draws")
        if r.size != self.N or (w is not None and w.size != self.N):
            raise ValueError(f"regional_totals(): region and weight hold one entry per site ({self.N})")
        G = int(n_regions)
        out_site = np.empty((n, G)) if site else None
        out_latent = np.empty((n, self.T, G)) if latent else None
        _ffi.check(self._lib.bl_regional_totals(self._h, n, _fp(d), C.c_uint64(int(seed) & (2 ** 64 - 1)), G,
                                                r.ctypes.data_as(C.POINTER(C.c_int32)), _dp(w), _dp(out_site), _dp(out_latent)))
        return out_site, out_latent

    def response_curves(self, draws, side: int, covariate: int, values, weight=None):
        """Per draw of draws (n, D) and grid value, the weighted total over the sites of a deterministic site with one covariate set to
        the value at every site, fused on the device (BUILDER-DEFINED): (n, V) float64.  ``side`` 0 replaces site covariate
        ``covariate`` and totals the first site (``psi``; occu_rn, nmixture: ``abundance``); ``side`` 1 replaces observation covariate
        ``covariate`` at every visit and totals the second (``prob_detection``; occu_cop: ``rate_detection``) summed over a site's
        T J visits.  ``values`` (V,) finite float32; ``weight`` (N,) finite float64, ``None`` = 1.  The terms are ``deterministic``'s
        float32 values on the modified covariates, bit for bit, times the weight in float64, summed in ``regional_totals``' order for
        one region (include/biolith_hip.h: bl_response_curves).  Nothing of size (n, V, N) exists on the device or the host."""
        d = self._draw_matrix(draws)
        n = d.shape[0]
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1))
        w = None if weight is None else np.ascontiguousarray(np.asarray(weight, dtype=np.float64).reshape(-1))
        if n == 0:
            raise ValueError("response_curves(): no draws")
        if w is not None and w.size != self.N:
            raise ValueError(f"response_curves(): weight holds one entry per site ({self.N})")
        out = np.empty((n, v.size))
        _ffi.check(self._lib.bl_response_curves(self._h, n, _fp(d), int(side), int(covariate), int(v.size), _fp(v), _dp(w), _dp(out)))
        return out

    TRAJECTORY_OUTPUTS = ("occupancy", "colonised", "extinct", "equilibrium", "z", "z_colonised", "z_extinct")   # the C-ABI's order

    def trajectory_totals(self, draws, region, n_regions: int, n_periods: int, weight=None, seed: int = 0, outputs=TRAJECTORY_OUTPUTS):
        """Per draw of draws (n, D) of an occu_dyn handle and region, the weighted totals of the occupancy trajectory over
        ``n_periods`` = T seasons without the observations, fused on the device (BUILDER-DEFINED): a dict of float64 arrays under the
        names in ``outputs`` -- ``occupancy`` and ``z`` (n, T, n_regions), ``colonised``, ``extinct``, ``z_colonised`` and
        ``z_extinct`` (n, T - 1, n_regions), ``equilibrium`` (n, n_regions).  T is the call's, not the handle's: the kernel reads the
        site covariates and no visit.  ``region`` (N,) holds 0 .. n_regions - 1, -1 = in no region; ``weight`` (N,) finite float64,
        ``None`` = 1.  The terms are float64 throughout, the ``z`` totals those of one ancestral path per draw, a function of (seed,
        draw, T, period, site), summed in ``regional_totals``' fixed order (include/biolith_hip.h: bl_trajectory_totals).  Nothing of
        size (n, T, N) exists on the device or the host."""
        d = self._draw_matrix(draws)
        n, G, T = d.shape[0], int(n_regions), int(n_periods)
        r = np.ascontiguousarray(np.asarray(region).reshape(-1), dtype=np.int32)
        w = None if weight is None else np.ascontiguousarray(np.asarray(weight, dtype=np.float64).reshape(-1))
        unknown = [k for k in outputs if k not in self.TRAJECTORY_OUTPUTS]
        if unknown or not outputs:
            raise ValueError(f"trajectory_totals(): outputs must name some of {self.TRAJECTORY_OUTPUTS}, got {tuple(outputs)}")
        if n == 0:
            raise ValueError("trajectory_totals(): no draws")
        if r.size != self.N or (w is not None and w.size != self.N):
            raise ValueError(f"trajectory_totals(): region and weight hold one entry per site ({self.N})")
        rows = dict(occupancy=T, colonised=T - 1, extinct=T - 1, z=T, z_colonised=T - 1, z_extinct=T - 1)   # (T < 1: the C-ABI refuses it)
        out = {k: np.empty((n, G) if k == "equilibrium" else (n, max(rows[k], 0), G)) for k in self.TRAJECTORY_OUTPUTS if k in outputs}
        _ffi.check(self._lib.bl_trajectory_totals(self._h, n, _fp(d), C.c_uint64(int(seed) & (2 ** 64 - 1)), T, G,
                                                  r.ctypes.data_as(C.POINTER(C.c_int32)), _dp(w),
                                                  *[_dp(out.get(k)) for k in self.TRAJECTORY_OUTPUTS]))
        return out

    def species_richness(self, draws, region=None, n_regions: int = 0, weight=None, site: bool = True, area: bool = True):
        """The posterior of the number of species present, for draws (n, S, D) of S species sampled under one chain -- block ``s`` of a
        draw is species ``s``'s draw for THIS handle, whose site covariates are every species' --, fused on the device
        (BUILDER-DEFINED): ``pmf, expected_mean, expected_sd, area``, float64, ``None`` where not wanted.  Given a draw the species'
        presences at a site are independent Bernoulli(``psi_s``), ``psi_s`` ``deterministic``'s float32 value bit for bit, so their
        number is Poisson-binomial; its pmf is a float64 recursion over the species in ascending order.  With ``site``: ``pmf``
        (N, S + 1) the pmf averaged over the draws, ``expected_mean`` and ``expected_sd`` (N,) the mean and sd (ddof 1, NaN for one
        draw) of ``sum_s psi_s`` over the draws, every sum in draw order.  With ``area``: (n, S + 1, n_regions), row ``r`` the
        weighted area holding exactly ``r`` species, summed in ``regional_totals``' fixed order; ``region`` (N,) holds
        0 .. n_regions - 1, -1 = in no region, ``weight`` (N,) finite float64, ``None`` = 1; both are read for ``area`` alone
        (include/biolith_hip.h: bl_species_richness).  Nothing of size (n, N) exists on the device or the host."""
        d = np.asarray(draws, dtype=np.float32)
        if d.ndim != 3 or d.shape[-1] != self.D:
            raise ValueError(f"species_richness(): draws must be (n, n_species, {self.D}) for this dataset, got shape {d.shape}")
        d = np.ascontiguousarray(d)
        n, S = d.shape[0], d.shape[1]
        if not (site or area):
            raise ValueError("species_richness(): neither the site outputs nor the area is wanted")
        if n == 0:
            raise ValueError("species_richness(): no draws")
        if S > _ffi.RICHNESS_MAX_SPECIES:
            raise NotImplementedError(f"species_richness(): {S} species, at most {_ffi.RICHNESS_MAX_SPECIES} (BL_RICHNESS_MAX_SPECIES)")
        r = w = None
        G = int(n_regions)
        if area:
            if region is None:
                raise ValueError("species_richness(): the area needs region")
            r = np.ascontiguousarray(np.asarray(region).reshape(-1), dtype=np.int32)
            w = None if weight is None else np.ascontiguousarray(np.asarray(weight, dtype=np.float64).reshape(-1))
            if r.size != self.N or (w is not None and w.size != self.N):
                raise ValueError(f"species_richness(): region and weight hold one entry per site ({self.N})")
        pmf = np.empty((self.N, S + 1)) if site else None
        mean = np.empty(self.N) if site else None
        sd = np.empty(self.N) if site else None
        out_area = np.empty((n, S + 1, max(G, 0))) if area else None
        _ffi.check(self._lib.bl_species_richness(self._h, S, n, _fp(d), G, None if r is None else r.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 _dp(w), _dp(pmf), _dp(mean), _dp(sd), _dp(out_area)))
        return pmf, mean, sd, out_area

    def residual_moran(self, draws, graph=None, seed: int = 0, seed_rep: int = 1, moran: bool = True, site: bool = True):
        """Spatial autocorrelation of the residuals of Wright, Irvine and Higgs (2019) for draws (n, D), fused on the device
        (BUILDER-DEFINED): ``moran_occ, moran_det, det_sites, occ_mean, det_mean, n_occupied``, ``None`` where not wanted.  The
        handle carries the observations.  Per draw and period, with ``moran``: ``moran_occ`` (n, T, 2) Moran's I over ``graph`` of
        the occupancy residual ``z - psi`` -- ``z`` is ``site_posterior``'s for ``seed``, ``psi`` ``deterministic``'s, bit for bit
        -- and of its replicate, ``predictive``'s ``z`` for ``seed_rep``; ``moran_det`` (n, T, 2) the same of the site-level
        detection residual, the mean of ``y - prob_detection`` over the cell's seen visits at the sites the draw has occupied,
        and of its replicate (``predictive``'s ``y`` and ``z``); ``det_sites`` (n, T, 2) int32 the sites in each.  The residual is
        against ``prob_detection``, as the reference's ``residuals`` forms it, also on a handle with a false-positive rate.
        ``I`` is NaN where fewer than two sites are in the field, where the weights in it sum to 0 or where its values are all
        equal.  With ``site``, over all the draws in draw order: ``occ_mean`` (T, N) the mean occupancy residual, ``n_occupied``
        (T, N) int32 the draws in which the site is in the detection field, ``det_mean`` (T, N) the detection residual's mean over
        those draws, NaN where there is none.  ``graph`` is CSR ``(indptr, indices, data)``, ``data`` ``None`` = 1, and need not be
        symmetric; it is read for ``moran`` alone.  Every sum has a fixed order: the same call returns the same bytes
        (include/biolith_hip.h: bl_residual_moran)."""
        d = np.asarray(draws, dtype=np.float32)
        if d.ndim != 2 or d.shape[1] != self.D:
            raise ValueError(f"residual_moran(): draws must be (n, {self.D}) for this dataset, got shape {d.shape}")
        d = np.ascontiguousarray(d)
        n = d.shape[0]
        if not (moran or site):
            raise ValueError("residual_moran(): neither Moran's I nor the site outputs are wanted")
        if n == 0:
            raise ValueError("residual_moran(): no draws")
        ptr = idx = w = None
        nnz = 0
        if moran:
            if graph is None:
                raise ValueError("residual_moran(): Moran's I needs the neighbour graph")
            ptr = np.ascontiguousarray(np.asarray(graph[0]).reshape(-1), dtype=np.int32)
            idx = np.ascontiguousarray(np.asarray(graph[1]).reshape(-1), dtype=np.int32)
            w = None if graph[2] is None else np.ascontiguousarray(np.asarray(graph[2], dtype=np.float64).reshape(-1))
            if ptr.size != self.N + 1 or (w is not None and w.size != idx.size):
                raise ValueError(f"residual_moran(): the graph's indptr holds N + 1 = {self.N + 1} entries, its data one per index")
            nnz = int(idx.size)
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        m_occ = np.empty((n, self.T, 2)) if moran else None
        m_det = np.empty((n, self.T, 2)) if moran else None
        sites = np.empty((n, self.T, 2), dtype=np.int32) if moran else None
        o_mean = np.empty((self.T, self.N)) if site else None
        d_mean = np.empty((self.T, self.N)) if site else None
        n_occ = np.empty((self.T, self.N), dtype=np.int32) if site else None
        mask = 2 ** 64 - 1
        _ffi.check(self._lib.bl_residual_moran(self._h, n, _fp(d), C.c_uint64(int(seed) & mask), C.c_uint64(int(seed_rep) & mask), nnz,
                                               ip(ptr), ip(idx), _dp(w), _dp(m_occ), _dp(m_det), ip(sites), _dp(o_mean), _dp(d_mean),
                                               ip(n_occ)))
        return m_occ, m_det, sites, o_mean, d_mean, n_occ

    def _per_draw(self, fn, draws, seed, outs, pinned=True):
        """Calls a per-draw entry ``fn(handle, n, draws, seed, *outputs)`` for draws (n, D).  ``outs`` lists (wanted, shape behind
        the draw axis, dtype) per output; returns the arrays, ``None`` where not wanted.  With ``pinned`` the 4-byte outputs come from
        ``_big_empty``; the byte-sized ones never do."""
        d = self._draw_matrix(draws)
        n = d.shape[0]
        empty = lambda dt: self._big_empty if pinned and np.dtype(dt).itemsize == 4 else np.empty
        arrays = tuple(empty(dt)((n,) + shape, dtype=dt) if want else None for want, shape, dt in outs)
        if n:
            ptrs = [None if a is None else a.ctypes.data_as(C.POINTER(_CTYPE[a.dtype.type])) for a in arrays]
            _ffi.check(fn(self._h, n, _fp(d), C.c_uint64(int(seed) & (2 ** 64 - 1)), *ptrs))
            if pinned:
                _PINNED.kick(self._lib)
        return arrays

    def predictive(self, draws, seed: int = 0, latent: bool = True, y: bool = True):
        """Posterior predictive draws of the discrete sites for draws (n, D): the latent state
        (``z`` for occu / occu_cop, ``N_i`` for occu_rn / nmixture) as (n, T, N) and ``y`` as (n, J, T, N); uint8, or
        int32 for the count models
        (biolith/utils/predict.py:66-92; occu.py:208-241; occu_rn.py:194-221)."""
        counts = self.model in ("occu_cop", "nmixture")  # their sampled sites are counts: int32 (bl_predict_counts)
        dt = np.int32 if counts else np.uint8
        return self._per_draw(self._lib.bl_predict_counts if counts else self._lib.bl_predict, draws, seed,
                              [(latent, (self.T, self.N), dt), (y, (self.J, self.T, self.N), dt)], pinned=False)

    def predictive_check(self, draws, obs, seed: int = 0, by_site: bool = True, by_revisit: bool = True):
        """The posterior predictive check's discrepancies for draws (n, D), fused on the device: ``by_site`` and ``by_revisit``, each
        (n, 4) float64 = ``ft_obs, ft_rep, chi_obs, chi_rep`` (Freeman-Tukey and chi-squared, of the observed and of the replicate data)
        or ``None``.  ``obs`` is (N, T, J), NaN = not observed, else 0 / 1; the replicate is ``predictive(draws, seed)``'s ``y`` and the
        expectation ``deterministic``'s ``psi * prob_detection``, neither of which is materialised.  occu handles with or without false
        positives / random effects (include/biolith_hip.h: bl_predictive_check; posterior_predictive_check.py:17-160)."""
        o = np.asarray(obs, dtype=np.float32)
        if o.shape != (self.N, self.T, self.J):
            raise ValueError(f"obs must have shape (n_sites, n_periods, n_replicates) = {(self.N, self.T, self.J)}, got {o.shape}")
        seen = np.isfinite(o)
        if not np.isin(o[seen], (0.0, 1.0)).all():
            raise ValueError("obs must hold 0, 1 or NaN")
        o8 = np.ascontiguousarray(np.where(seen, o, 255.0).astype(np.uint8).transpose(2, 1, 0))   # (J, T, N)
        fn = lambda h, n, d, s, *outs: self._lib.bl_predictive_check(h, n, d, s, o8.ctypes.data_as(C.POINTER(C.c_uint8)), *outs)
        return self._per_draw(fn, draws, seed, [(by_site, (4,), np.float64), (by_revisit, (4,), np.float64)], pinned=False)

    def predictive_check_counts(self, draws, obs, seed: int = 0, by_site: bool = True, by_revisit: bool = True):
        """``predictive_check`` for the abundance and count models (BUILDER-DEFINED): ``by_site`` and ``by_revisit``, each (n, 4) float64
        = ``ft_obs, ft_rep, chi_obs, chi_rep`` or ``None``, for draws (n, D).  ``obs`` is (N, T, J): non-negative whole counts (occu_rn:
        0 / 1), NaN = not observed.  The replicate is ``predictive(draws, seed)``'s ``y``; the expectation is the model's mean of ``y``
        with the latent state summed out, from ``deterministic``'s float32 sites; neither is materialised.  occu_rn, nmixture and
        occu_cop handles with or without a false-positive rate / random effects (include/biolith_hip.h: bl_predictive_check_counts)."""
        o = np.asarray(obs, dtype=np.float64)
        if o.shape != (self.N, self.T, self.J):
            raise ValueError(f"obs must have shape (n_sites, n_periods, n_replicates) = {(self.N, self.T, self.J)}, got {o.shape}")
        seen = ~np.isnan(o)
        whole = o[seen]
        if not (np.isfinite(whole).all() and (whole >= 0).all() and (whole == np.floor(whole)).all() and (whole < 2 ** 31).all()):
            raise ValueError("obs must hold non-negative whole counts or NaN")
        if self.model == "occu_rn" and (whole > 1).any():
            raise ValueError("obs must hold 0, 1 or NaN (occu_rn)")
        o32 = np.ascontiguousarray(np.where(seen, o, -1.0).astype(np.int32).transpose(2, 1, 0))   # (J, T, N)
        fn = lambda h, n, d, s, *outs: self._lib.bl_predictive_check_counts(h, n, d, s, o32.ctypes.data_as(C.POINTER(C.c_int32)), *outs)
        return self._per_draw(fn, draws, seed, [(by_site, (4,), np.float64), (by_revisit, (4,), np.float64)], pinned=False)

    def predictive_density(self, draws, obs, seed: int = 0, marginal: bool = False, per_draw: bool = True, point_lse: bool = True,
                           point_var: bool = True):
        """The pointwise log-likelihood of ``obs`` under draws (n, D), reduced on the device without being stored: ``per_draw`` (n,)
        = its sum over the points per draw; ``point_lse`` (N, T, J) = ``log mean exp`` over the draws per point; ``point_var`` (N, T, J) =
        its variance over the draws, ddof 1 (0 for one draw); float64, or ``None``.  ``obs`` is (N, T, J): 0 / 1, NaN = not a point (the
        caller folds the covariate masks in), where both point outputs are 0.  ``marginal=False`` is the log-likelihood at
        ``predictive(draws, seed)``'s ``z`` (evaluation.log_likelihood), ``True`` the marginal ``psi * p`` form
        (log_likelihood_manual).  occu handles with or without false positives / random effects (include/biolith_hip.h:
        bl_predictive_density)."""
        o = np.asarray(obs, dtype=np.float32)
        if o.shape != (self.N, self.T, self.J):
            raise ValueError(f"obs must have shape (n_sites, n_periods, n_replicates) = {(self.N, self.T, self.J)}, got {o.shape}")
        seen = np.isfinite(o)
        if not np.isin(o[seen], (0.0, 1.0)).all():
            raise ValueError("obs must hold 0, 1 or NaN")
        o8 = np.ascontiguousarray(np.where(seen, o, 255.0).astype(np.uint8).transpose(2, 1, 0))   # (J, T, N)
        d = self._draw_matrix(draws)
        n = d.shape[0]
        out_draw = np.zeros(n) if per_draw else None
        out_lse, out_var = (np.zeros((self.J, self.T, self.N)) if want else None for want in (point_lse, point_var))
        if n:
            ptrs = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_double)) for a in (out_draw, out_lse, out_var)]
            _ffi.check(self._lib.bl_predictive_density(self._h, n, _fp(d), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                       o8.ctypes.data_as(C.POINTER(C.c_uint8)), int(bool(marginal)), *ptrs))
        return (out_draw,) + tuple(None if a is None else a.transpose(2, 1, 0) for a in (out_lse, out_var))

    def site_posterior(self, draws, seed: int = 0, log_lik: bool = True, z_prob: bool = True, z: bool = True):
        """Conditional occupancy for draws (n, D), each output (n, T, N): ``log_lik`` float32, the z-marginalised log-likelihood of a
        (period, site)'s unmasked observations; ``z_prob`` float32 = P(z = 1 | those observations, theta); ``z`` uint8 ~
        Bernoulli(z_prob), a function of (seed, draw, period, site).  occu (false positives, random effects) and occu_comb handles
        (include/biolith_hip.h: bl_site_posterior); no counterpart in the reference."""
        cell = (self.T, self.N)
        return self._per_draw(self._lib.bl_site_posterior, draws, seed,
                              [(log_lik, cell, np.float32), (z_prob, cell, np.float32), (z, cell, np.uint8)])

    def abundance_posterior(self, draws, seed: int = 0, log_lik: bool = True, n_mean: bool = True, occ_prob: bool = True, n_draw: bool = True):
        """Conditional abundance for draws (n, D), each output (n, T, N): ``log_lik`` float32, the N-marginalised log-likelihood of a
        (period, site)'s unmasked observations; ``n_mean`` float32 = E[N | those observations, theta]; ``occ_prob`` float32 =
        P(N > 0 | those observations, theta); ``n_draw`` int32, one draw of N given them, a function of (seed, draw, period, site).
        occu_rn (false-positive rate, random effects) and nmixture (random effects) handles (include/biolith_hip.h:
        bl_abundance_posterior); no counterpart in the reference."""
        cell = (self.T, self.N)
        return self._per_draw(self._lib.bl_abundance_posterior, draws, seed,
                              [(log_lik, cell, np.float32), (n_mean, cell, np.float32), (occ_prob, cell, np.float32), (n_draw, cell, np.int32)])

    def path_posterior(self, draws, seed: int = 0, log_lik: bool = True, z_prob: bool = True, col_prob: bool = True, ext_prob: bool = True,
                       z: bool = True):
        """Conditional dynamics of an occu_dyn handle for draws (n, D): ``log_lik`` (n, N) float32, the site's path-marginalised
        log-likelihood; ``z_prob`` (n, T, N) float32 = P(z_t = 1 | all seasons' data, theta), the smoothed marginal; ``col_prob`` /
        ``ext_prob`` (n, T - 1, N) float32 = P(z_t = 0, z_t+1 = 1 | .) / P(z_t = 1, z_t+1 = 0 | .); ``z`` (n, T, N) uint8, one joint
        draw of the path by forward filtering, backward sampling, a function of (seed, draw, period, site)
        (include/biolith_hip.h: bl_path_posterior); builder-defined like the model."""
        cell, pair = (self.T, self.N), (self.T - 1, self.N)
        return self._per_draw(self._lib.bl_path_posterior, draws, seed,
                              [(log_lik, (self.N,), np.float32), (z_prob, cell, np.float32), (col_prob, pair, np.float32),
                               (ext_prob, pair, np.float32), (z, cell, np.uint8)])

    def score_posterior(self, draws, seed: int = 0, visits: bool = True):
        """Conditional scores of an occu_cs handle for draws (n, D): ``log_lik`` (n, T, N) float32, the cell's log-likelihood with z and
        every f summed out; ``z_prob`` (n, T, N) float32 = P(z = 1 | the cell's scores, theta); ``z`` (n, T, N) uint8 ~ Bernoulli(z_prob);
        ``f_prob`` (n, J, T, N) float32 = P(f_j = 1 | the cell's scores, theta), whether recording j was a true positive; ``f``
        (n, J, T, N) uint8, drawn jointly with ``z`` (``f <= z``).  ``z`` and ``f`` are functions of (seed, draw, period, site), and ``z``
        is the same with and without ``visits``; ``visits=False`` skips the two replicate-level outputs (``None``)
        (include/biolith_hip.h: bl_score_posterior); no counterpart in the reference."""
        cell, visit = (self.T, self.N), (self.J, self.T, self.N)
        return self._per_draw(self._lib.bl_score_posterior, draws, seed,
                              [(True, cell, np.float32), (True, cell, np.float32), (True, cell, np.uint8),
                               (visits, visit, np.float32), (visits, visit, np.uint8)])

    def count_posterior(self, draws, seed: int = 0, visits: bool = True):
        """Conditional counts of an occu_cop handle for draws (n, D): ``log_lik`` (n, T, N) float32, the cell's log-likelihood with z
        summed out (the Poisson pmf's parameter-free part included); ``z_prob`` (n, T, N) float32 = P(z = 1 | the cell's counts, theta);
        ``z`` (n, T, N) uint8 ~ Bernoulli(z_prob); ``true_mean`` (n, J, T, N) float32 = z_prob y_j rho_j, the expected number of visit
        j's counted detections that were real, rho_j = lambda_j / (lambda_j + rate_fp_constant); ``true_count`` (n, J, T, N) int32 =
        z Binomial(y_j, rho_j), drawn jointly with ``z`` (``true_count <= z y``).  ``z`` and ``true_count`` are functions of (seed, draw,
        period, site), and ``z`` is the same with and without ``visits``; ``visits=False`` skips the two visit-level outputs (``None``)
        (include/biolith_hip.h: bl_count_posterior); no counterpart in the reference."""
        cell, visit = (self.T, self.N), (self.J, self.T, self.N)
        return self._per_draw(self._lib.bl_count_posterior, draws, seed,
                              [(True, cell, np.float32), (True, cell, np.float32), (True, cell, np.uint8),
                               (visits, visit, np.float32), (visits, visit, np.int32)])

    def predictive_comb(self, draws, seed: int = 0, z: bool = True, y_pc: bool = True, y_aru: bool = True, scores: bool = True):
        """Posterior predictive of an occu_comb handle for draws (n, D), all three observed sites withheld: ``z`` (n, T, N) uint8 ~
        Bernoulli(psi); ``y_pc`` (n, Jpc, T, N) and ``y_aru`` (n, Jaru, T, N) uint8; ``scores`` (n, Js, T, N) float32.  Every output is
        a function of (seed, draw, period, site) only and does not depend on which others are asked for (``None`` where not wanted)
        (include/biolith_hip.h: bl_predict_comb); builder-defined: the reference's predict cannot withhold the scores."""
        cell = (self.T, self.N)
        return self._per_draw(self._lib.bl_predict_comb, draws, seed,
                              [(z, cell, np.uint8), (y_pc, (self.J,) + cell, np.uint8), (y_aru, (getattr(self, "Ja", 0),) + cell, np.uint8),
                               (scores, (getattr(self, "Js", 0),) + cell, np.float32)])   # (another model's handle: the entry refuses it)

    def deterministic_comb(self, draws, psi: bool = True, pc_prob: bool = True, aru_prob: bool = True):
        """occu_comb's deterministic sites for draws (n, D): ``psi`` (n, T, N), ``PC_prob_detection`` (n, Jpc, T, N) and
        ``ARU_prob_detection`` (n, Jaru, T, N), float32, ``None`` where not wanted (include/biolith_hip.h: bl_deterministic_comb;
        occu_comb.py:224-331)."""
        cell = (self.T, self.N)
        fn = lambda h, n, d, seed, *outs: self._lib.bl_deterministic_comb(h, n, d, *outs)   # (the entry takes no seed)
        return self._per_draw(fn, draws, 0, [(psi, cell, np.float32), (pc_prob, (self.J,) + cell, np.float32),
                                             (aru_prob, (getattr(self, "Ja", 0),) + cell, np.float32)])


def _predictive_scores(self, draws, seed: int = 0):
    """occu_cs: posterior predictive ``z`` (n, T, N), ``f`` (n, J, T, N) as uint8 and the scores ``s`` (n, J, T, N) float32
    (biolith/models/occu_cs.py:196-232 with obs withheld)."""
    visit = (self.J, self.T, self.N)
    return self._per_draw(self._lib.bl_predict_scores, draws, seed,
                          [(True, (self.T, self.N), np.uint8), (True, visit, np.uint8), (True, visit, np.float32)], pinned=False)


OccuDataset.predictive_scores = _predictive_scores


def rng_streams(seed: int, chain: int, nstreams: int = _ffi.RNG_STREAMS_PER_CHAIN) -> np.ndarray:
    out = np.zeros((nstreams, 4), dtype=np.uint32)
    _ffi.check(_ffi.load().bl_rng_streams(int(seed), int(chain), int(nstreams),
                                          out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def adaptation_schedule(num_warmup: int):
    s = (C.c_int32 * 40)()
    e = (C.c_int32 * 40)()
    n = _ffi.load().bl_adaptation_schedule(int(num_warmup), s, e, 40)
    return [(s[i], e[i]) for i in range(n)]


def psis_loo(log_lik, device: int = 0, cells_per_launch: int = 0):
    """PSIS-LOO of every cell of a log-likelihood array ``(n, ...)``: ``(elpd, pareto_k, lppd)``, float64 of shape ``log_lik.shape[1:]``
    (include/biolith_hip.h: bl_psis_loo, where the definition is).  ``log_lik`` is what any conditional posterior returns; it is passed
    as float32.  A cell whose column holds a non-finite value is NaN in all three.  ``cells_per_launch`` (0: chosen by the library) only
    sets how many cells travel to the device together; it changes no bit of the result."""
    ll = np.asarray(log_lik, dtype=np.float32)
    if ll.ndim < 1:
        raise ValueError("psis_loo(): log_lik must have the draws on its first axis")
    shape = ll.shape[1:]
    ll = np.ascontiguousarray(ll.reshape(ll.shape[0], -1))
    outs = [np.empty(ll.shape[1], dtype=np.float64) for _ in range(3)]
    _ffi.check(_ffi.load().bl_psis_loo(int(device), int(ll.shape[0]), int(ll.shape[1]), _fp(ll), int(cells_per_launch), *map(_dp, outs)))
    return tuple(o.reshape(shape) for o in outs)
