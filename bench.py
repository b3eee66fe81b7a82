#!/usr/bin/env python3
"""Headline benchmark: effective samples / second of psi for occu NUTS on 10k sites x 5 visits.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one complete pass of the hot path over the workload BASELINE.json's metric is quoted
on (its configs[1]): simulate(n_sites=10000, 3 site + 3 obs covariates, 5 visits), 4 chains per
GPU x (1000 warmup + 1000 draws) of NUTS, i.e. exactly what ``fit(occu, **data, num_chains=4)``
runs behind the C-ABI.  The dataset is resident in HBM before the timed region.  With N > 1 GPUs
every rank runs its own 4 chains (weak scaling; chains are the unit the path shards over, no
data-path collective) and the result blocks are all-gathered over RCCL (``bl_gather_draws``, on librccl
behind the C-ABI) inside the timed region.  ESS is computed afterwards with the NumPyro estimator
(mean over sites of per-site ESS of psi).

A plain run does only what the headline figure needs: set up, W untimed steps, K timed steps, ESS, the result line
(and ``--dump-outputs DIR``: the last timed step's result arrays as DIR/<name>.npy).  ``--full`` adds everything else,
after the timed region: the end-to-end ``fit()`` clock, the CPU baseline, the live PMC passes, the verbose record file,
and (--gpus 1, workload occu) a ``secondary`` array: BASELINE.json configs[3] (occu_rn), the SURVEY section 8 row f3
workload (occu with site random effects) and the stacked-period stand-in of configs[4] (no reference counterpart), each a
few steps with its own ``roofline`` and a bounded-sample ``cpu_baseline`` (``--no-secondary`` skips them).

``--gpus N`` with N > 1 and no WORLD_SIZE in the environment: this process is only a LAUNCHER.  It starts N
fresh child processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, one per GPU) before importing torch or
touching HIP, relays rank 0's JSON line and exits non-zero if any rank fails (e.g. fewer than N GPUs).
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CFG2 = dict(n_sites=10000, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=35, session_duration=7, random_seed=0)
CFG4 = dict(n_sites=5000, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=70, session_duration=7, random_seed=0)
CHAINS_PER_GPU = 4   # default; --chains-per-gpu C overrides it for every workload (BASELINE.json configs[2]: --gpus 8 --chains-per-gpu 1)
CFG5S = dict(n_sites=2000, n_periods=8, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=28, session_duration=7, random_seed=0)
# --workload: "occu" is the headline (BASELINE.json configs[1], what the driver runs); the others are the secondary lines
# (same JSON shape): "occu_rn" = configs[3] (metric on `abundance`), "occu_re" = SURVEY section 8 row f3, "occu_stacked" = the
# stacked-period stand-in of configs[4].  The default run appends them, shortened, as `secondary` (SECONDARY below).
WORKLOADS = {
    # cpu_sample: the oracle leg runs the SAME 4 chains x (1000 + 1000) as the GPU (about 45 s on 4 cores of this class)
    "occu": dict(model="occu", cfg=CFG2, num_warmup=1000, num_samples=1000, cpu_sample=(1000, 1000), site="psi",
                 metric="effective samples/sec (psi) for occu NUTS, 10k sites x 5 visits",
                 text="biolith simulate(n_sites=10000, n_site_covs=3, n_obs_covs=3, 5 visits, seed 0); fit(occu)"),
    # BASELINE.json configs[0]: simulate()'s own defaults (100 sites x 52 visits, one covariate each; occu.py:251-252, 336), 2 chains --
    # the many-visits regime, where a site pair is shared by a group of lanes (occu_device.hpp: bl_eval_sites_grp)
    "occu_cfg1": dict(model="occu", cfg=dict(random_seed=0), chains=2, num_warmup=1000, num_samples=1000, cpu_sample=(1000, 1000), site="psi",
                      metric="effective samples/sec (psi) for occu NUTS, simulate() defaults: 100 sites x 52 visits, 2 chains",
                      text="biolith simulate() defaults (100 sites, 52 visits, 1 + 1 covariates, seed 0); fit(occu, num_chains=2)"),
    # (cpu_sample: --cpu-baseline runs the oracle's OWN sampler, 4 x (200 + 200), a few minutes on 4 cores -- the measured figure of
    # profiles/r05/e_cpu_baseline_rn.json; the default run's secondary line carries the scaled estimate)
    "occu_rn": dict(model="occu_rn", cfg=CFG4, num_warmup=1000, num_samples=1000, cpu_sample=(200, 200), site="abundance",
                    metric="effective samples/sec (abundance) for occu_rn NUTS, 5k sites x 10 visits",
                    text="biolith simulate_rn(n_sites=5000, n_site_covs=3, n_obs_covs=3, 10 visits, seed 0); "
                         "fit(occu_rn, max_abundance=100)"),
    # SURVEY section 8 row f3 (no BASELINE config of its own): occu with site random effects, 20 009 coordinates.  (With
    # observation effects as well the Bernoulli data leave obs_re_sd and the detection coefficients nearly unidentified: NUTS
    # mixes in neither the reference's parameterisation nor here, R-hat > 2 -- not a throughput workload.)
    "occu_re": dict(model="occu_re", cfg=dict(n_sites=10000, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=70, session_duration=7,
                                              site_random_effects=True, random_seed=0),
                    num_warmup=1000, num_samples=1000, cpu_sample=(20, 20), site="psi",
                    options=dict(site_random_effects=True),
                    metric="effective samples/sec (psi) for occu NUTS with site random effects, 10k sites x 10 visits",
                    text="biolith simulate(n_sites=10000, n_site_covs=3, n_obs_covs=3, 10 visits, site random effects, seed 0); "
                         "fit(occu, site_random_effects=True)"),
    # BASELINE.json configs[4] names a dynamic (colonisation / extinction) model the reference does not have;
    # its nearest reference behaviour is the stacked-period form (occu.py:198-210: psi shared by the periods), at the stated size.
    "occu_stacked": dict(model="occu", cfg=CFG5S, num_warmup=1000, num_samples=1000, cpu_sample=(100, 100), site="psi",
                         metric="effective samples/sec (psi) for occu NUTS, 2k sites x 8 stacked periods x 4 visits (configs[4] stand-in: "
                                "no reference counterpart for the dynamic model)",
                         text="biolith simulate(n_sites=2000, n_periods=8, n_site_covs=3, n_obs_covs=3, 4 visits per period, seed 0); fit(occu)"),
    # ... and the dynamic model itself, BUILDER-DEFINED (models/occu_dyn.py, csrc/dyn_device.hpp): initial occupancy, colonisation,
    # extinction, the latent paths summed by the forward recursion in the kernel.  Parity against the builder's own oracle only.
    "occu_dyn": dict(model="occu_dyn", cfg=dict(n_sites=2000, n_periods=8, n_site_covs=3, n_obs_covs=3, deployment_days_per_site=28,
                                                 session_duration=7, random_seed=0),
                     num_warmup=1000, num_samples=1000, cpu_sample=(100, 100), site="psi",
                     metric="effective samples/sec (initial psi) for dynamic-occupancy NUTS (colonisation / extinction, forward algorithm), "
                            "2k sites x 8 seasons x 4 visits (configs[4] as worded: builder-defined model, no reference counterpart)",
                     text="biolith_amd simulate_dyn(n_sites=2000, n_periods=8, n_site_covs=3, n_obs_covs=3, 4 visits per season, seed 0); fit(occu_dyn)"),
}
# (workload, timed steps, untimed steps) appended to the default run's line; each with a bounded cpu_baseline
SECONDARY = (("occu_rn", 3, 1), ("occu_re", 2, 1), ("occu_stacked", 3, 1), ("occu_dyn", 3, 1), ("occu_cfg1", 3, 1))
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
# Transcendental (v_exp / v_log / v_rcp ...) issue rate: a wave64 instruction costs 8 issue cycles where an FMA costs 4
# (MI355X_MICROARCH.md:489, row "vector-instruction ISSUE cost") = 8 lanes per SIMD per cycle, 4 SIMDs per CU = 32 lanes per clock
# per CU at 2.4 GHz = 76.8 G per second per CU; 256 CUs.
TRANS_PER_CU_PER_S = 32 * 2.4e9
# the measured CPU figure of BASELINE.json configs[3] (the oracle's own sampler, 4 x (200 + 200), two minutes on 4 cores): too long for
# the default run, so the line quotes the committed record and keeps the live scaled estimate beside it
RN_CPU_MEASURED = "profiles/r05/e_cpu_baseline_rn.json"
N_CUS = 256
# ESS(psi) of a 10k-site step costs about a second of host time on one thread (a third of that on ESS_WORKERS_MAX): it is computed
# for at most this many timed steps, spread evenly over the run (the first and the last included), and their mean stands for every
# step; a run of this many steps or fewer evaluates each of them, as before
ESS_STEPS_MAX = 40
ESS_WORKERS_MAX = 8
DUMP_LIMIT_BYTES = 63 * 10 ** 6   # --dump-outputs: under 64 MB in all, the .npy headers included


COMPACT_LIMIT = 4096   # bytes: the driver keeps an 8 KB tail of stdout; BENCH_r05 lost its 19.5 KB line to that


def _short(x, n=120):
    """A note of at most n characters (the compact line carries no paragraphs)."""
    x = str(x)
    return x if len(x) <= n else x[: n - 3] + "..."


def _num(x, sig=7):
    """Floats rounded to `sig` significant figures; non-finite -> None (the line is strict JSON: allow_nan=False)."""
    import math

    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    x = float(x)
    if not math.isfinite(x):
        return None
    return float(f"{x:.{sig}g}")


def compact_line(out, full_path=None):
    """The LAST stdout line: what benchmarks/occu_spoccupancy.py:104-113 prints (the number) in the driver's contract, at most
    COMPACT_LIMIT bytes, strict JSON.  The verbose record (full secondary workloads, long notes) goes to `full_path`."""
    rf, cb, cfg = out.get("roofline", {}), out.get("cpu_baseline"), out.get("config", {})
    line = {k: _num(out[k]) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                      "vs_baseline", "dtype", "data", "rccl_world", "gather_hung") if k in out}
    line["metric"] = _short(line.get("metric", ""), 160)
    line["config"] = {k: (_short(cfg[k], 200 if k == "workload" else 120) if isinstance(cfg[k], str) else cfg[k])
                      for k in ("workload", "chains_per_gpu", "total_chains", "num_warmup", "num_samples", "parallelism", "wgs_per_chain", "gather", "env_overrides")
                      if k in cfg}
    line["roofline"] = {k: (_short(rf[k]) if isinstance(rf[k], str) else _num(rf[k]))
                        for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "bytes_per_gradient_evaluation",
                                  "gradient_evaluations_per_launch", "us_per_leapfrog_per_chain", "latency_floor_us",
                                  "executed_terms_per_evaluation", "frac_executed") if k in rf}
    if cb is not None:
        line["cpu_baseline"] = {k: (_short(cb[k]) if isinstance(cb[k], str) else _num(cb[k]))
                                for k in ("value", "unit", "cores", "kind", "scaled") if k in cb}
        line["cpu_baseline"]["sample"] = _short(cb.get("sample_short", cb.get("sample", "")))
    elif "cpu_baseline_error" in out:
        line["cpu_baseline_error"] = _short(out["cpu_baseline_error"])
    for k in ("gpu_over_cpu", "fit_e2e_ms", "value_e2e"):
        if k in out:
            line[k] = _num(out[k])
    if "secondary_summary" in out:
        # [value ESS/s, ms_per_step, us_per_leapfrog_per_chain, roofline.frac, cpu_baseline.value]
        line["secondary_summary"] = out["secondary_summary"]
    if full_path:
        line["full_record"] = full_path
    s = json.dumps(line, allow_nan=False)
    if len(s) > COMPACT_LIMIT:   # (cannot happen with the caps above; never print an over-long line)
        for k in ("secondary_summary", "full_record", "value_e2e", "fit_e2e_ms"):
            line.pop(k, None)
        s = json.dumps(line, allow_nan=False)
    return s


def write_full_record(out, path):
    """The verbose record beside the compact line (gpurun_out/ travels back from the GPU box; profiles/ keeps the judged copies)."""
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f)
            f.write("\n")
        return os.path.relpath(path, ROOT)
    except OSError:
        return None


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline", action="store_true",
                    help="secondary workloads: time the oracle's own sampler on a short run (minutes on 4 cores) instead of the "
                         "bounded, scaled sample of its evaluations")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end fit() timing (fit_e2e_ms / value_e2e)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary workloads of the default run")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="roofline.traffic from profiles/pmc_traffic.json instead of the two rocprofv3 --pmc passes this run makes over a child process")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)   # the child those passes profile: launches only
    ap.add_argument("--wgs-per-chain", type=int, default=0)
    ap.add_argument("--chains-per-gpu", type=int, default=0,
                    help="chains every rank runs (default: the workload's own, 4 for the headline); BASELINE.json configs[2] "
                         "(8 chains sharded 1 per GPU) is --gpus 8 --chains-per-gpu 1")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="occu")
    ap.add_argument("--full-out", default=None,
                    help="where the verbose record goes (default gpurun_out/bench_full[_<workload>].json); stdout's last line is the compact one")
    ap.add_argument("--full-line", action="store_true", help="print the verbose record as the one stdout line (tools/; not what the driver reads)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the end-to-end fit() timing, the CPU baseline, the live PMC passes, the secondary "
                         "workloads and the verbose record file (a plain run does none of these; the --no-* flags trim --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's result arrays (draws, diverging, num_steps, ...) as DIR/<name>.npy, float32 or float64")
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------ launcher ----
def launch_ranks(args, argv):
    """--gpus N > 1 without a torchrun environment: start N rank processes (fresh interpreters; nothing in THIS process has
    imported torch or touched HIP), one per GPU, and relay rank 0's line.  Mirrors chain_method="parallel" (fit.py:109-113)."""
    import socket

    n = args.gpus
    # the rendezvous port: bound and released here, taken again by rank 0's store a moment later (a race with another process of
    # this host is possible in principle; BENCH_MASTER_PORT overrides)
    port = int(os.environ.get("BENCH_MASTER_PORT", "0"))
    if port == 0:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    # every rank's stderr (and rank 0's stdout: a pipe would block a chatty rank 0 at 64 KB) goes to a file, so that a failed
    # N-rank run leaves evidence: gpurun_out/ travels back from the GPU box
    logdir = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(logdir, exist_ok=True)
    except OSError:
        import tempfile

        logdir = tempfile.mkdtemp(prefix="bench_ranks_")
    procs, files = [], []
    out0_path = os.path.join(logdir, "rank0.out")
    for r in range(n):
        # HSA_ENABLE_IPC_MODE_LEGACY=0: this pool's host driver only supports dmabuf IPC; without it RCCL's buffer sharing across
        # processes fails with "hipIpcGetMemHandle: invalid argument"
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), BENCH_LAUNCHED_BY="bench.py", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        ferr = open(os.path.join(logdir, f"rank{r}.err"), "w")
        fout = open(out0_path, "w") if r == 0 else subprocess.DEVNULL
        files += [ferr] + ([fout] if r == 0 else [])
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env, stdout=fout, stderr=ferr))
    out0 = None
    failed = None
    deadline = time.monotonic() + float(os.environ.get("BENCH_LAUNCH_TIMEOUT", "3000"))
    pending = set(range(n))
    while pending and failed is None:
        for r in sorted(pending):
            rc = procs[r].poll()
            if rc is None:
                continue
            pending.discard(r)
            if rc != 0:
                failed = (r, rc)
                break
        if time.monotonic() > deadline:
            failed = (-1, 124)
        if pending and failed is None:
            time.sleep(0.05)
    if failed is not None:
        for p in procs:   # the exact processes started above, nothing else
            if p.poll() is None:
                p.kill()
    for p in procs:
        p.wait()
    for f in files:
        f.close()
    if failed is not None:
        sys.stderr.write(f"bench.py: rank {failed[0]} of {n} failed (exit code {failed[1]}); no result line; the ranks' stderr is in {logdir}/rank<r>.err\n")
        if failed[0] >= 0:
            try:
                with open(os.path.join(logdir, f"rank{failed[0]}.err")) as f:
                    sys.stderr.write("".join(f.readlines()[-15:]))
            except OSError:
                pass
        raise SystemExit(failed[1] if 0 < failed[1] < 256 else 1)
    with open(out0_path) as f:
        out0 = f.read()
    line = [ln for ln in (out0 or "").splitlines() if ln.startswith("{")]
    if not line:
        sys.stderr.write("bench.py: rank 0 printed no JSON line\n")
        raise SystemExit(1)
    print(line[-1])


# --------------------------------------------------------------------------------------------- helpers ----
def workload_chains(wl, chains_per_gpu=0):
    """Chains per GPU of a workload: --chains-per-gpu if given, else the workload's own (BASELINE configs[0]: 2), else 4."""
    return int(chains_per_gpu) if chains_per_gpu and chains_per_gpu > 0 else int(wl.get("chains", CHAINS_PER_GPU))


def rank_shard(rank, chains):
    """The chains rank `rank` runs (fit.py:109-113, chain_method="parallel"): `chains` consecutive global chain ids starting at
    rank x chains; a chain's xoshiro streams depend on its global id only, so N ranks x C chains are the chains of one N C-chain launch."""
    return dict(num_chains=int(chains), chain_offset=int(rank) * int(chains))


def algorithmic_bytes_per_eval(N, T, J, Ks, Ko, S=1):
    """float32 bytes one potential+gradient evaluation of one chain must read."""
    return 4 * (N * Ks + N * T * J * Ko + S * N * T * J)


def rn_executed_terms(data, theta, Ks, K=100, chunk=8, nats=20.0):
    """(n, visit) terms the Royle-Nichols evaluator EXECUTES per gradient evaluation at coefficients `theta` (the posterior mean of the
    run): every site keeps the n whose term is within `nats` of its largest (rn_device.hpp's rule, restated in NumPy as
    tools/rn_workload_stats.py does), in items of `chunk` consecutive n over all J visits; a site without a detection has a closed
    form and no items (rn_device.hpp).  Returns (executed, items)."""
    import numpy as np
    from scipy.special import gammaln

    X = np.asarray(data["site_covs"], dtype=np.float64)
    W = np.asarray(data["obs_covs"], dtype=np.float64)
    Y = np.asarray(data["obs"], dtype=np.float64)
    W = W.reshape(W.shape[0], -1, W.shape[-1])                 # (N, T, J, Ko) -> (N, T J, Ko); one period at configs[3]
    Y = (Y[0] if Y.ndim == 4 else Y).reshape(X.shape[0], -1)  # (species, N, T, J) -> (N, T J); NaN = a missing visit (neither branch)
    beta, alpha = theta[: Ks + 1], theta[Ks + 1:]
    eta, nu = beta[0] + X @ beta[1:], alpha[0] + W @ alpha[1:]
    lq = -np.logaddexp(0.0, nu)
    n = np.arange(0, K + 1)
    a = eta + np.where(Y == 0, lq, 0.0).sum(1)
    L = n[None, :] * a[:, None] - gammaln(n + 1)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        L = L + np.where((Y == 1)[:, :, None], np.log1p(-np.exp(lq[:, :, None] * n[None, None, :])), 0.0).sum(1)
    keep = L >= L.max(1)[:, None] - nats
    cut = np.array([np.max(np.nonzero(k)[0]) for k in keep])
    detected = np.nansum(Y == 1, axis=1) > 0      # (a site without a detection is in closed form since round 6: no items)
    items = int((np.ceil(cut / chunk).clip(1) * detected).sum())
    return items * chunk * Y.shape[1], items


def psi_draws(draws, X, site="psi", effects=None):
    """draws (C, S, D) -> psi (C, S, N) float32 = sigmoid(beta0 + X beta)  (occu.py:198-207), or
    abundance = exp(beta0 + X beta) for occu_rn (occu_rn.py:192).  effects: (C, S, N) site_re_occ draws of these sites."""
    import numpy as np

    Ks = X.shape[1]
    eta = draws[..., :1] + draws[..., 1:Ks + 1] @ X.T
    if effects is not None:
        eta = eta + effects
    return (np.exp(eta) if site == "abundance" else 1.0 / (1.0 + np.exp(-eta))).astype(np.float32)


def ess_of_site_function(draws, X, site="psi", chunk=1000, o_u=None, workers=1):
    """Mean over sites of ESS(psi_i) (or abundance_i), computed over site chunks so that the (chains, draws, sites)
    array of the deterministic site never exists as a whole (8 GPUs x 4 chains x 1000 draws x 10 000 sites).  `workers` > 1
    evaluates the chunks on that many threads; the chunk sums are added in site order either way (the same float)."""
    from concurrent.futures import ThreadPoolExecutor

    from biolith_amd.evaluation import effective_sample_size

    n = X.shape[0]

    def chunk_sum(s0):
        eff = None if o_u is None else draws[..., o_u + s0: o_u + min(s0 + chunk, n)]   # random effects: psi_i carries site_re_occ_i
        return float(effective_sample_size(psi_draws(draws, X[s0:s0 + chunk], site, eff)).sum())

    if workers > 1:
        with ThreadPoolExecutor(max_workers=workers) as ex:
            sums = list(ex.map(chunk_sum, range(0, n, chunk)))
    else:
        sums = [chunk_sum(s0) for s0 in range(0, n, chunk)]
    total = 0.0
    for s in sums:
        total += s
    return total / n


def host_workers():
    """Threads for host-side number crunching: the CPUs this process may run on, at most ESS_WORKERS_MAX."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(ESS_WORKERS_MAX, n))


def dump_outputs(path, arrays, limit=DUMP_LIMIT_BYTES, seed=0):
    """--dump-outputs: every array as path/<name>.npy, float32 kept, any other dtype as float64.  At most `limit` bytes in all: an
    array over its share keeps a fixed, seeded sample of its last axis, and the kept indices go beside it as <name>_index.npy."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    arrays = {k: (v if v.dtype == np.float32 else v.astype(np.float64)) for k, v in arrays.items()}
    left, written = int(limit), {}
    order = sorted(arrays, key=lambda k: arrays[k].nbytes)
    for i, name in enumerate(order):
        a = arrays[name]
        share = left // (len(order) - i)
        if a.nbytes > share and a.ndim >= 1 and a.shape[-1] > 1:
            col = a.nbytes // a.shape[-1]                       # bytes of one index of the last axis, + 8 for the index itself
            keep = max(1, min(a.shape[-1], share // (col + 8)))
            idx = np.sort(np.random.default_rng(seed).choice(a.shape[-1], size=keep, replace=False))
            a = np.ascontiguousarray(a[..., idx])
            np.save(os.path.join(path, f"{name}_index.npy"), idx.astype(np.float64))
            left -= idx.size * 8
        np.save(os.path.join(path, f"{name}.npy"), a)
        left -= a.nbytes
        written[name] = list(a.shape)
    return written


def cpu_baseline(data, threads, wl, chains=CHAINS_PER_GPU):
    """Oracle (port of the same algorithm, float64 C) on host cores: the same chains x (warmup + draws) as the GPU for the
    headline workload, a bounded sample for the heavier ones.  Built -O3 -march=native on THIS host (oracle/Makefile `native`)."""
    import numpy as np

    os.environ["OCCU_ORACLE_FLAVOR"] = "native"
    import oracle
    from biolith_amd.evaluation import effective_sample_size  # noqa: F401

    od = oracle.OracleData(data["site_covs"], data["obs_covs"], data["obs"], model=wl["model"], **wl.get("options", {}))
    w, s = wl["cpu_sample"]
    t0 = time.perf_counter()
    r = oracle.nuts_run(od, w, s, num_chains=chains, seed=0, threads=threads)
    wall = time.perf_counter() - t0
    X = np.asarray(data["site_covs"], dtype=np.float32).astype(np.float64)
    ess = ess_of_site_function(r["draws"], X, wl["site"], o_u=od.Ks + od.Ko + 3 if wl["model"] == "occu_re" else None)
    nleap = int(r["n_leapfrog"].sum())
    same = (w, s) == (wl["num_warmup"], wl["num_samples"])
    return dict(value=ess / wall, unit="ESS/s", cores=int(r["threads"]), kind="port",
                sample_short=f"oracle NUTS (f64 C), {chains} chains x ({w}+{s}){' = GPU workload' if same else ' bounded'}, {int(r['threads'])}/{os.cpu_count()} cores, "
                             f"{wall:.1f} s, ESS {ess:.0f}",
                sample=f"oracle NUTS (float64 C restatement, gcc -O3 -march=native -fno-fast-math, one thread per chain), same data, "
                       f"{chains} chains x ({w} warmup + {s} draws){' = the GPU workload' if same else ' (bounded sample)'} "
                       f"on {int(r['threads'])} of {os.cpu_count()} host cores: {wall:.1f} s, {nleap} gradient evaluations, "
                       f"{1e3 * wall * int(r['threads']) / nleap:.2f} ms per evaluation per core, ESS({wl['site']}) {ess:.0f}")


def cpu_baseline_scaled(aux, wl, threads, budget_s=12.0, chains=CHAINS_PER_GPU):
    """Bounded CPU leg of a secondary workload: the oracle's potential + gradient (the whole cost of a leapfrog) is timed at
    posterior draws of the GPU run for about `budget_s` seconds on `threads` cores, and scaled to the metric's unit with the run's
    own size: CPU seconds per step = gradient evaluations per chain x seconds per evaluation (chains side by side, one per core);
    ESS per step is the GPU run's (same algorithm, same target: the oracle's sampler is the kernel's restatement)."""
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np

    os.environ["OCCU_ORACLE_FLAVOR"] = "native"
    import oracle

    data = aux["data"]
    od = oracle.OracleData(data["site_covs"], data["obs_covs"], data["obs"], model=wl["model"], **wl.get("options", {}))
    th = np.asarray(aux["draws"], dtype=np.float64).reshape(-1, aux["D"])
    th = th[:: max(1, len(th) // 64)][:64]
    t0 = time.perf_counter()
    od.potential_grad(th[:1])
    one = max(time.perf_counter() - t0, 1e-4)
    per_thread = int(min(max(budget_s / one, 2), 2000))

    def work(k):
        idx = (np.arange(per_thread) + k * per_thread) % len(th)
        return od.potential_grad(th[idx])[0].sum()

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(work, range(threads)))
    wall = time.perf_counter() - t0
    s_eval = wall / per_thread                        # seconds per evaluation per core, all `threads` cores busy
    chains_rounds = -(-chains // threads)
    cpu_s_per_step = chains_rounds * (aux["leap_per_step"] / chains) * s_eval
    # NOT like for like with the GPU figure: ESS per step is borrowed from the GPU run, not measured; the oracle is the plain
    # float64 statement of the model (occu_rn: every term of every visit up to where the terms have died out under a double's rounding --
    # about a third of the max_abundance + 1, where the kernel keeps the eighth within 20 nats of the largest) on `threads` of the host's cores.  Reported as context; no gpu_over_cpu is derived from a scaled baseline.
    return dict(value=aux["ess_per_step"] / cpu_s_per_step, unit="ESS/s", cores=threads, kind="port", scaled=True, comparable=False,
                sample_short=f"SCALED: oracle potential+gradient {1e3 * s_eval:.2f} ms/eval/core x {aux['leap_per_step'] / chains:.0f} evals/chain, "
                             f"{threads}/{os.cpu_count()} cores, {wall:.1f} s; ESS as the GPU run's",
                sample=f"SCALED ESTIMATE, not a sampler run: oracle potential + gradient (float64 C restatement, gcc -O3 -march=native -fno-fast-math) at {per_thread} posterior "
                       f"draws per core on {threads} of {os.cpu_count()} host cores: {wall:.1f} s, {1e3 * s_eval:.2f} ms per evaluation per core; scaled: "
                       f"{aux['leap_per_step'] / chains:.0f} gradient evaluations per chain per step x that = {cpu_s_per_step:.1f} s per step "
                       f"({chains} chains side by side), ESS per step as the GPU run's ({aux['ess_per_step']:.0f}); validated against the oracle's "
                       f"own sampler run: profiles/r04/c_cpu_baseline_validation_rn.json, profiles/r05/e_cpu_baseline_rn.json")


def committed_cpu_baseline(relpath):
    """The cpu_baseline object of a committed bench record (a sampler run of the oracle too long for the default run), marked as such."""
    try:
        with open(os.path.join(ROOT, relpath)) as f:
            cb = dict(json.load(f)["cpu_baseline"])
    except (OSError, ValueError, KeyError):
        return None
    cb.update(scaled=False, measured_in=relpath, sample=f"NOT timed in this run ({relpath}): " + cb.get("sample", ""),
              sample_short=f"oracle NUTS (f64 C) 4 x (200+200), {cb.get('cores')} cores; NOT timed in this run: {relpath}")
    return cb


def fit_end_to_end(data, reps=3, chains=CHAINS_PER_GPU):
    """What biolith's own benchmark times (benchmarks/occu_spoccupancy.py:104-113): the clock around the whole
    ``fit(occu, **data, num_chains=4)`` -- host arrays in, upload, sampling, draws back -- plus the ``psi`` fetch that the
    metric needs (the reference's samples are device arrays until looked at; here psi is computed on first access)."""
    from biolith_amd.evaluation import effective_sample_size  # noqa: F401
    from biolith_amd.models import occu
    from biolith_amd.utils import fit

    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fit(occu, **data, num_chains=chains)
        t1 = time.perf_counter()
        psi = res.samples["psi"]
        t2 = time.perf_counter()
        rec = dict(fit_ms=1e3 * (t1 - t0), psi_fetch_ms=1e3 * (t2 - t1), total_ms=1e3 * (t2 - t0), kernel_ms=res.mcmc.result.kernel_ms,
                   draws=res.mcmc.result.draws)
        runs.append(rec)
        del psi, res
    return runs


PMC_CHILD_LAUNCHES = 2


def pmc_child(args):
    """What the live PMC passes profile: the workload's own launches (same geometry as the timed steps), nothing else.  No torch."""
    from biolith_amd.engine import OccuDataset
    from biolith_amd.models import simulate, simulate_dyn, simulate_rn

    wl = WORKLOADS[args.workload]
    with contextlib.redirect_stdout(io.StringIO()):
        data, _ = {"occu_rn": simulate_rn, "occu_dyn": simulate_dyn}.get(wl["model"], simulate)(**wl["cfg"])
    ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"], model=wl["model"], **wl.get("options", {}))
    for s in range(1 + PMC_CHILD_LAUNCHES):
        ds.launch(num_warmup=wl["num_warmup"], num_samples=wl["num_samples"], num_chains=workload_chains(wl, args.chains_per_gpu), seed=s,
                  wgs_per_chain=args.wgs_per_chain)
        ds.wait()


def live_hbm_traffic(name, kernel_substr, wgs_per_chain=0, timeout_s=240, chains_per_gpu=0):
    """HBM bytes per launch of the workload's sampler kernel measured in THIS run: one rocprofv3 --pmc pass per counter (FETCH_SIZE and
    WRITE_SIZE do not fit one pass; MI355X_MICROARCH.md) over a child process that only launches (`--pmc-child`), the counters summed
    over each dispatch's rows, the mean over its dispatches taken, FETCH_SIZE doubled (that guide's gfx950 correction) -- what
    tools/pmc_run.sh + tools/pmc_summary.py do for the committed profiles.  Returns (bytes or None, how it was obtained / why not)."""
    import csv
    import glob
    import shutil
    import tempfile
    from collections import defaultdict

    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not found"
    if any(k.startswith(("ROCPROF", "ROCP_", "ROCTX")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return None, "this process is itself running under a profiler"
    kb = {}
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(td, counter)
            cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "--", sys.executable,
                   os.path.abspath(__file__), "--pmc-child", "--workload", name, "--wgs-per-chain", str(wgs_per_chain),
                   "--chains-per-gpu", str(chains_per_gpu)]
            try:
                r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=timeout_s)
            except subprocess.TimeoutExpired:
                return None, f"rocprofv3 --pmc {counter} pass timed out"
            if r.returncode != 0:
                return None, f"rocprofv3 --pmc {counter} pass failed (rc {r.returncode}): {r.stderr.strip()[-200:]}"
            per_dispatch = defaultdict(float)
            for path in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                with open(path) as f:
                    for row in csv.DictReader(f):
                        if kernel_substr in row["Kernel_Name"] and row["Counter_Name"] == counter:
                            per_dispatch[row["Dispatch_Id"]] += float(row["Counter_Value"])
            if not per_dispatch:
                return None, f"no {counter} rows for {kernel_substr} in the pass's output"
            kb[counter] = sum(per_dispatch.values()) / len(per_dispatch)
    return (2.0 * kb["FETCH_SIZE"] + kb["WRITE_SIZE"]) * 1024.0, (
        "measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE, then WRITE_SIZE, over a child process making "
        f"{1 + PMC_CHILD_LAUNCHES} launches of this workload; per-launch mean (FETCH_SIZE {kb['FETCH_SIZE']:.1f} KB doubled per "
        f"MI355X_MICROARCH.md + WRITE_SIZE {kb['WRITE_SIZE']:.1f} KB)")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.pmc_child:
        return pmc_child(args)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args, argv)     # before torch / HIP are touched in this process
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import numpy as np

    selftest = os.environ.get("BENCH_SELFTEST") == "1"   # tests/: launcher + rendezvous on gloo, no GPU work, not a bench line
    import torch

    if not selftest:
        have = torch.cuda.device_count()     # (does not initialise HIP)
        if have < world or local_rank >= have:
            raise SystemExit(f"bench.py: --gpus {world} but only {have} GPU(s) visible on this node (rank {rank}); "
                             "refusing to run fewer ranks than asked")
    dist = None
    use_dist = world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1"  # the env knob exercises the RCCL path on one GPU
    if use_dist:
        import torch.distributed as dist

        # NCCL_DEBUG=VERSION (set on the GPU boxes) makes RCCL print a five-line banner on STDOUT when the first
        # communicator is created; stdout is reserved for the one JSON line, so that banner is turned off
        if os.environ.get("NCCL_DEBUG", "").upper() == "VERSION":
            del os.environ["NCCL_DEBUG"]
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        if selftest:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    elif not selftest:
        torch.cuda.set_device(local_rank)
    if selftest:
        t = torch.tensor([float(rank)], dtype=torch.float64)
        if dist is not None:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            dist.barrier()
        if rank == 0:
            print(json.dumps({"selftest": True, "n_gpus": world, "world": dist.get_world_size() if dist is not None else 1,
                              "rank_sum": float(t.item()), "launcher": os.environ.get("BENCH_LAUNCHED_BY", "external")}))
        if dist is not None:
            dist.destroy_process_group()
        return

    from biolith_amd.distributed import comm_from_env, gather_draws, rccl_version
    from biolith_amd.engine import OccuDataset
    from biolith_amd.evaluation import effective_sample_size, split_gelman_rubin
    from biolith_amd.models import simulate, simulate_dyn, simulate_rn

    stream = torch.cuda.current_stream().cuda_stream
    # the data-path communicator: the engine's own (librccl behind the C-ABI); made before the timed region, cost reported
    comm, gather_fallback = None, None
    if use_dist:
        try:
            if os.environ.get("BENCH_FORCE_GATHER_FALLBACK") == "1":   # (exercises the fallback below on a one-GPU box)
                raise RuntimeError("BENCH_FORCE_GATHER_FALLBACK=1")
            comm = comm_from_env(local_rank, rank, world)
        except Exception as exc:  # noqa: BLE001 -- the scaling line must not be lost to the engine's own communicator
            gather_fallback = f"bl_comm_init_rank failed on rank {rank}: {type(exc).__name__}: {exc}"
    GATHERED = ("draws", "diverging", "num_steps", "accept_prob", "potential_energy", "step_size", "inv_mass", "n_leapfrog")

    def agree_on_gather():
        """Every rank takes the same gather: the engine's (bl_gather_draws on librccl) unless ANY rank failed with it, then
        torch.distributed's all-gather (backend nccl = the same RCCL) for the rest of the run -- said so in the line."""
        nonlocal comm, gather_fallback
        if dist is None:
            return
        bad = torch.tensor([0.0 if gather_fallback is None else 1.0], dtype=torch.float64, device=f"cuda:{local_rank}")
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        if bad.item() != 0.0:
            reasons = [None] * world
            dist.all_gather_object(reasons, gather_fallback)
            gather_fallback = "; ".join(r for r in reasons if r) or "a peer failed"
            if comm is not None:
                if gather_hung[0]:
                    comm._h = None   # a collective is still pending on it: neither waited for nor destroyed (bl_comm_destroy would wait)
                else:
                    with contextlib.suppress(Exception):
                        comm.close()
                comm = None

    def torch_gather(res):
        """The fallback gather: every per-chain array of the local result through torch.distributed (RCCL), rank order."""
        import copy

        from biolith_amd.distributed import gather_host_arrays

        full = copy.copy(res)
        for nm in GATHERED:
            a = np.ascontiguousarray(getattr(res, nm))
            t = torch.from_numpy(a.astype(np.uint8) if a.dtype == np.bool_ else a).to(f"cuda:{local_rank}")
            g = gather_host_arrays(t).cpu().numpy()
            setattr(full, nm, g.astype(np.bool_) if a.dtype == np.bool_ else g)
        return full

    agree_on_gather()

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    in_warmup, nonlocal_fail = [False], [None]
    first_gather, gather_hung, kept_alive = [True], [False], []

    def bench_workload(name, n_steps, n_warmup):
        """W untimed + exactly K timed steps of one workload; rank 0 gets the line (a dict), the others None."""
        nonlocal comm
        wl = WORKLOADS[name]
        NUM_WARMUP, NUM_SAMPLES = wl["num_warmup"], wl["num_samples"]
        NCH = workload_chains(wl, args.chains_per_gpu)   # chains per GPU of this workload
        chains_per_rank = [NCH] * world
        shard = rank_shard(rank, NCH)
        with contextlib.redirect_stdout(io.StringIO()):
            data, truth = {"occu_rn": simulate_rn, "occu_dyn": simulate_dyn}.get(wl["model"], simulate)(**wl["cfg"])
        X = np.asarray(data["site_covs"], dtype=np.float32).astype(np.float64)
        ds = OccuDataset(data["site_covs"], data["obs_covs"], data["obs"], device=local_rank,
                         model=wl["model"], **wl.get("options", {}))  # resident in HBM from here on

        def one_step(step_seed):
            ds.launch(num_warmup=NUM_WARMUP, num_samples=NUM_SAMPLES, seed=step_seed, wgs_per_chain=args.wgs_per_chain, stream=stream, **shard)
            ds.wait()
            if comm is None:
                res = ds.fetch()
                if gather_fallback is not None:   # (the engine's communicator failed somewhere: agree_on_gather)
                    full = torch_gather(res)
                    return res, (full.draws if rank == 0 else None)
                return res, res.draws
            # bl_gather_draws: ONE all-gather of every rank's result block over RCCL / xGMI, the path's only collective;
            # only rank 0 copies the gathered blocks to the host
            try:
                if in_warmup[0] and first_gather[0] and (world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1"):
                    # The run's FIRST gather over several ranks (untimed): bounded.  It runs in a worker thread; if it has not returned
                    # after BENCH_FIRST_GATHER_TIMEOUT seconds (a peer failed inside the collective, a rendezvous that never completes)
                    # this rank gives the engine's communicator up -- the thread and the communicator are left behind, not waited for --
                    # and the ranks agree (agree_on_gather) to gather through torch.distributed for the rest of the run.
                    import threading

                    first_gather[0] = False
                    box = {}

                    def work():
                        try:
                            if os.environ.get("BENCH_TEST_FIRST_GATHER_HANG") == "1":   # (exercises the bound on a one-GPU box)
                                time.sleep(3600)
                            box["full"] = gather_draws([comm], [ds], chains_per_rank, want_result=(rank == 0))
                        except Exception as exc_:  # noqa: BLE001
                            box["exc"] = exc_

                    th = threading.Thread(target=work, daemon=True)
                    th.start()
                    th.join(float(os.environ.get("BENCH_FIRST_GATHER_TIMEOUT", "180")))
                    if th.is_alive():
                        gather_hung[0] = True
                        raise TimeoutError("the first bl_gather_draws did not return within its bound")
                    if "exc" in box:
                        raise box["exc"]
                    full = box["full"]
                else:
                    full = gather_draws([comm], [ds], chains_per_rank, want_result=(rank == 0))
            except Exception as exc:  # noqa: BLE001 -- only recoverable during the untimed steps (see below); else it ends the run
                if not in_warmup[0]:
                    raise
                nonlocal_fail[0] = f"bl_gather_draws failed on rank {rank}: {type(exc).__name__}: {exc}"
                res = ds.fetch()
                return res, None
            local = ds.fetch() if rank != 0 else None
            if rank == 0:
                lo = shard["chain_offset"]
                import copy

                local = copy.copy(full)
                for nm in ("draws", "diverging", "num_steps", "accept_prob", "potential_energy", "step_size", "inv_mass", "n_leapfrog"):
                    setattr(local, nm, getattr(full, nm)[lo: lo + NCH])
            return local, (full.draws if full is not None else None)

        for w in range(n_warmup):
            # (--warmup 0 has no untimed gather: neither the bound on the first gather nor the fallback to torch.distributed applies then)
            in_warmup[0] = True
            one_step(10_000 + w)
            in_warmup[0] = False
            if comm is not None and (world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1") and w == 0:   # the first gather of the run, untimed: did it work on every rank?
                nonlocal gather_fallback
                gather_fallback = nonlocal_fail[0]
                agree_on_gather()
        sync_all()
        t0 = time.perf_counter()
        steps = [one_step(s) for s in range(n_steps)]
        sync_all()
        elapsed = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([elapsed], dtype=torch.float64, device=f"cuda:{local_rank}")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())

        # ---- per-rank kernel statistics (HIP events on the launch stream, recorded inside the timed region)
        kernel_ms = np.array([r.kernel_ms for r, _ in steps])
        leap = np.array([int(r.n_leapfrog.sum()) + NCH for r, _ in steps])  # + the initial evaluation of each chain
        kernel_ms_per_rank = [float(kernel_ms.mean())]
        if dist is not None:
            agg = torch.tensor([kernel_ms.mean(), leap.mean()], dtype=torch.float64, device=f"cuda:{local_rank}")
            every = [torch.zeros_like(agg) for _ in range(world)]
            dist.all_gather(every, agg)
            kernel_ms_per_rank = [float(e[0].item()) for e in every]
            kernel_ms_mean = float(np.mean(kernel_ms_per_rank))
            leap_mean = float(np.mean([float(e[1].item()) for e in every]))
        else:
            kernel_ms_mean, leap_mean = float(kernel_ms.mean()), float(leap.mean())
        if rank != 0:
            return None, None, None

        # ---- metric numerator: ESS(psi), NumPyro estimator, mean over sites (diagnostics.py:28-32) ----
        # (at most ESS_STEPS_MAX steps evaluated, evenly spread; with more timed steps their mean stands for every step)
        ess_at = sorted({int(round(x)) for x in np.linspace(0, n_steps - 1, min(n_steps, ESS_STEPS_MAX))})
        ess_psi, ess_coef, rhat = [], [], []
        for i, (_, d) in enumerate(steps):
            G0 = ds.Ks + ds.Ko + 2
            fixed = d[..., :G0] if wl["model"] == "occu_re" else d   # (with random effects: min ESS / R-hat over the fixed effects)
            if i in ess_at:
                ess_psi.append(ess_of_site_function(d.astype(np.float64), X, wl["site"], o_u=G0 + 1 if wl["model"] == "occu_re" else None,
                                                    workers=host_workers()))
            ess_coef.append(effective_sample_size(fixed).min())
            rhat.append(float(split_gelman_rubin(fixed).max()))
        total_ess = float(np.sum(ess_psi)) if len(ess_psi) == n_steps else float(np.mean(ess_psi)) * n_steps
        N, T, J, Ks, Ko = ds.N, ds.T, ds.J, ds.Ks, ds.Ko
        bytes_eval = algorithmic_bytes_per_eval(N, T, J, Ks, Ko)
        if wl["model"] == "occu_re":   # + the sampler's own vectors: about 14 of them are read or written per leapfrog
            bytes_eval += 56 * ds.D
        res0 = steps[0][0]
        achieved = leap_mean * bytes_eval / (kernel_ms_mean * 1e-3) / 1e9
        # roofline.traffic: HBM bytes per launch from the PMC passes (tools/pmc_run.sh, separate --pmc runs of this same
        # command); a STATIC figure read from a committed file, not measured in this run
        traffic, traffic_source = None, None
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tpath):
            with open(tpath) as f:
                tj = json.load(f)
            ent = tj.get(name) or (tj if name == "occu" and "hbm_bytes_per_launch" in tj else None)
            if ent:
                traffic = ent.get("hbm_bytes_per_launch")
                traffic_source = f"profiles/pmc_traffic.json (static; from {ent.get('source')})"
        if world == 1 and args.full and not args.no_live_pmc:
            # measured NOW (two --pmc passes over a child process, after this workload's timed region; a few seconds each); the
            # committed figure stays as the fallback and is quoted beside it
            try:
                live, how = live_hbm_traffic(name, "bl_re_nuts_kernel" if wl["model"] == "occu_re" else "bl_nuts_kernel", args.wgs_per_chain,
                                                 chains_per_gpu=args.chains_per_gpu)
            except Exception as e:  # noqa: BLE001 -- a profiler hiccup must not cost the line
                live, how = None, f"live PMC passes failed: {e!r}"
            if live is not None:
                traffic_static, traffic, traffic_source = traffic, live, how
            else:
                traffic_static = None
                traffic_source = f"{traffic_source}; live passes: {how}"
        else:
            traffic_static = None
        # the instantiation that ran, as the engine reports it (bl_nuts_kernel_name) and rocprofv3 prints it:
        # bl_nuts_kernel<KS, KO, LDS-staged, model, compute waves, lane-group form, visits-per-period form, lean form>,
        # bl_re_nuts_kernel<covariate capacity, model kind, rows in LDS, sampler-vector tier in LDS, effects as compile-time facts>
        kernel_name = res0.kernel_name
        # (the launch ends with its slowest chain: this rank's kernel time over THAT chain's gradient evaluations is the kernel's own
        # per-leapfrog time; the figure over the mean below also moves with how evenly the chains adapted)
        us_leap_slowest = float(np.mean([r.kernel_ms * 1e3 / (int(r.n_leapfrog.reshape(NCH, -1).sum(axis=1).max()) + 1) for r, _ in steps]))
        us_leap = 1e3 * kernel_ms_mean / (leap_mean / NCH)
        roofline = {
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic, "traffic_source": traffic_source, **({"traffic_committed": traffic_static} if traffic_static is not None else {}),
            "kernel": kernel_name, "kernel_ms": kernel_ms_mean,
            "algorithmic_bytes_per_launch": leap_mean * bytes_eval, "bytes_per_gradient_evaluation": bytes_eval,
            "gradient_evaluations_per_launch": leap_mean,
            "us_per_leapfrog_per_chain": us_leap, "us_per_leapfrog_slowest_chain": us_leap_slowest,
            "note": "data is LDS-resident after one HBM read, so this is an effective (algorithmic) bandwidth; "
                    "the sequential-leapfrog latency (us_per_leapfrog_per_chain) is the real bound",
        }
        if name == "occu":
            # The tick's floor as numbers, re-derived in round 5 from a variant that took NumPyro's decisions off the
            # critical path altogether (a gather wave + a decision wave: profiles/r05/b_split_control_waves.patch, b_stamps_split_v*.txt --
            # bit-identical, 2.48 us): a tick cannot be shorter than the site evaluation (1 605 cycles) + evaluation-complete-to-gathered
            # (~1 800: store to L2, round alignment, one L2 round trip, skew of the chain's 81 compute waves, f64 sums and folds) +
            # the next position (210) + the release barrier (~170) = ~3 780 cycles at 2.39 GHz, times 1.137 ticks per leapfrog (one
            # evaluation is dropped per transition).  The kernel of record is 10 % above it: the part of the decisions at doubling and
            # transition-end ticks that outlasts the evaluation.
            roofline["latency_floor_us"] = 1.8
            roofline["latency_floor_note"] = ("per leapfrog, every decision hidden: site evaluation 1 605 cycles + evaluation-complete-to-gathered ~1 800 (store to L2 "
                                              "~300, round alignment ~330, one L2 round trip 650-730, skew of 81 compute waves, f64 sums and folds ~200) + next "
                                              "position 210 + release barrier ~170 = ~3 780 cycles per tick at 2.39 GHz x 1.137 ticks per leapfrog; measured on a "
                                              "variant with the decisions on a wave of their own (profiles/r05/b_stamps_split_v1.txt, b_ab_split.txt: bit-identical "
                                              "draws, 2.48 us -- dropped); stamps of the kernel of record: profiles/r05/h_stamps.txt (tick 4 201 cycles)")
        if wl["model"] == "occu_rn":
            # config 4 is VALU-transcendental-bound (about 5 M enumerated (site, visit, n) terms per evaluation,
            # one transcendental each), not HBM-bound.  Peak = quarter-rate transcendental issue of the CUs the launch occupies.
            terms = N * T * J * 101
            cus = NCH * res0.wgs_per_chain
            ach = leap_mean * terms / (kernel_ms_mean * 1e-3) / 1e9
            try:
                d_last = steps[-1][1]
                executed, n_items = rn_executed_terms(data, d_last.reshape(-1, d_last.shape[-1]).mean(axis=0).astype(np.float64), Ks)
            except Exception:  # noqa: BLE001 -- a diagnostic; never costs the line
                executed, n_items = None, None
            roofline = {
                "bound": "valu-transcendental", "achieved": ach, "peak": cus * TRANS_PER_CU_PER_S / 1e9, "unit": "Gtrans/s",
                "frac": ach / (cus * TRANS_PER_CU_PER_S / 1e9), "frac_of_chip": ach / (N_CUS * TRANS_PER_CU_PER_S / 1e9),
                "cus_used": cus, "transcendentals_per_gradient_evaluation": terms,
                # what the kernel EXECUTES of them (items of 8 consecutive n x all J visits, the sites' n-ranges cut where their terms
                # have died out; counted in NumPy at the run's posterior mean) -- `achieved` and `frac` price the ALGORITHMIC terms
                "executed_terms_per_evaluation": executed, "items_per_evaluation": n_items,
                "frac_executed": (executed / terms) if executed else None,
                "achieved_executed": (ach * executed / terms) if executed else None,
                "traffic": traffic, "traffic_source": traffic_source, "kernel": kernel_name, "kernel_ms": kernel_ms_mean,
                "gradient_evaluations_per_launch": leap_mean, "us_per_leapfrog_per_chain": us_leap, "us_per_leapfrog_slowest_chain": us_leap_slowest,
                "hbm_effective_GBps": achieved, "bytes_per_gradient_evaluation": bytes_eval,
                "note": "algorithmic transcendentals = N x T x J x (max_abundance + 1) enumerated terms (SURVEY.md section 8d); the kernel "
                        "cuts every site's n-range where its terms die out (items of 8 terms, rn_device.hpp): executed_terms_per_evaluation, "
                        "frac_executed; peak = 8 lanes x 4 SIMDs x 2.4 GHz per CU (8 issue cycles per wave64 transcendental, MI355X_MICROARCH.md:489)",
            }
        out = {
            "metric": wl["metric"],
            "value": total_ess / elapsed,
            "unit": "ESS/s",
            "n_gpus": world,
            "steps": n_steps,
            "warmup": n_warmup,
            "ms_per_step": 1e3 * elapsed / n_steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "rccl_world": comm.world if comm is not None else 1,
            # true: the engine's first (untimed) bl_gather_draws did not return within its bound on this rank; the run went on with
            # torch.distributed's all-gather (config.gather says so).  That path has only been exercised with a simulated hang on one GPU.
            "gather_hung": bool(gather_hung[0]),
            "kernel_ms_per_rank": kernel_ms_per_rank,
            "config": {
                "workload": f"{wl['text']}: NUTS {NCH} chain{'s' if NCH != 1 else ''} per GPU x ({NUM_WARMUP} warmup + {NUM_SAMPLES} draws), "
                            "one step = one full fit",
                "chains_per_gpu": NCH, "total_chains": NCH * world,
                "num_warmup": NUM_WARMUP, "num_samples": NUM_SAMPLES, "parallelism": f"chains x{world} (1 process per GPU)",
                "wgs_per_chain": res0.wgs_per_chain, "lds_bytes_per_wg": res0.lds_bytes, "lds_staged": res0.lds_staged,
                "env_overrides": res0.env_overrides,   # BIOLITH_HIP_* knobs set at the launch ("" = none)
                "lanes_per_site_pair": {"period_lanes": res0.lane_group[0], "visit_lanes": res0.lane_group[1]},
                "gather": (f"bl_gather_draws: one ncclAllGather of {world} result blocks (RCCL {rccl_version()}), communicator init "
                           f"{comm.init_ms:.0f} ms outside the timed region") if comm is not None else
                          ("none (one rank)" if gather_fallback is None else
                           f"FALLBACK torch.distributed all_gather (backend nccl = RCCL) of the per-chain arrays -- the engine's own gather was "
                           f"given up: {gather_fallback}"),
                "torch_process_group": (dist.get_backend() + f" x{dist.get_world_size()} (barrier / max-over-ranks only)") if dist is not None else None,
            },
            "roofline": roofline,
            "sampler": {  # rank 0's chains, last timed step (SURVEY.md section 8d "also report")
                "mean_num_steps": float(steps[-1][0].num_steps.mean()), "divergences": int(steps[-1][0].diverging.sum()),
                "mean_tree_depth": float(np.log2(steps[-1][0].num_steps.astype(np.float64) + 1.0).mean()),
                "step_size": [float(x) for x in steps[-1][0].step_size], "mean_accept_prob": float(steps[-1][0].accept_prob.mean()),
                "leapfrogs_per_s_per_chain": 1e3 * (leap_mean / NCH) / kernel_ms_mean,
            },
            "ess": {f"{wl['site']}_mean_over_sites_per_step": ess_psi, "steps_evaluated": ess_at, "min_coef_per_step": [float(x) for x in ess_coef],
                    "max_split_rhat": max(rhat), "draws_per_step": NCH * world * NUM_SAMPLES},
        }
        # what the scaled CPU baseline of a secondary workload needs: posterior draws to evaluate at, and the launch's size
        aux = dict(data=data, X=X, draws=steps[-1][1], leap_per_step=leap_mean, ess_per_step=total_ess / n_steps, D=ds.D, chains=NCH,
                   last=steps[-1][0])
        if gather_hung[0]:
            kept_alive.append(ds)   # the abandoned worker thread still refers to it (its events must outlive the thread): kept until exit
        del ds
        return out, aux, wl

    out, aux, wl = bench_workload(args.workload, args.steps, args.warmup)
    if rank == 0 and args.dump_outputs:
        # what the timed path handed its caller in the last timed step (rank 0's chains; with several ranks also the gathered draws)
        last = aux["last"]
        arrays = {nm: getattr(last, nm) for nm in GATHERED}
        if world > 1 and aux["draws"] is not None:
            arrays["draws_all_ranks"] = aux["draws"]
        dump_outputs(args.dump_outputs, arrays)
    if rank == 0:
        # Everything below runs AFTER the measured line exists: a failure in a late leg is recorded in the line, never loses it.
        if world == 1 and args.full and args.workload == "occu" and not args.no_e2e:
            try:
                # SURVEY section 8d's second clock: end-to-end fit() from host arrays, PCIe and the psi fetch included (never `value`)
                runs = fit_end_to_end(aux["data"], chains=aux["chains"])
                e2e = min(runs, key=lambda r: r["total_ms"])
                ess_e2e = ess_of_site_function(e2e["draws"].astype(np.float64), aux["X"], "psi")
                out["fit_e2e_ms"] = e2e["total_ms"]
                out["value_e2e"] = ess_e2e / (e2e["total_ms"] * 1e-3)
                out["fit_e2e"] = {"fit_call_ms": e2e["fit_ms"], "psi_fetch_ms": e2e["psi_fetch_ms"], "kernel_ms": e2e["kernel_ms"],
                                  "ess_psi": ess_e2e, "total_ms_each": [r["total_ms"] for r in runs],
                                  "total_ms_median": float(np.median([r["total_ms"] for r in runs])),
                                  "what": "best of 3 (all three and their median beside it; the first call pins its output buffers, later ones "
                                          f"reuse them): clock around fit(occu, **data, num_chains={aux['chains']}) from host NumPy arrays (upload, sampling, "
                                          f"draws back) + samples['psi'] ({aux['chains'] * 1000} x 10000 float32 computed on the device and copied over PCIe), "
                                          "as biolith/benchmarks/occu_spoccupancy.py:104-113 times it; library already loaded"}
            except Exception as exc:  # noqa: BLE001
                out["fit_e2e_error"] = f"{type(exc).__name__}: {exc}"
        if world == 1 and args.full and not args.no_cpu_baseline:
            try:
                threads = min(aux["chains"], os.cpu_count() or 1)
                if args.workload in ("occu", "occu_cfg1") or args.cpu_baseline:   # the oracle's own sampler run (the headline: the same chains x draws as the GPU)
                    out["cpu_baseline"] = cpu_baseline(aux["data"], threads=threads, wl=wl, chains=aux["chains"])
                    out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
                    if args.cpu_baseline and args.workload not in ("occu", "occu_cfg1"):   # ... and the scaled estimate beside it: validates the scaling once
                        out["cpu_baseline_scaled"] = cpu_baseline_scaled(aux, wl, threads=threads, chains=aux["chains"])
                        out["cpu_baseline_scaled"]["sampler_run_over_scaled"] = out["cpu_baseline"]["value"] / out["cpu_baseline_scaled"]["value"]
                else:                                              # the other workloads: a bounded sample of oracle evaluations, scaled (no ratio derived)
                    out["cpu_baseline"] = cpu_baseline_scaled(aux, wl, threads=threads, chains=aux["chains"])
                    if args.workload == "occu_rn":
                        measured = committed_cpu_baseline(RN_CPU_MEASURED)
                        if measured is not None:
                            out["cpu_baseline_scaled"], out["cpu_baseline"] = out["cpu_baseline"], measured
            except Exception as exc:  # noqa: BLE001
                out["cpu_baseline_error"] = f"{type(exc).__name__}: {exc}"
    aux = None
    if world == 1 and args.full and args.workload == "occu" and not args.no_secondary and rank == 0:
        # ---- the other workloads of SURVEY section 8 in the same driver-run line (only the headline was driver-measured) ----
        out["secondary"] = []
        for name, k_steps, k_warm in SECONDARY:
            try:
                o2, a2, w2 = bench_workload(name, k_steps, k_warm)
                entry = {"workload": name, "metric": o2["metric"], "value": o2["value"], "unit": o2["unit"], "steps": k_steps, "warmup": k_warm,
                         "ms_per_step": o2["ms_per_step"], "us_per_leapfrog_per_chain": o2["roofline"]["us_per_leapfrog_per_chain"],
                         "dtype": "f32", "config": o2["config"], "roofline": o2["roofline"], "sampler": o2["sampler"], "ess": o2["ess"]}
                if name == "occu_dyn":
                    entry["reference_counterpart"] = "none: builder-defined model (models/occu_dyn.py); parity against the builder's own oracle only"
                if name == "occu_stacked":
                    entry["reference_counterpart"] = "none for BASELINE.json configs[4] as worded (dynamic colonisation / extinction); this is the stacked-period form of occu.py:198-210 at its size"
                if not args.no_cpu_baseline:
                    try:
                        thr = min(a2["chains"], os.cpu_count() or 1)
                        if name == "occu_cfg1":   # small enough for the oracle's own sampler: the same 2 chains x (1000 + 1000), a measured baseline
                            entry["cpu_baseline"] = cpu_baseline(a2["data"], threads=thr, wl=w2, chains=a2["chains"])
                            entry["gpu_over_cpu"] = entry["value"] / entry["cpu_baseline"]["value"]
                        else:                     # a scaled estimate (flagged "comparable": false): no speed-up is derived from it
                            entry["cpu_baseline"] = cpu_baseline_scaled(a2, w2, threads=thr, chains=a2["chains"])
                            if name == "occu_rn":     # BASELINE.json configs[3]: the MEASURED figure leads, the live scaled estimate stays beside it
                                measured = committed_cpu_baseline(RN_CPU_MEASURED)
                                if measured is not None:
                                    entry["cpu_baseline_scaled"], entry["cpu_baseline"] = entry["cpu_baseline"], measured
                    except Exception as exc:  # noqa: BLE001
                        entry["cpu_baseline_error"] = f"{type(exc).__name__}: {exc}"
                out["secondary"].append(entry)
            except Exception as exc:  # noqa: BLE001
                out["secondary"].append({"workload": name, "error": f"{type(exc).__name__}: {exc}"})
    if rank == 0:
        if "secondary" in out:
            # LAST key of the line, short: a record that keeps only the tail of stdout still holds every workload's figures
            # [value ESS/s, ms_per_step, us_per_leapfrog_per_chain, roofline.frac, cpu_baseline.value]
            out["secondary_summary"] = {
                e["workload"]: ([round(e["value"], 1), round(e["ms_per_step"], 2), round(e["us_per_leapfrog_per_chain"], 3),
                                 round(e["roofline"]["frac"], 4),
                                 (round(e["cpu_baseline"]["value"], 2) if "cpu_baseline" in e else None)]
                                if "error" not in e else "error") for e in out["secondary"]}
        full_path = args.full_out or os.path.join(ROOT, "gpurun_out", "bench_full.json" if args.workload == "occu" else f"bench_full_{args.workload}.json")
        wrote = write_full_record(out, full_path) if args.full or args.full_out else None   # (a plain run writes no record)
        sys.stdout.flush()
        print(json.dumps(out) if args.full_line else compact_line(out, wrote), flush=True)
    if comm is not None:
        comm.close()
    if dist is not None:
        dist.barrier()
        if gather_hung[0]:   # a pending collective of the abandoned communicator would block the runtime's teardown
            sys.stdout.flush()
            os._exit(0)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
