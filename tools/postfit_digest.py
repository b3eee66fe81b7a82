#!/usr/bin/env python3
"""One SHA-256 per (case, entry, output) of every post-fit entry, for each library named on the command line (each in its own process):
   python tools/postfit_digest.py path/to/libbiolith_hip_a.so path/to/libbiolith_hip_b.so
With one library it prints that library's listing; with several, every line carries the first library's digest | the other's and "equal"
or "DIFFERENT", the last line counts them, and the exit status is 1 if any differs (profiles/predict_math/digests.txt is that output).
Fixed inputs from numpy.random.default_rng, hand-made float32 draws uniform in (-1, 1) (occu_comb's six trailing coordinates set as
tools/time_latent.py sets them), seed 3.  Every entry is tried on every handle, once with all its outputs and once with its first alone
(a NULL output must not move another one); where an entry does not serve a handle the line holds the refusal's own text (any ValueError
or NotImplementedError of the call is listed so: read the text).  bl_predictive_density is also called for its point outputs alone (no
per-draw sums: the points' launch is then the entry's only one).  The cases: a single site, one site past a 256-thread block, 2 periods
x 3 visits, more draws than the 1024 grid rows, covariate counts below the kernels' capacity, every kind of handle, bl_deterministic
across its 8192-draw chunk boundary, and two short fits (the samplers compile next to the code that moved)."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, U8, I32, F64 = "float32", "uint8", "int32", "float64"


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def data(N, T, J, Ks, Ko, species=1):
    import numpy as np
    r = np.random.default_rng(N * 1000 + T * 100 + J * 10 + Ks)
    X, W = r.normal(size=(N, Ks)).astype(np.float32), r.normal(size=(N, T, J, Ko)).astype(np.float32)
    Y = (r.uniform(size=(species, N, T, J)) < 0.4).astype(np.float32)
    Cn = r.poisson(2.0, size=(1, N, T, J)).astype(np.float32)
    miss = r.uniform(size=(N, T, J)) < 0.15
    miss[0, 0, 0] = False
    Y[:, miss], Cn[:, miss] = np.nan, np.nan
    W[r.uniform(size=W.shape) < 0.05] = np.nan
    return dict(X=X, W=W, Y=Y, C=Cn, dur=r.uniform(0.5, 2.0, size=(N, T, J)).astype(np.float32),
                scores=np.where(np.isnan(Y), np.nan, r.normal(size=Y.shape)).astype(np.float32),
                Wa=r.normal(size=(N, T, 2, 1)).astype(np.float32), Ya=(r.uniform(size=(1, N, T, 2)) < 0.4).astype(np.float32),
                Sc=r.normal(size=(1, N, T, 3)).astype(np.float32))


def handles(d):
    from biolith_amd.engine import OccuDataset
    both = dict(site_random_effects=True, obs_random_effects=True)
    mk = lambda model, obs="Y", **o: (lambda: OccuDataset(d["X"], d["W"], d[obs], model=model, **o))
    cop = lambda **o: mk("occu_cop", "C", session_duration=d["dur"], **o)
    return [("occu", mk("occu")), ("occu_fp constant", mk("occu_fp", fp_mode="constant")), ("occu_fp unoccupied", mk("occu_fp", fp_mode="unoccupied")),
            ("occu_re", mk("occu_re", **both)), ("occu_re fp", mk("occu_re", re_fp_mode="unoccupied", **both)),
            ("occu_rn", mk("occu_rn", max_abundance=20)), ("occu_rn fp", mk("occu_rn", max_abundance=20, re_fp_mode="constant")),
            ("occu_rn re", mk("occu_rn", max_abundance=20, **both)),
            ("nmixture", mk("nmixture", "C", max_abundance=20)), ("nmixture re", mk("nmixture", "C", max_abundance=20, **both)),
            ("occu_cop", cop(fp_mode=None)), ("occu_cop constant", cop(fp_mode="constant")), ("occu_cop unoccupied", cop(fp_mode="unoccupied")),
            ("occu_cop re", cop(fp_mode=None, **both)), ("occu_cop re fp", cop(fp_mode="constant", **both)),
            ("occu_cs", mk("occu_cs", "scores")),
            ("occu_comb", lambda: OccuDataset(d["X"], d["W"], d["Y"], model="occu_comb", ARU_obs_covs=d["Wa"], ARU_obs=d["Ya"], scores_obs=d["Sc"])),
            ("occu_dyn", mk("occu_dyn"))]


def entries(ds, obs):
    """name -> (call(wanted flags) -> arrays, output names)"""
    import ctypes as C
    L, cell, vis = ds._lib, (ds.T, ds.N), (ds.J, ds.T, ds.N)
    ja, js = (getattr(ds, "Ja", 0),) + cell, (getattr(ds, "Js", 0),) + cell
    counts = ds.model in ("occu_cop", "nmixture")
    per_draw = lambda fn, *outs: (lambda th, want: ds._per_draw(fn, th, 3, [(w, s, t) for w, (_, s, t) in zip(want, outs)], pinned=False),
                                  [o[0] for o in outs])
    no_seed = lambda fn: (lambda h, n, dr, seed, *o: fn(h, n, dr, *o))
    density = lambda marginal: (lambda th, want: ds.predictive_density(th, obs, seed=3, marginal=marginal, per_draw=want[0], point_lse=want[1],
                                                                       point_var=want[2]), ["per_draw", "point_lse", "point_var"])
    return {
        "predict": per_draw(L.bl_predict, ("latent", cell, U8), ("y", vis, U8)),
        "predict_counts": per_draw(L.bl_predict_counts, ("latent", cell, I32), ("y", vis, I32)),
        "predict_scores": per_draw(L.bl_predict_scores, ("z", cell, U8), ("f", vis, U8), ("s", vis, F32)),
        "deterministic": per_draw(no_seed(L.bl_deterministic), ("psi", cell, F32), ("prob_detection", vis, F32)),
        "predict_comb": per_draw(L.bl_predict_comb, ("z", cell, U8), ("y_pc", vis, U8), ("y_aru", ja, U8), ("scores", js, F32)),
        "deterministic_comb": per_draw(no_seed(L.bl_deterministic_comb), ("psi", cell, F32), ("pc_prob", vis, F32), ("aru_prob", ja, F32)),
        "predictive_check": (lambda th, want: ds.predictive_check(th, obs, seed=3, by_site=want[0], by_revisit=want[1]), ["by_site", "by_revisit"]),
        "predictive_density": density(False), "predictive_density marginal": density(True),
        "site_posterior": per_draw(L.bl_site_posterior, ("log_lik", cell, F32), ("z_prob", cell, F32), ("z", cell, U8)),
        "abundance_posterior": per_draw(L.bl_abundance_posterior, ("log_lik", cell, F32), ("n_mean", cell, F32), ("occ_prob", cell, F32),
                                        ("n_draw", cell, I32)),
        "path_posterior": per_draw(L.bl_path_posterior, ("log_lik", (ds.N,), F32), ("z_prob", cell, F32), ("col_prob", (ds.T - 1, ds.N), F32),
                                   ("ext_prob", (ds.T - 1, ds.N), F32), ("z", cell, U8)),
        "score_posterior": per_draw(L.bl_score_posterior, ("log_lik", cell, F32), ("z_prob", cell, F32), ("z", cell, U8), ("f_prob", vis, F32),
                                    ("f", vis, U8)),
        "count_posterior": per_draw(L.bl_count_posterior, ("log_lik", cell, F32), ("z_prob", cell, F32), ("z", cell, U8), ("true_mean", vis, F32),
                                    ("true_count", vis, I32)),
    }


def draws_for(ds, n):
    import numpy as np
    r = np.random.default_rng(0)
    th = r.uniform(-1, 1, size=(n, ds.D)).astype(np.float32)
    if ds.model == "occu_comb":
        th[:, -6:] = (np.array([-1.2, -1.5, -2.0, 1.6, 1.5, 1.1]) + r.uniform(-0.4, 0.4, size=(n, 6))).astype(np.float32)
    return th


def run_case(case, name, make, d, n, only=None):
    ds = make()
    th, obs = draws_for(ds, n), d["Y"][0]
    for entry, (call, outs) in entries(ds, obs).items():
        if only and entry not in only:
            continue
        variants = [("all", [True] * len(outs)), ("first", [True] + [False] * (len(outs) - 1))]
        if entry.startswith("predictive_density"):
            variants.append(("rest", [False] + [True] * (len(outs) - 1)))
        for label, want in variants:
            try:
                arrays = call(th, want)
            except (NotImplementedError, ValueError) as e:
                if label == "all":
                    print(f"{case:10s} {name:20s} {entry:28s} refused: {type(e).__name__}: {e}")
                break
            for o, a in zip(outs, arrays):
                if a is not None:
                    print(f"{case:10s} {name:20s} {entry:28s} {label:5s} {o:14s} {a.dtype.name:7s} {a.shape!s:18s} {sha(a)}")
    sys.stdout.flush()
    ds.close()


def child():
    import numpy as np
    from biolith_amd.engine import OccuDataset
    plain = ("predict", "deterministic", "predictive_check", "predictive_density", "predictive_density marginal", "site_posterior")
    for case, (N, T, J, n) in (("N=1", (1, 1, 2, 5)), ("N=257", (257, 1, 2, 5)), ("T2J3", (70, 2, 3, 5)), ("wrap", (70, 2, 3, 1030))):
        d = data(N, T, J, 2, 2)
        run_case(case, "occu", handles(d)[0][1], d, n, only=plain)
    d = data(70, 2, 3, 5, 3)
    run_case("Ks5Ko3", "occu", handles(d)[0][1], d, 33, only=plain)
    d = data(70, 2, 3, 2, 2)
    for name, make in handles(d):
        run_case("handles", name, make, d, 33)
    d2 = data(70, 2, 3, 2, 2, species=2)
    run_case("handles", "occu two species", lambda: OccuDataset(d2["X"], d2["W"], d2["Y"]), d2, 33)
    # bl_deterministic across its chunk boundary: 8192 draws of 4 x 1 x 2048 float32 fill 256 MB, the last 8 come from a second launch
    d = data(2048, 1, 4, 2, 2)
    ds = handles(d)[0][1]()
    th = draws_for(ds, 8200)
    for want in ((True, True), (True, False), (False, True)):
        for o, a in zip(("psi", "prob_detection"), ds.deterministic(th, *want)):
            if a is not None:
                for part, b in (("", a), (" last 8 draws", a[-8:])):
                    print(f"{'chunk':10s} {'occu':20s} {'deterministic' + part:28s} {'all' if all(want) else 'alone':5s} {o:14s} {b.dtype.name:7s} {b.shape!s:18s} {sha(b)}")
    ds.close()
    # the samplers: draws | num_steps | step_size | inv_mass of a short fit
    d = data(60, 2, 3, 2, 2)
    for name, make in (handles(d)[0], handles(d)[3]):
        ds = make()
        r = ds.nuts(num_warmup=50, num_samples=50, num_chains=2, seed=5)
        h = hashlib.sha256(np.ascontiguousarray(r.draws).tobytes() + np.ascontiguousarray(r.num_steps).tobytes()
                           + np.ascontiguousarray(r.step_size).tobytes() + np.ascontiguousarray(r.inv_mass).tobytes()).hexdigest()
        print(f"{'fit':10s} {name:20s} {'nuts 50 + 50, 2 chains':28s} draws | num_steps | step_size | inv_mass {h}")
        ds.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
    else:
        listings = []
        for lib in sys.argv[1:]:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=dict(os.environ, BIOLITH_HIP_LIB=os.path.abspath(lib)),
                               stdout=subprocess.PIPE, text=True)
            if r.returncode:
                sys.exit(r.returncode) # (a fault: nothing more is started on the device)
            listings.append(r.stdout.splitlines())
        print("libraries: " + " | ".join(sys.argv[1:]))
        different = 0
        for lines in zip(*listings): # a line is "what  digest" (or a refusal's text): the same `what` must come from every library
            what, first = lines[0].rsplit(" ", 1) if " refused: " not in lines[0] else (lines[0], "")
            if len(listings) == 1:
                print(lines[0])
                continue
            same = all(l == lines[0] for l in lines[1:])
            different += not same
            rest = [l.rsplit(" ", 1)[1] if l.startswith(what + " ") and first else l for l in lines[1:]]
            print(f"{what} {first}" + "".join(f" | {x}" for x in rest if first) + ("  equal" if same else "  DIFFERENT" + ("" if first else ": " + " | ".join(rest))))
        if len(listings) > 1:
            ragged = len(set(map(len, listings))) > 1
            print(f"{len(listings[0])} lines, {different} different" + (", and the listings differ in length" if ragged else ""))
            sys.exit(1 if different or ragged else 0)
