"""One SHA-256 per output array of every post-fit entry (bl_site_posterior, bl_abundance_posterior, bl_path_posterior,
bl_score_posterior, bl_predict, bl_predict_counts, bl_predict_scores) on a fixed list of small handles, fixed draws and seed 3: two builds that print the same listing
compute the same bits.  70 sites = a 64-thread block and a partial one, 300 = a 256-thread block and a partial one; 2 periods x 3
visits with missing visits; occu_dyn once with a single period (no transitions).  Every posterior entry is also called with each
output alone.      python tools/posterior_digest.py > listing.txt"""
import contextlib
import hashlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from biolith_amd.engine import OccuDataset  # noqa: E402
from biolith_amd.models import simulate, simulate_comb, simulate_dyn, simulate_nmixture  # noqa: E402

POSTERIOR = {"site_posterior": ("log_lik", "z_prob", "z"), "abundance_posterior": ("log_lik", "n_mean", "occ_prob", "n_draw"),
             "path_posterior": ("log_lik", "z_prob", "col_prob", "ext_prob", "z")}


def handles(N):
    kw = dict(n_sites=N, n_periods=2, n_site_covs=2, n_obs_covs=2, deployment_days_per_site=21, session_duration=7, simulate_missing=True)
    with contextlib.redirect_stdout(io.StringIO()):
        d, cnt, comb = simulate(**kw)[0], simulate_nmixture(**kw)[0], simulate_comb(n_sites=N, n_periods=2, ARU_replicates=3,
                                                                                   scores_replicates=3, simulate_missing=True)[0]
        dyn = [simulate_dyn(**dict(kw, n_periods=T))[0] for T in ((2, 1) if N == 70 else (2,))]
    X, W, Y, C = d["site_covs"], d["obs_covs"], d["obs"], cnt["obs"]
    mk = lambda model, obs=Y, **o: (lambda: OccuDataset(X, W, obs, model=model, **o))
    both = dict(site_random_effects=True, obs_random_effects=True)
    out = [("occu", "site_posterior", mk("occu")), ("occu_fp constant", "site_posterior", mk("occu_fp", fp_mode="constant")),
           ("occu_fp unoccupied", "site_posterior", mk("occu_fp", fp_mode="unoccupied")), ("occu_re", "site_posterior", mk("occu_re", **both)),
           ("occu_comb", "site_posterior", lambda: OccuDataset(comb["site_covs"], comb["PC_obs_covs"], comb["PC_obs"], model="occu_comb",
                                                               ARU_obs_covs=comb["ARU_obs_covs"], ARU_obs=comb["ARU_obs"], scores_obs=comb["scores_obs"])),
           ("occu_rn", "abundance_posterior", mk("occu_rn", max_abundance=20)),
           ("occu_rn fp", "abundance_posterior", mk("occu_rn", max_abundance=20, re_fp_mode="constant")),
           ("nmixture", "abundance_posterior", mk("nmixture", C, max_abundance=20)),
           ("nmixture re", "abundance_posterior", mk("nmixture", C, max_abundance=20, **both)),
           ("occu_cs", None, mk("occu_cs", np.where(np.isnan(Y), np.nan, Y * 2.0 - 1.0))),
           ("occu_cop", None, mk("occu_cop", C, fp_mode="constant", session_duration=np.ones(Y.shape[1:])))]
    return out + [(f"occu_dyn T={g['obs'].shape[2]}", "path_posterior",
                   lambda g=g: OccuDataset(g["site_covs"], g["obs_covs"], g["obs"], model="occu_dyn")) for g in dyn]


def main():
    for N in (70, 300):
        for name, posterior, make in handles(N):
            ds = make()
            th = np.random.default_rng(0).uniform(-1, 1, size=(5, ds.D)).astype(np.float32)
            calls = []
            if posterior:
                outs = POSTERIOR[posterior]
                calls.append((posterior, outs, getattr(ds, posterior)(th, seed=3)))
                for i, o in enumerate(outs):
                    only = getattr(ds, posterior)(th, seed=3, **{k: k == o for k in outs})
                    calls.append((f"{posterior} {o} alone", (o,), (only[i],)))
            if ds.model == "occu_cs":
                calls.append(("predictive_scores", ("z", "f", "s"), ds.predictive_scores(th, seed=3)))
                calls.append(("score_posterior", ("log_lik", "z_prob", "z", "f_prob", "f"), ds.score_posterior(th, seed=3)))
                calls.append(("score_posterior cells alone", ("log_lik", "z_prob", "z"), ds.score_posterior(th, seed=3, visits=False)[:3]))
            elif ds.model not in ("occu_dyn", "occu_comb"):
                calls.append(("predictive", ("latent", "y"), ds.predictive(th, seed=3)))
            for entry, outs, arrays in calls:
                for o, a in zip(outs, arrays):
                    sha = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
                    print(f"{name:18s} N={N:<3d} {entry:34s} {o:8s} {a.dtype.name:7s} {a.shape!s:16s} {sha}")
            ds.close()


if __name__ == "__main__":
    main()
