// site_diagnostics.hpp -- what bl_site_diagnostics (biolith_hip.hip) hands to its kernels (site_diagnostics.hip, a translation unit of its
// own: no existing kernel is recompiled next to it).
//
// The kernels read what bl_site_summary's read -- the site covariates at the head of the handle's rows, the raw observation covariates
// -- and all the draws at once, chain-major: chain c owns draws c n .. c n + n - 1.  They write per cell (a site, or (j, t, site) in
// bl_deterministic's order) and nothing per draw.  The only workspace is three float64 means per chain and thread (the chain's and its
// two halves'), which a thread writes and reads back itself: it grows with the chains, not with the draws.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/biolith_hip.h"
#include "draw_coords.hpp"

constexpr int BL_SD_THREADS = 256;
// the lags a pass over a chain sums at once (BL_SD_LAGS / 2 pairs of Geyer's sequence): an accumulator each and a ring of as many trailing
// values, all at static register indices
constexpr int BL_SD_LAGS = 32;

struct BlSiteDiagnosticsParams {
    const float *rows;   // rows 0 .. Ks - 1 = the site covariates, [.][ns], NaN -> 0
    const float *wraw;   // [T J][Ko][ns], site-fastest, NaN -> 0 (the second site only)
    int ns, N, T, J, Ks, Ko, D;
    int model;           // the plain model whose branch the handle runs, as BlPredictParams::model
    BlDrawCoords c;
    const float *draws;  // [n_chains n][D], device: all of them, chain-major
    int n_chains, n;     // chains, draws per chain (>= 2)
    double *means;       // device workspace [n_chains][3][threads of the launch]: the chain's mean, its first half's, its second half's
    // device, NULL = skip; cells = N (the first site) or J T N (the second)
    double *n_eff, *r_hat, *mean, *sd; // [cells]
};

extern "C" int bl_launch_site_diagnostics_psi(const BlSiteDiagnosticsParams *p, hipStream_t st);
extern "C" int bl_launch_site_diagnostics_prob(const BlSiteDiagnosticsParams *p, hipStream_t st);
// the float64 values the launch's workspace holds (BlSiteDiagnosticsParams::means)
size_t bl_site_diagnostics_workspace(const BlSiteDiagnosticsParams *p, bool visit);
