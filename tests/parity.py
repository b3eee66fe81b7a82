"""The sampler's own log density against the float64 oracle, draw by draw (TEST INFRASTRUCTURE).

Every kept draw comes with the potential the persistent kernel computed for it inside its tree (cold->potential[s] = (float)U,
nuts_kernel.hpp; R.potential[s], re_kernel.hpp), at the kernel form, the workgroups per chain and the exchange the launch ran.  The
oracle evaluates U in float64 at the stored float32 draw, so every transition of every chain is checked against a plain
high-precision reference:  |potential_energy - U_oracle| <= rtol |U_oracle| + ulp32(U_oracle) / 2  (the half ulp is the float32 store)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ORACLE_THREADS = 16   # the oracle's C code holds no state between calls; ctypes lets go of the GIL around each one


def potential_at_draws(od, result):
    """U of the oracle in float64 at every stored draw: shape (C, S)."""
    draws = np.asarray(result.draws, dtype=np.float64)
    Cn, S, D = draws.shape
    assert D == od.D, (D, od.D)
    flat = draws.reshape(-1, D)
    n = flat.shape[0]
    parts = np.array_split(np.arange(n), min(ORACLE_THREADS, n))
    with ThreadPoolExecutor(max_workers=len(parts)) as ex:
        Us = list(ex.map(lambda idx: od.potential_grad(flat[idx])[0], parts))
    return np.concatenate(Us).reshape(Cn, S)


def half_ulp32(x):
    """Half a float32 ulp at |x| (the rounding of the kernel's double U to the float32 it stores)."""
    return 0.5 * np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def potential_ratio(U, Uo, rtol):
    """|U - Uo| / (rtol |Uo| + ulp32(Uo) / 2): <= 1 passes."""
    U, Uo = np.asarray(U, dtype=np.float64), np.asarray(Uo, dtype=np.float64)
    return np.abs(U - Uo) / (rtol * np.abs(Uo) + half_ulp32(Uo))


def relative_excess(U, Uo):
    """max over draws of (|U - Uo| - ulp32(Uo) / 2)+ / |Uo|: the relative error beyond the float32 store (what rtol bounds)."""
    U, Uo = np.asarray(U, dtype=np.float64), np.asarray(Uo, dtype=np.float64)
    return float(np.max(np.maximum(np.abs(U - Uo) - half_ulp32(Uo), 0.0) / np.abs(Uo)))


def assert_potential_parity(result, Uo, rtol, label):
    """Every draw, potential and step size finite; every potential within rtol (+ half a float32 ulp) of the oracle's.
    Returns (worst ratio, relative excess) for the record."""
    assert np.all(np.isfinite(result.draws)), f"{label}: non-finite draw"
    assert np.all(np.isfinite(result.potential_energy)), f"{label}: non-finite potential"
    assert np.all(np.isfinite(result.step_size)) and np.all(result.step_size > 0), f"{label}: step sizes {result.step_size}"
    assert np.all(np.isfinite(Uo)), f"{label}: the oracle's potential is not finite at a stored draw"
    U = np.asarray(result.potential_energy, dtype=np.float64)
    assert U.shape == Uo.shape, (U.shape, Uo.shape)
    ratio = potential_ratio(U, Uo, rtol)
    c, s = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[c, s])
    assert worst <= 1.0, (f"{label}: chain {c} draw {s}: kernel U {U[c, s]!r} oracle U {Uo[c, s]!r} (|dU| / |U| = "
                          f"{abs(U[c, s] - Uo[c, s]) / abs(Uo[c, s]):.3g}), {worst:.3g} x the bound at rtol {rtol:g}; "
                          f"{int((ratio > 1).sum())} of {ratio.size} draws out")
    return worst, relative_excess(U, Uo)


def describe_launch(ds):
    """The form the last launch of ``ds`` ran: kernel instantiation, workgroups per chain, threads per workgroup, rows in LDS, chains on
    the L2-local exchange, lanes per site pair (bl_nuts_kernel_name, bl_nuts_geometry, bl_nuts_lane_group)."""
    k, thr, lds, staged, loc = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert ds._lib.bl_nuts_geometry(ds._h, C.byref(k), C.byref(thr), C.byref(lds), C.byref(staged), C.byref(loc)) == 0
    gt, gj = C.c_int(1), C.c_int(1)
    assert ds._lib.bl_nuts_lane_group(ds._h, C.byref(gt), C.byref(gj)) == 0
    return dict(kernel=ds._kernel_name(), wgs_per_chain=int(k.value), threads=int(thr.value), lds_staged=bool(staged.value & 1),
                chains_on_l2_local_exchange=int(loc.value), lane_group=(int(gt.value), int(gj.value)))
