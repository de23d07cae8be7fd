"""Inputs shared by tests/test_cpu_light_interp.py and tests/test_gpu_light_interp.py: positions stated as LUT voxel
coordinates (the fractions of lightLUT.get_voxel before it truncates), LUTs and segment records."""
import numpy as np

import helpers as H
from larndsim_amd import consts, synth


def padded_borders(itpc):
    """(x_min, x_max, y_min, y_max, z_min, z_max) of lightLUT.get_voxel for TPC ``itpc``: the borders -+ 2e-2"""
    b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[itpc]
    return b[0][0] - 2e-2, b[0][1] + 2e-2, b[1][0] - 2e-2, b[1][1] + 2e-2, b[2][0] - 2e-2, b[2][1] + 2e-2


def position(fx, fy, fz, itpc, vox_div):
    """the position whose voxel coordinates are (fx, fy, fz) in TPC ``itpc`` (up to the rounding of the way back)"""
    nx, ny, nz = vox_div
    b = np.asarray(consts.detector.TPC_BORDERS)[itpc]
    x_min, x_max, y_min, y_max, z_min, z_max = padded_borders(itpc)
    even = b[2][1] > b[2][0]
    x = x_min + fx / nx * (x_max - x_min) if even else x_max - fx / nx * (x_max - x_min)
    return x, y_max - fy / ny * (y_max - y_min), z_min + fz / nz * (z_max - z_min)


def records(x, y, z, itpc, seed):
    """segment records at the given positions (what the light incidence reads: position, TPC, photons, time)"""
    n = len(x)
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=H.REF_DTYPE)
    r["segment_id"] = np.arange(n)
    r["x"], r["y"], r["z"], r["pixel_plane"] = x, y, z, itpc
    r["n_photons"] = H.f4(rng.uniform(1e3, 1e5, n))
    r["t0"] = rng.uniform(0.0, 50.0, n)
    r["t0_start"], r["t0_end"] = r["t0"], r["t0"]
    return r


def mixed_segments(n, vox_div, seed, outside_every=11):
    """``n`` segment records over all TPCs of the loaded configuration, by row index modulo 4: uniform in the TPC; within 1e-3 cm
    of one of the six TPC borders (the clamp region: the outermost voxel centres lie half a voxel further in), the borders taken
    in turn; exactly on a voxel centre; on a voxel face.  Every ``outside_every``-th row (from row 5) is outside every TPC."""
    rng = np.random.default_rng(seed)
    n_tpc = len(consts.detector.TPC_BORDERS)
    dims = np.array(vox_div)
    xs, ys, zs, tp = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    for i in range(n):
        itpc = int(rng.integers(0, n_tpc))
        f = rng.uniform(0, 1, 3) * dims
        kind = i % 4
        if kind == 2:
            f = np.floor(f) + 0.5
        elif kind == 3:
            a = int(rng.integers(0, 3))
            f[a] = float(rng.integers(0, dims[a] + 1))
        x, y, z = position(f[0], f[1], f[2], itpc, vox_div)
        if kind == 1:
            b = np.sort(np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[itpc], axis=-1)
            a, side = (i // 4) % 3, (i // 12) % 2
            p = [x, y, z]
            p[a] = b[a][side] + (1 - 2 * side) * rng.uniform(0, 1e-3)
            x, y, z = p
        xs[i], ys[i], zs[i], tp[i] = x, y, z, itpc
    r = records(xs, ys, zs, tp, seed + 1)
    r["pixel_plane"][5::outside_every] = consts.detector.DEFAULT_PLANE_INDEX
    return r


def small_lut(vox_div, n_det, seed, n_prof=8):
    return synth.make_lut(tuple(vox_div), n_det, n_prof, seed)


def ulp_close(got, exp):
    """within 1 f4 ulp of the expected f4 value, everywhere"""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    return bool((np.abs(got.astype(np.float64) - exp.astype(np.float64)) <= np.spacing(np.abs(exp)).astype(np.float64)).all())
