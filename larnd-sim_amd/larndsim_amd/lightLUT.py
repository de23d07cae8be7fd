"""Light incidence from the look-up table -- mirrors larndsim/lightLUT.py:65-136 -- and the host twin of the trilinear
visibility interpolation (context option ``light_lut_interp``)."""
import ctypes as C

import numpy as np

from . import consts, lib
from ._kernel import kernel
from .layout import make_layout

def _ensure_lut(lut):
    lib.set_light(lut)                # channel tables always, the LUT only when it is not already resident


@kernel
def calculate_light_incidence(tracks, lut, light_incidence, voxel):
    """``calculate_light_incidence[bpg, tpb](tracks, lut, light_incidence, voxel)``; ``light_incidence`` is the
    structured array with ``n_photons_det`` / ``t0_det`` (f4) the reference driver allocates.  Like the reference the call
    writes into what the caller passed: rows of segments outside every TPC, and ``t0_det`` in trigger mode 1, keep their values
    (under the context option ``light_lut_interp`` they read zero, like the numpy twin's)."""
    lay = make_layout(tracks.dtype)
    n, n_out = light_incidence.shape
    lib.context()
    _ensure_lut(lut)
    nph = np.array(light_incidence['n_photons_det'], dtype=np.float32, order='C')
    t0d = (np.array(light_incidence['t0_det'], dtype=np.float32, order='C') if 't0_det' in light_incidence.dtype.names
           else np.zeros((n, n_out), dtype=np.float32))
    vox = np.array(voxel, dtype=np.int32, order='C')
    if vox.shape != (n, 3):
        raise ValueError("voxel must be [n_tracks, 3]")
    lib.check(lib.load().ldsim_light_incidence(lib.context(refresh_consts=False), lib.ptr(tracks), C.c_int64(n),
                                               C.byref(lay), C.c_int32(n_out), lib.ptr(nph), lib.ptr(t0d),
                                               lib.ptr(vox)))
    light_incidence['n_photons_det'] = nph
    if 't0_det' in light_incidence.dtype.names:
        light_incidence['t0_det'] = t0d
    voxel[:] = vox


# ---- trilinear visibility between voxel centres (context option "light_lut_interp") ------------
# The numpy f64 twin of light_incidence_interp_kernel: the same fractions, corner order and summation order, so a LUT can be
# checked offline and the GPU tests have their expected value.  One arithmetic, stated in the kernel file's comment:
#   f = get_voxel's fraction before it truncates, u = f - 0.5, i0 = floor(u), w1 = u - i0, w0 = 1 - w1,
#   corners clamp(i0), clamp(i0 + 1) per axis; corner c = 4 dx + 2 dy + dz weighs (wx[dx] * wy[dy]) * wz[dz].
_MUS = 1e-6 * 1e9           # the reference's units.mus / units.ns as the kernels and the oracle spell it


def _lut_fractions(x, y, z, itpc, lut_vox_div):
    """(fx, fy, fz): the voxel coordinates of lightLUT.get_voxel (larndsim/lightLUT.py:15-63) before the cast to int"""
    nx, ny, nz = (int(v) for v in lut_vox_div)
    b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[itpc]
    is_even = b[:, 2, 1] > b[:, 2, 0]
    x_min, x_max = b[:, 0, 0] - 2e-2, b[:, 0, 1] + 2e-2
    y_min, y_max = b[:, 1, 0] - 2e-2, b[:, 1, 1] + 2e-2
    z_min, z_max = b[:, 2, 0] - 2e-2, b[:, 2, 1] + 2e-2
    fx = np.where(is_even, (x - x_min) / (x_max - x_min) * nx, (x_max - x) / (x_max - x_min) * nx)
    fy = (y_max - y) / (y_max - y_min) * ny
    fz = (z - z_min) / (z_max - z_min) * nz
    return fx, fy, fz


def _axis_corners(f, n):
    u = f - 0.5
    i0 = np.floor(u)
    w1 = u - i0
    w0 = 1.0 - w1
    lo = np.clip(i0, 0, n - 1).astype(np.int64)
    hi = np.clip(i0 + 1.0, 0, n - 1).astype(np.int64)
    return np.stack([lo, hi], axis=-1), np.stack([w0, w1], axis=-1)


def interpolation_corners(x, y, z, itpc, lut_vox_div):
    """The eight LUT voxels around each position and their trilinear weights.

    ``x, y, z``: positions [n] in the frame ``calculate_light_incidence`` sees them in; ``itpc``: TPC index (scalar or [n]);
    ``lut_vox_div``: (nx, ny, nz).  Returns (corner indices [n, 8, 3] i8, weights [n, 8] f8), corner c = 4 dx + 2 dy + dz.
    Beyond the outermost voxel centres both corners of an axis are the same voxel: the field is constant there."""
    x, y, z = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (x, y, z))
    itpc = np.broadcast_to(np.asarray(itpc, dtype=np.int64), x.shape)
    nx, ny, nz = (int(v) for v in lut_vox_div)
    fx, fy, fz = _lut_fractions(x, y, z, itpc, (nx, ny, nz))
    (ix, wx), (iy, wy), (iz, wz) = _axis_corners(fx, nx), _axis_corners(fy, ny), _axis_corners(fz, nz)
    idx = np.zeros((len(x), 8, 3), dtype=np.int64)
    w = np.zeros((len(x), 8))
    for c in range(8):
        dx, dy, dz = c >> 2, (c >> 1) & 1, c & 1
        idx[:, c, 0], idx[:, c, 1], idx[:, c, 2] = ix[:, dx], iy[:, dy], iz[:, dz]
        w[:, c] = (wx[:, dx] * wy[:, dy]) * wz[:, dz]
    return idx, w


def interpolated_light_incidence(tracks, lut, n_out=None):
    """``calculate_light_incidence`` with the visibility interpolated trilinearly between voxel centres, on the host in f64:
    what the kernels compute under ``lib.set_option("light_lut_interp", 1)``.

    Returns (n_photons_det [n, n_out] f4, t0_det [n, n_out] f4, voxel [n, 3] i4).  ``t0_det`` (threshold trigger only) is the
    mean of the corners' ``t0`` over the corners with visibility > 0, renormalised by their weights, and the nearest voxel's
    where none is lit.  ``voxel`` is the nearest voxel as before: ``sum_light_signals`` takes the time profile from it, whose
    shape is not interpolated.  Segments outside every TPC keep zeros."""
    det, light = consts.detector, consts.light
    n = len(tracks)
    n_out = int(light.N_OP_CHANNEL if n_out is None else n_out)
    nx, ny, nz, ndet = lut.shape
    nph = np.zeros((n, n_out), dtype=np.float32)
    t0d = np.zeros((n, n_out), dtype=np.float32)
    vox = np.zeros((n, 3), dtype=np.int32)
    plane = np.asarray(tracks["pixel_plane"], dtype=np.int64)
    rows = np.flatnonzero((plane != det.DEFAULT_PLANE_INDEX) & (plane >= 0) & (plane < len(det.TPC_BORDERS)))
    if not len(rows) or not n_out:
        return nph, t0d, vox
    itpc = plane[rows]
    x, y, z = (np.asarray(tracks[k][rows], dtype=np.float64) for k in ("x", "y", "z"))
    for a, f, m in zip(range(3), _lut_fractions(x, y, z, itpc, (nx, ny, nz)), (nx, ny, nz)):
        vox[rows, a] = np.clip(np.trunc(f), 0, m - 1).astype(np.int32)
    idx, w = interpolation_corners(x, y, z, itpc, (nx, ny, nz))
    vis = np.asarray(lut["vis"], dtype=np.float32)
    t0 = np.asarray(lut["t0"], dtype=np.float32)
    li = np.arange(n_out) % ndet
    trig0 = light.LIGHT_TRIG_MODE == 0
    vis_i, S, T = (np.zeros((len(rows), n_out)) for _ in range(3))
    for c in range(8):
        at = (idx[:, c, 0], idx[:, c, 1], idx[:, c, 2])
        v = vis[at][:, li]
        wc = w[:, c, None]
        vis_i += wc * v.astype(np.float64)
        if trig0:
            S += np.where(v > 0, wc, 0.0)
            T += np.where(v > 0, wc * t0[at][:, li].astype(np.float64), 0.0)
    off = n_out * (itpc // 2) if n_out < light.N_OP_CHANNEL else np.zeros_like(itpc)
    op = np.arange(n_out)[None, :] + off[:, None]
    own = np.asarray(light.OP_CHANNEL_TO_TPC)[op] == itpc[:, None]
    eff = np.asarray(light.OP_CHANNEL_EFFICIENCY, dtype=np.float64)[op]
    n_photons = np.asarray(tracks["n_photons"][rows], dtype=np.float64)[:, None]
    nph[rows] = (eff * (vis_i * own) * n_photons).astype(np.float32)
    if trig0:
        nearest = t0[vox[rows, 0], vox[rows, 1], vox[rows, 2]][:, li].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0_lut = np.where(S > 0, T / S, nearest)
        seg_t0 = np.asarray(tracks["t0"][rows], dtype=np.float64)[:, None]
        t0d[rows] = ((t0_lut * 1.0 + seg_t0 * _MUS) / _MUS).astype(np.float32)
    return nph, t0d, vox
