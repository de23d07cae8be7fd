#!/usr/bin/env python3
"""
TEST INFRASTRUCTURE -- golden-vector generator (runs only in the build container).

Imports the reference's own, unmodified Python kernels from /root/reference and runs
them serially on small seeded inputs, writing NUMBERS-ONLY fixtures to tests/golden/
and constants snapshots to larnd-sim_amd/larndsim_amd/snapshots/.

The reference kernels are Numba ``@cuda.jit`` functions; numba / cupy / h5py / larpix
are not installed here (ordinary ModuleNotFoundError), so minimal stand-in modules are
placed in ``sys.modules``: ``numba.njit`` = identity, ``numba.cuda.jit`` =
a launcher that walks the launch grid serially and serves ``cuda.grid`` /
``cuda.gridsize`` / ``cuda.atomic``; ``cupy`` = numpy.  No reference source or bytecode
is written anywhere; the fixtures hold inputs and outputs only.

Faithfulness rules (Numba types arithmetic as f64; NumPy-2 scalars do not):
  * float record fields are f8 but hold f4-representable values; integer fields keep
    their real dtypes (u4 n_electrons -> truncation on store, i4 pixel_plane);
  * between stages the mutated float fields are rounded through f4 (the HDF5 schema);
  * FEE noise constants are 0 (the Numba RNG stream is third-party and unpinned).

Usage:  python oracle/gen_golden.py [--sets consts,qd,pixels,pixels_wide,chain,sampled,light,light_response,light_wvfm,light_wvfm_edges,light_edges,fee,mc] [--jobs 8]
"""
import argparse
import importlib
import itertools
import json
import os
import sys
import types
from multiprocessing import Pool

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLD = os.path.join(REPO, "tests", "golden")
SNAP = os.path.join(REPO, "larnd-sim_amd", "larndsim_amd", "snapshots")
sys.path.insert(0, os.path.join(REPO, "larnd-sim_amd"))
sys.path.insert(0, REPO)

CONFIGS = {
    "module0": ("detector_properties/module0.yaml", "pixel_layouts/multi_tile_layout-2.3.16.yaml",
                "simulation_properties/singles_sim.yaml"),
    "2x2_no_modvar": ("detector_properties/2x2_no_modvar.yaml", "pixel_layouts/multi_tile_layout-2.4.16.yaml",
                      "simulation_properties/2x2_NuMI_sim_no_modvar.yaml"),
    "ndlar": ("detector_properties/ndlar-module.yaml", "pixel_layouts/multi_tile_layout-3.0.40.yaml",
              "simulation_properties/NDLAr_LBNF_sim.yaml"),
}


# --------------------------------------------------------------------------
# stand-in modules
# --------------------------------------------------------------------------
class _State:
    pos = (0, 0, 0)
    size = (1, 1, 1)
    z_only = None       # optional iterable restricting the 3rd grid axis (sampled ticks)
    x_only = None       # optional iterable restricting the 1st grid axis (one segment per worker; the grid size stays)


def _tup3(v):
    if isinstance(v, (int, np.integer)):
        return (int(v), 1, 1)
    v = tuple(int(x) for x in v)
    return v + (1,) * (3 - len(v))


class _Kernel:
    def __init__(self, fn):
        self.fn = fn

    def __getitem__(self, cfg):
        bpg, tpb = _tup3(cfg[0]), _tup3(cfg[1])
        size = tuple(b * t for b, t in zip(bpg, tpb))

        def launch(*args):
            _State.size = size
            zs = range(size[2]) if _State.z_only is None else [z for z in _State.z_only if z < size[2]]
            for x in (range(size[0]) if _State.x_only is None else [x for x in _State.x_only if x < size[0]]):
                for y in range(size[1]):
                    for z in zs:
                        _State.pos = (x, y, z)
                        self.fn(*args)
        return launch


def _install_standins(normal=None):
    """normal: the stand-in for numba.cuda.random.xoroshiro128p_normal_float32 (None: every normal is 0.0)"""
    numba = types.ModuleType("numba")
    cuda = types.ModuleType("numba.cuda")
    crandom = types.ModuleType("numba.cuda.random")
    nerrors = types.ModuleType("numba.core.errors")

    def njit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    def cjit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return _Kernel(a[0])
        return (lambda f: f) if k.get("device") else (lambda f: _Kernel(f))

    def grid(n):
        return _State.pos[0] if n == 1 else tuple(_State.pos[:n])

    def gridsize(n):
        return _State.size[0] if n == 1 else tuple(_State.size[:n])

    class _Atomic:
        @staticmethod
        def add(arr, idx, val):
            arr[idx] += val

        @staticmethod
        def max(arr, idx, val):
            if val > arr[idx]:
                arr[idx] = val

    numba.njit = njit
    numba.cuda = cuda
    cuda.jit = cjit
    cuda.grid = grid
    cuda.gridsize = gridsize
    cuda.atomic = _Atomic
    cuda.random = crandom
    cuda.to_device = lambda a: a
    cuda.device_array = lambda n, dtype=None: np.zeros(n, dtype=dtype)
    crandom.xoroshiro128p_normal_float32 = normal if normal is not None else (lambda states, i: 0.0)
    crandom.xoroshiro128p_uniform_float32 = lambda states, i: 0.5
    crandom.create_xoroshiro128p_states = lambda n, seed=0: np.zeros(n)
    nerrors.NumbaPerformanceWarning = Warning
    numba.core = types.ModuleType("numba.core")
    numba.core.errors = nerrors

    cupy = types.ModuleType("cupy")
    for name in dir(np):
        if not name.startswith("__"):
            setattr(cupy, name, getattr(np, name))
    cupy.get_array_module = lambda *a: np
    cupy.asnumpy = np.asarray
    cupy.cuda = types.ModuleType("cupy.cuda")

    mods = {"numba": numba, "numba.cuda": cuda, "numba.cuda.random": crandom, "numba.core": numba.core,
            "numba.core.errors": nerrors, "cupy": cupy, "cupy.cuda": cupy.cuda, "h5py": types.ModuleType("h5py")}
    larpix = types.ModuleType("larpix")
    for sub, names in (("packet", ["Packet_v2", "TimestampPacket", "TriggerPacket", "SyncPacket", "PacketCollection"]),
                       ("key", ["Key"]), ("format", ["hdf5format"])):
        m = types.ModuleType("larpix." + sub)
        for nm in names:
            setattr(m, nm, type(nm, (), {}))
        setattr(larpix, sub, m)
        mods["larpix." + sub] = m
    mods["larpix"] = larpix
    sys.modules.update(mods)


class Ref:
    """The reference package loaded for one configuration."""

    def __init__(self, cfgname, noise_zero=True, normal=None):
        _install_standins(normal)
        if REF not in sys.path:
            sys.path.insert(0, REF)
        for m in [m for m in sys.modules if m == "larndsim" or m.startswith("larndsim.")]:
            del sys.modules[m]
        det, pix, simf = (os.path.join(REF, "larndsim", p) for p in CONFIGS[cfgname])
        from larndsim import consts
        consts.load_properties(det, pix, simf)
        if noise_zero:
            consts.detector.RESET_NOISE_CHARGE = 0
            consts.detector.UNCORRELATED_NOISE_CHARGE = 0
            consts.detector.DISCRIMINATOR_NOISE = 0
        self.consts = consts
        from larndsim.consts import physics, units
        consts.physics, consts.units = physics, units
        self.detector, self.light, self.sim, self.physics = consts.detector, consts.light, consts.sim, physics
        for name in ("quenching", "drifting", "pixels_from_track", "detsim", "fee", "lightLUT", "light_sim"):
            setattr(self, name, importlib.import_module("larndsim." + name))


# --------------------------------------------------------------------------
# record helpers
# --------------------------------------------------------------------------
F4_FIELDS = ["x_start", "y_start", "z_start", "x_end", "y_end", "z_end", "x", "y", "z", "dx", "dEdx", "dE",
             "t", "t_start", "t_end", "n_photons", "long_diff", "tran_diff"]
REF_DTYPE = np.dtype([("event_id", "u4"), ("segment_id", "u4"), ("traj_id", "u4"), ("n_electrons", "u4"),
                      ("pixel_plane", "i4")] + [(f, "f8") for f in F4_FIELDS] +
                     [("t0", "f8"), ("t0_start", "f8"), ("t0_end", "f8")])


def f4(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def to_ref(seg):
    """152-B schema (or any structured array) -> reference-run records (f8 floats holding f4 values)."""
    r = np.zeros(seg.shape[0], dtype=REF_DTYPE)
    for n in REF_DTYPE.names:
        if n in seg.dtype.names:
            r[n] = seg[n]
    return r


def round_f4_fields(r, fields):
    for n in fields:
        r[n] = f4(r[n])


def swap_xz(seg):
    for a, b in (("x_start", "z_start"), ("x_end", "z_end"), ("x", "z")):
        tmp = seg[a].copy(); seg[a] = seg[b]; seg[b] = tmp
    return seg


def hand_segments(det, n, seed, plane_choices=None, long_frac=0.2, steep_frac=0.25, dtype=None):
    """Diverse hand-made segments in the TPC frame (post-swap), f4-rounded."""
    from larndsim_amd.layout import segments_dtype
    rng = np.random.default_rng(seed)
    seg = np.zeros(n, dtype=segments_dtype)
    B = np.asarray(det.TPC_BORDERS)
    sb = np.sort(B, axis=-1)
    ntpc = B.shape[0]
    for i in range(n):
        p = int(rng.integers(0, ntpc)) if plane_choices is None else int(rng.choice(plane_choices))
        lo, hi = sb[p, :, 0] + 0.8, sb[p, :, 1] - 0.8
        c = rng.uniform(lo, hi)
        L = rng.uniform(0.3, 1.6) if rng.random() < long_frac else rng.uniform(0.03, 0.5)
        if rng.random() < steep_frac:
            cz = rng.choice([-1, 1]) * rng.uniform(0.9, 0.9995)
        else:
            cz = rng.uniform(-1, 1)
        ph = rng.uniform(0, 2 * np.pi)
        s = np.sqrt(1 - cz * cz)
        d = np.array([s * np.cos(ph), s * np.sin(ph), cz])
        a, b = c - 0.5 * L * d, c + 0.5 * L * d
        seg["x_start"][i], seg["y_start"][i], seg["z_start"][i] = a
        seg["x_end"][i], seg["y_end"][i], seg["z_end"][i] = b
        seg["dx"][i] = L
        seg["dEdx"][i] = np.clip(rng.normal(2.1, 0.6), 0.5, 12.0)
        seg["event_id"][i] = 0
    for ax in "xyz":
        seg[ax] = 0.5 * (seg[ax + "_start"].astype(np.float64) + seg[ax + "_end"])
    seg["dE"] = seg["dEdx"].astype(np.float64) * seg["dx"]
    seg["segment_id"] = np.arange(n)
    seg["traj_id"] = np.arange(n) // 3
    return seg


def corner_segments(det, n, seed):
    """Geometry corners for tracks_current (the shapes tools/fuzz_chain.py's last three flavours draw): segments hugging a TPC
    face in x / y (neighbour pixels fall off the plane -> pID -1 slots), very short ones (0.5-50 um), nearly along the drift
    axis (0.1-0.8 degrees off it) and nearly perpendicular to it (|dz| ~ 1e-4 of the length), plus a heavily ionising long one."""
    seg = hand_segments(det, n, seed)
    rng = np.random.default_rng(seed + 1000)
    B = np.sort(np.asarray(det.TPC_BORDERS), axis=-1)
    for i in range(n):
        flavour = i % 5
        p = int(rng.integers(0, B.shape[0]))
        lo, hi = B[p, :, 0] + 0.8, B[p, :, 1] - 0.8
        c = rng.uniform(lo, hi)
        L, cz, ph = rng.uniform(0.05, 0.6), rng.uniform(-0.9, 0.9), rng.uniform(0, 2 * np.pi)
        if flavour == 0:                         # hugging a face: centre 0.02-0.2 cm inside the border in x or y
            ax = int(rng.integers(0, 2))
            side = int(rng.integers(0, 2))
            c[ax] = B[p, ax, side] + (1 - 2 * side) * rng.uniform(0.02, 0.2)
            L = rng.uniform(0.02, 0.3)
        elif flavour == 1:                       # very short
            L = 10 ** rng.uniform(-4.3, -2.3)
        elif flavour == 2:                       # along the drift axis
            # 0.1-0.8 degrees off the axis: closer to it the reference's z_interval hands its slice loop ranges that take the
            # pure-Python launcher hours per segment (the HIP-vs-oracle fuzz covers 1e-7 off the axis in seconds)
            cz = rng.choice([-1, 1]) * (1 - 10 ** rng.uniform(-5.7, -4))
            L = rng.uniform(0.05, 0.4)
        elif flavour == 3:                       # perpendicular to it
            cz = rng.choice([-1, 1]) * 10 ** rng.uniform(-5, -3.5)
            L = rng.uniform(0.1, 1.0)
        else:                                    # heavily ionising, long
            L = rng.uniform(1.0, 1.6)
            seg["dEdx"][i] = rng.uniform(8, 30)
        sxy = np.sqrt(max(0.0, 1 - cz * cz))
        d = np.array([sxy * np.cos(ph), sxy * np.sin(ph), cz])
        a, b = c - 0.5 * L * d, c + 0.5 * L * d
        seg["x_start"][i], seg["y_start"][i], seg["z_start"][i] = a
        seg["x_end"][i], seg["y_end"][i], seg["z_end"][i] = b
        seg["dx"][i] = L
    for ax in "xyz":
        seg[ax] = 0.5 * (seg[ax + "_start"].astype(np.float64) + seg[ax + "_end"])
    seg["dE"] = seg["dEdx"].astype(np.float64) * seg["dx"]
    return seg


def run_quench_drift(ref, r, mode):
    n = r.shape[0]
    ref.quenching.quench[max(1, -(-n // 256)), 256](r, mode)
    round_f4_fields(r, ["n_photons"])
    ref.drifting.drift[max(1, -(-n // 256)), 256](r)
    round_f4_fields(r, ["long_diff", "tran_diff", "t", "t_start", "t_end"])
    return r


# --------------------------------------------------------------------------
# fixture sets
# --------------------------------------------------------------------------
def gen_consts():
    from larndsim_amd import consts as my
    os.makedirs(SNAP, exist_ok=True)
    for cfg in CONFIGS:
        ref = Ref(cfg, noise_zero=False)
        snap = my.snapshot_dict(ref.detector, ref.light, ref.sim)
        with open(os.path.join(SNAP, cfg + ".json"), "w") as f:
            json.dump(snap, f)
        print("snapshot", cfg, "TPCs", np.asarray(ref.detector.TPC_BORDERS).shape[0])
    # the module-variation configuration `2x2` of the reference's config.yaml: detector properties 2x2.yaml, pixel layouts
    # [2.4.16, 2.5.16] with PIXEL_LAYOUT_ID [0, 0, 1, 0], 2x2_NuMI_sim.yaml -- one snapshot per module, loaded the way the
    # driver's module loop does (cli/simulate_pixels.py:452-454, 678-682)
    ref = Ref("2x2_no_modvar", noise_zero=False)
    R = os.path.join(REF, "larndsim")
    layouts = [os.path.join(R, "pixel_layouts", f) for f in ("multi_tile_layout-2.4.16.yaml", "multi_tile_layout-2.5.16.yaml")]
    per_module = [layouts[i] for i in (0, 0, 1, 0)]
    det = os.path.join(R, "detector_properties", "2x2.yaml")
    for i_mod in (1, 2, 3, 4):
        ref.consts.light.set_light_properties(det)
        ref.consts.sim.set_simulation_properties(os.path.join(R, "simulation_properties", "2x2_NuMI_sim.yaml"))
        ref.consts.detector.set_detector_properties(det, per_module, i_mod)
        snap = my.snapshot_dict(ref.consts.detector, ref.consts.light, ref.consts.sim)
        with open(os.path.join(SNAP, f"2x2_mod{i_mod}.json"), "w") as f:
            json.dump(snap, f)
        print("snapshot 2x2 module", i_mod, "pitch", ref.consts.detector.PIXEL_PITCH, "bin", ref.consts.detector.RESPONSE_BIN_SIZE,
              "sampling", ref.consts.detector.RESPONSE_SAMPLING, "N_PIXELS", ref.consts.detector.N_PIXELS)


def gen_qd():
    """quench (Birks + Box) and drift on 152-B-schema values incl. edge cases."""
    for cfg, seed in (("module0", 11), ("2x2_no_modvar", 12), ("ndlar", 13)):
        ref = Ref(cfg)
        seg = hand_segments(ref.detector, 48, seed)
        # edge cases: dEdx = 0, huge dEdx, midpoint outside every TPC, nonzero t0
        seg["dEdx"][0] = 0.0; seg["dE"][0] = 1.0
        seg["dEdx"][1] = 1e10; seg["dE"][1] = 1e10
        for f in ("x", "x_start", "x_end"):
            seg[f][2] += 500.0
        seg["t0"][3:] = np.random.default_rng(seed).uniform(0, 5, 45)
        seg["t0_start"] = seg["t0"]; seg["t0_end"] = seg["t0"]
        out = {"segments_in": seg}
        for mode, name in ((ref.physics.BIRKS, "birks"), (ref.physics.BOX, "box")):
            r = to_ref(seg)
            ref.quenching.quench[1, 256](r, mode)
            round_f4_fields(r, ["n_photons"])
            out[f"{name}_n_electrons"] = r["n_electrons"].copy()
            out[f"{name}_n_photons"] = r["n_photons"].copy()
            if name == "birks":
                ref.drifting.drift[1, 256](r)
                for f in ("pixel_plane", "n_electrons", "long_diff", "tran_diff", "t", "t_start", "t_end"):
                    out["drift_" + f] = r[f].copy()          # f64 values before f4 narrowing
        np.savez_compressed(os.path.join(GOLD, f"qd_{cfg}.npz"), **out)
        print("qd", cfg, "planes", np.unique(out["drift_pixel_plane"])[:6])


def _pixel_stage(ref, r):
    det = ref.detector
    n = r.shape[0]
    bpg = max(1, -(-n // 128))
    max_radius = int(np.ceil(max(r["tran_diff"]) * 5 / det.PIXEL_PITCH))
    mp = np.array([0])
    ref.pixels_from_track.max_pixels[bpg, 128](r, mp)
    P = (2 * max_radius + 1) * mp[0] + (1 + 2 * max_radius) * max_radius * 2
    active = np.full((n, mp[0]), -1, dtype=np.int32)
    neigh = np.full((n, P), -1, dtype=np.int32)
    nrad = np.full((n, P), -1, dtype=np.int32)
    nlist = np.zeros(n)
    ref.pixels_from_track.get_pixels[bpg, 128](r, active, neigh, nrad, nlist, max_radius)
    starts = np.empty(n)
    tmax = np.array([0])
    ref.detsim.time_intervals[bpg, 128](starts, tmax, r)
    return dict(max_radius=max_radius, max_pixels=int(mp[0]), active=active, neigh=neigh, nrad=nrad,
                n_pixels_list=nlist, track_starts=starts, max_length=int(tmax[0]))


def gen_pixels():
    for cfg, seed in (("module0", 21), ("2x2_no_modvar", 22), ("ndlar", 23)):
        ref = Ref(cfg)
        seg = hand_segments(ref.detector, 64, seed, long_frac=0.35)
        # push a few segments across / beyond the pixel-plane edges so -1 gaps appear
        sb = np.sort(np.asarray(ref.detector.TPC_BORDERS), axis=-1)
        for i in (0, 1, 2):
            p = i % sb.shape[0]
            seg["x_start"][i] = sb[p, 0, 0] + 0.1; seg["x_end"][i] = sb[p, 0, 0] - 0.5 + 0.3 * i
            seg["y_start"][i] = sb[p, 1, 1] - 0.2; seg["y_end"][i] = sb[p, 1, 1] + 0.4
            seg["z_start"][i] = seg["z_end"][i] = 0.5 * (sb[p, 2, 0] + sb[p, 2, 1])
            for ax in "xyz":
                seg[ax][i] = 0.5 * (float(seg[ax + "_start"][i]) + float(seg[ax + "_end"][i]))
        seg["x"][0] = sb[0, 0, 0] + 0.05   # keep midpoints inside so drift assigns a plane
        seg["y"][0] = sb[0, 1, 1] - 0.05
        r = run_quench_drift(ref, to_ref(seg), ref.physics.BIRKS)
        keep = r["pixel_plane"] != ref.detector.DEFAULT_PLANE_INDEX   # reference indexes OOB otherwise
        r = r[keep]
        out = _pixel_stage(ref, r)
        out["segments_in"] = seg[keep]
        np.savez_compressed(os.path.join(GOLD, f"pixels_{cfg}.npz"), **out)
        print("pixels", cfg, "P", out["neigh"].shape, "max_length", out["max_length"])


# --------------------------------------------------------------------------
# pixels_wide: neighbourhoods of radius 1-4 (ring codes 0-8 and -1), the maps and the pixel sums built on them
# --------------------------------------------------------------------------
WIDE_CFGS = (("module0", 71), ("ndlar", 73))
WIDE_RADII = (1, 2, 3, 4)
WIDE_T = 40


def wide_segments(det, seed):
    """16 hand-placed segments in the TPC frame: 0 hugs the low-x edge of the pixel plane, 1 sits in the far corner, 2 hugs the
    low-y edge (second TPC), 3 starts beside 0 and leaves the plane over the low-x edge (its active row gets -1 gaps), 4 lies
    outside every TPC, 5 crosses several pixels (second TPC), 6-15 cluster over a few pixels so that pixels collect many
    tracks at different ring distances."""
    seg = hand_segments(det, 16, seed, plane_choices=[0])
    rng = np.random.default_rng(seed + 7)
    B = np.asarray(det.TPC_BORDERS)
    pitch = det.PIXEL_PITCH
    N0, N1 = int(det.N_PIXELS[0]), int(det.N_PIXELS[1])

    def put(i, p, a, b, zfrac, dz):
        """end points in pixel units (0.5 = centre of pixel 0) of plane p, depth as a fraction of the drift length"""
        z = B[p, 2, 0] + zfrac * (B[p, 2, 1] - B[p, 2, 0])
        seg["x_start"][i], seg["y_start"][i] = B[p, 0, 0] + a[0] * pitch, B[p, 1, 0] + a[1] * pitch
        seg["x_end"][i], seg["y_end"][i] = B[p, 0, 0] + b[0] * pitch, B[p, 1, 0] + b[1] * pitch
        seg["z_start"][i], seg["z_end"][i] = z - 0.5 * dz, z + 0.5 * dz

    put(0, 0, (0.4, 50.5), (0.6, 50.7), 0.5, 0.05)
    put(1, 0, (N0 - 0.3, N1 - 0.4), (N0 - 0.6, N1 - 0.7), 0.3, 0.02)
    put(2, 1, (30.2, 1.3), (31.7, 0.4), 0.6, 0.1)
    put(3, 0, (2.3, 52.6), (-1.4, 53.2), 0.4, 0.2)
    put(4, 0, (20.5, 20.5), (20.9, 20.7), 0.5, 0.05)
    for f in ("x_start", "x_end"):
        seg[f][4] += 500.0
    put(5, 1, (70.2, 140.3), (74.6, 143.8), 0.7, 0.3)
    for i in range(6, 16):
        c = np.array([60.5, 120.5]) + rng.uniform(-1.2, 1.2, 2)
        d = rng.uniform(-0.4, 0.4, 2)
        put(i, 0, c - d, c + d, rng.uniform(0.2, 0.8), rng.uniform(-0.2, 0.2))
    for ax in "xyz":
        seg[ax] = 0.5 * (seg[ax + "_start"].astype(np.float64) + seg[ax + "_end"])
    d = np.stack([seg[ax + "_end"].astype(np.float64) - seg[ax + "_start"] for ax in "xyz"])
    seg["dx"] = np.sqrt((d * d).sum(axis=0))
    seg["dE"] = seg["dEdx"].astype(np.float64) * seg["dx"]
    return seg


def sparse_fields(name, a):
    """A mostly-zero array as {name_shape, name_step, name_val}: the flat indices of its non-zero entries as differences
    (first index, then steps; cumsum restores them) and the values, f4 where that loses nothing (tests/helpers.py dense_field)."""
    flat = np.ascontiguousarray(a).ravel()
    idx = np.flatnonzero(flat)
    val = flat[idx]
    if np.array_equal(val.astype(np.float32).astype(val.dtype), val):
        val = val.astype(np.float32)
    return {name + "_shape": np.array(a.shape, dtype=np.int64), name + "_step": np.diff(idx, prepend=0).astype(np.int64),
            name + "_val": val}


def save_npz_fixed(path, arrays):
    """np.savez_compressed with the members in sorted order and a fixed time stamp: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def _wide_job(args):
    cfg, seed, radius = args
    ref = Ref(cfg)
    det = ref.detector
    seg = wide_segments(det, seed)
    r = run_quench_drift(ref, to_ref(seg), ref.physics.BIRKS)
    n = r.shape[0]
    # the reference indexes TPC_BORDERS[pixel_plane] with the "no plane" value of a segment outside every TPC (IndexError
    # here, an out-of-bounds read on the device): its kernels run on the other rows, and the row of that segment keeps what
    # the driver allocates (-1 ids and codes, 0 pixels; cli/simulate_pixels.py:930-933)
    inside = r["pixel_plane"] != det.DEFAULT_PLANE_INDEX
    assert (~inside).sum() == 1 and not inside[4]
    ri = r[inside]
    ni = ri.shape[0]
    bpg = max(1, -(-ni // 128))
    mp = np.array([0])
    ref.pixels_from_track.max_pixels[bpg, 128](ri, mp)
    nmax = int(mp[0])
    P = (2 * radius + 1) * nmax + (1 + 2 * radius) * radius * 2          # cli/simulate_pixels.py:928
    act_i = np.full((ni, nmax), -1, dtype=np.int32)
    neigh_i = np.full((ni, P), -1, dtype=np.int32)
    nrad_i = np.full((ni, P), -1, dtype=np.int32)
    nlist_i = np.zeros(ni)
    ref.pixels_from_track.get_pixels[bpg, 128](ri, act_i, neigh_i, nrad_i, nlist_i, radius)
    active = np.full((n, nmax), -1, dtype=np.int32); active[inside] = act_i
    neigh = np.full((n, P), -1, dtype=np.int32); neigh[inside] = neigh_i
    nrad = np.full((n, P), -1, dtype=np.int32); nrad[inside] = nrad_i
    nlist = np.zeros(n); nlist[inside] = nlist_i
    # unique pixels and the index map as the driver forms them (cli/simulate_pixels.py:953-956, 1021-1025)
    unique_pix = np.unique(neigh.reshape(-1))
    unique_pix = unique_pix[unique_pix != -1]
    U = unique_pix.shape[0]
    pixel_index_map = np.full(neigh.shape, -1, dtype=np.int64)
    for i_ in range(n):
        compare = neigh[i_, ..., np.newaxis] == unique_pix
        idx = np.where(compare)
        pixel_index_map[i_, idx[0]] = idx[1]
    max_distance = int(nrad.max()) + 1

    def pixel_map(M):
        tpm = np.full((U, M), -1, dtype=np.int64)
        ref.detsim.get_track_pixel_map2[max(1, -(-U // 32)), 32](_PadRows(tpm, 32), _PadVec(unique_pix, 32), neigh, nrad,
                                                                 max_distance)
        return tpm

    # synthetic currents: a multiple of 1/16 below 16 per tick (every sum is exact in f8 whatever the order), starts on the
    # tick grid with one track beginning before tick 0 and one running past the last tick
    rng = np.random.default_rng(1000 * seed + radius)
    NT = len(det.TIME_TICKS)
    signals = (rng.integers(1, 256, size=(n, P, WIDE_T)) / 16.0).astype(np.float32)
    start_ticks = rng.integers(150, NT - 400, size=n)
    start_ticks[6] = -15
    start_ticks[7] = NT - 12
    track_starts = start_ticks * det.TIME_SAMPLING
    assert np.array_equal(np.round(track_starts / det.TIME_SAMPLING), start_ticks)

    def sums(tpm):
        M = tpm.shape[1]
        ps = np.zeros((U, NT)); pts = np.zeros((U, NT, M)); ovf = np.zeros(U)
        ref.detsim.sum_pixel_signals[(n, P, -(-WIDE_T // 64)), (1, 1, 64)](ps, signals, track_starts, pixel_index_map, tpm,
                                                                           pts, ovf)
        return ps, pts, ovf

    M = int(ref.sim.MAX_TRACKS_PER_PIXEL)
    tpm = pixel_map(M)
    # pairs that can take a slot, per unique pixel
    mappable = np.zeros(U, dtype=np.int64)
    np.add.at(mappable, pixel_index_map[(pixel_index_map >= 0) & (nrad >= 0)], 1)
    assert mappable.max() <= M and np.array_equal((tpm >= 0).sum(axis=1), mappable)
    M_low = max(1, int(mappable.max()) // 2)
    tpm_low = pixel_map(M_low)
    # what the fixture is for
    codes = set(np.unique(nrad[neigh >= 0]).tolist())
    if radius == 4:
        assert codes == set(range(-1, 9)), codes
    if radius >= 3:
        assert -1 in codes
        assert ((tpm >= 0).sum(axis=1) == 0).any(), "no unique pixel whose every pair has distance -1"
    else:
        assert -1 not in codes
    assert (mappable > M_low).any(), "the lowered cap overflows on no pixel"
    assert (active[inside] == -1).any() and (active[3] == -1).any()
    out = dict(segments_in=seg, radius=radius, max_pixels=nmax, active=active, neigh=neigh, nrad=nrad, n_pixels_list=nlist,
               unique_pix=unique_pix, pixel_index_map=pixel_index_map.astype(np.int32), track_pixel_map=tpm.astype(np.int32),
               track_pixel_map_low=tpm_low.astype(np.int32), max_tracks_low=M_low, signals_seed=1000 * seed + radius,
               signals_ticks=WIDE_T, start_ticks=start_ticks)
    for tag, m in (("", tpm), ("_low", tpm_low)):
        ps, pts, ovf = sums(m)
        assert ps.min() >= 0 and (ps[:, 0] > 0).any() and (ps[:, NT - 1] > 0).any()      # both ends of the tick axis clip
        out.update(sparse_fields("pixels_signals" + tag, ps))
        out.update(sparse_fields("pixels_tracks_signals" + tag, pts))
        out["overflow" + tag] = ovf.astype(np.int8)
        if tag:
            assert (ovf[mappable > M_low] == 1).all()
    path = os.path.join(GOLD, f"pixels_wide_{cfg}_r{radius}.npz")
    save_npz_fixed(path, out)
    return (cfg, radius, P, int((neigh >= 0).sum()), U, int(((tpm >= 0).sum(axis=1) == 0).sum()), sorted(codes), M_low,
            os.path.getsize(path))


def gen_pixels_wide(jobs):
    """get_pixels at radius 1-4 passed as its argument, unique pixels, index map, get_track_pixel_map2 and sum_pixel_signals
    (synthetic seeded currents; tracks_current is not run) at MAX_TRACKS_PER_PIXEL and at a cap low enough to overflow."""
    with Pool(jobs) as pool:
        for res in pool.map(_wide_job, [(cfg, seed, rad) for cfg, seed in WIDE_CFGS for rad in WIDE_RADII], chunksize=1):
            print("pixels_wide %s radius %d: P %d, %d pairs, %d unique pixels, %d without a slot, codes %s, low cap %d, "
                  "%d bytes" % res)


def _current_job(args):
    cfg, r, neigh, T, itrk, z_only, resp_kind = args
    from larndsim_amd import synth
    ref = Ref(cfg)
    response = synth.make_response(resp_kind, response_sampling=ref.detector.RESPONSE_SAMPLING)
    P = neigh.shape[1]
    sig = np.zeros((1, P, T), dtype=np.float32)
    _State.z_only = z_only
    ref.detsim.tracks_current[(1, P, -(-T // 64)), (1, 1, 64)](sig, neigh[itrk:itrk + 1], r[itrk:itrk + 1], response)
    _State.z_only = None
    return itrk, sig[0]


def gen_chain(jobs):
    """Full chain quench -> ... -> digitize on a handful of segments (all ticks)."""
    from larndsim_amd import synth
    for cfg, seed, nseg in (("module0", 31, 5),):
        ref = Ref(cfg)
        det = ref.detector
        B = np.asarray(det.TPC_BORDERS)
        # one short "track" of 4 consecutive segments sharing pixels + 1 isolated segment
        seg = hand_segments(det, nseg, seed, plane_choices=[0])
        p0 = np.array([B[0, 0, 0] + 12.3, B[0, 1, 0] + 40.7, B[0, 2, 0] + 6.0 * np.sign(B[0, 2, 1] - B[0, 2, 0])])
        d = np.array([0.62, 0.35, 0.70]); d /= np.linalg.norm(d)
        cuts = np.array([0.0, 0.21, 0.47, 0.58, 0.93])
        for i in range(4):
            a, b = p0 + cuts[i] * d, p0 + cuts[i + 1] * d
            seg["x_start"][i], seg["y_start"][i], seg["z_start"][i] = a
            seg["x_end"][i], seg["y_end"][i], seg["z_end"][i] = b
            seg["dx"][i] = cuts[i + 1] - cuts[i]
            seg["dEdx"][i] = 2.0 + 0.3 * i
        for ax in "xyz":
            seg[ax] = 0.5 * (seg[ax + "_start"].astype(np.float64) + seg[ax + "_end"])
        seg["dE"] = seg["dEdx"].astype(np.float64) * seg["dx"]
        r = run_quench_drift(ref, to_ref(seg), ref.physics.BIRKS)
        pix = _pixel_stage(ref, r)
        neigh, nrad, T = pix["neigh"], pix["nrad"], pix["max_length"]
        n = r.shape[0]
        # tracks_current over ALL ticks costs ~20 min per (segment, pixel) in pure Python (64000 rho calls per tick),
        # so the full-tick `signals` of this set come from the oracle (oracle/ldsim_oracle.c), which the `sampled_*`
        # sets pin to the reference's tracks_current; every stage downstream runs the reference's own source.
        try:
            from oracle import oracle as ORC
        except ImportError:      # run as a script: the script directory shadows the package name
            import oracle as ORC
        from larndsim_amd import consts as my_consts
        my_consts.load_snapshot({"module0": "module0"}[cfg])
        for kk in ("RESET_NOISE_CHARGE", "UNCORRELATED_NOISE_CHARGE", "DISCRIMINATOR_NOISE"):
            setattr(my_consts.detector, kk, 0)
        signals = ORC.tracks_current(r, neigh, T, synth.make_response("golden"))
        # spot-check against the reference itself on a few ticks of every segment
        peak_tick = int(np.argmax(np.abs(signals).sum(axis=(0, 1))))
        spot = sorted({3, peak_tick - 7, peak_tick, peak_tick + 5, T - 2})
        with Pool(jobs) as pool:
            res = pool.map(_current_job, [(cfg, r, neigh, T, i, spot, "golden") for i in range(n)])
        for itrk, sref in res:
            np.testing.assert_allclose(signals[itrk][:, spot], sref[:, spot], rtol=3e-7, atol=0)
        unique_pix = np.unique(neigh.ravel())
        unique_pix = unique_pix[unique_pix != -1]
        pixel_index_map = np.full(neigh.shape, -1, dtype=np.int64)
        for i_ in range(n):
            compare = neigh[i_, ..., np.newaxis] == unique_pix
            idx = np.where(compare)
            pixel_index_map[i_, idx[0]] = idx[1]
        M = ref.sim.MAX_TRACKS_PER_PIXEL
        track_pixel_map = np.full((unique_pix.shape[0], M), -1, dtype=np.int64)
        U = unique_pix.shape[0]
        ref.detsim.get_track_pixel_map2[max(1, -(-U // 32)), 32](
            track_pixel_map[:0] if U == 0 else _PadRows(track_pixel_map, 32),
            _PadVec(unique_pix, 32), neigh, nrad, int(nrad.max()) + 1)
        NT = len(det.TIME_TICKS)
        pixels_signals = np.zeros((U, NT))
        pixels_tracks_signals = np.zeros((U, NT, M))
        overflow = np.zeros(U)
        ref.detsim.sum_pixel_signals[(n, neigh.shape[1], -(-T // 64)), (1, 1, 64)](
            pixels_signals, signals, pix["track_starts"], pixel_index_map, track_pixel_map,
            pixels_tracks_signals, overflow)
        A = ref.sim.MAX_ADC_VALUES
        out = dict(segments_in=seg, signals=signals, unique_pix=unique_pix, pixel_index_map=pixel_index_map,
                   track_pixel_map=track_pixel_map, pixels_signals=pixels_signals, overflow=overflow,
                   response_kind="golden", signals_source="oracle (spot-checked against the reference at 5 ticks per segment)", **pix)
        for thr_name, thr in (("default", det.DISCRIMINATION_THRESHOLD * ref.consts.units.e), ("low", 600.0)):
            time_ticks = np.linspace(0, 1 * det.TIME_INTERVAL[1], NT + 1)
            integral = np.zeros((U, A)); ticks = np.zeros((U, A)); frac = np.zeros((U, A, M))
            thresholds = np.full(U, thr)
            ref.fee.get_adc_values[max(1, -(-U // 128)), 128](
                pixels_signals, pixels_tracks_signals, time_ticks, integral, ticks, 0, np.zeros(1), frac, thresholds)
            out[f"adc_integral_{thr_name}"] = integral
            out[f"adc_ticks_{thr_name}"] = ticks
            out[f"adc_fractions_{thr_name}"] = frac
            out[f"adc_digit_{thr_name}"] = ref.fee.digitize(integral)
            out[f"threshold_{thr_name}"] = thr
        np.savez_compressed(os.path.join(GOLD, f"chain_{cfg}.npz"), **out)
        print("chain", cfg, "U", U, "T", T, "hits(default)", int((out["adc_integral_default"] != 0).sum()),
              "hits(low)", int((out["adc_integral_low"] != 0).sum()))


class _PadRows:
    """Lets a launch of ceil(U/32)*32 threads index rows >= U harmlessly (the reference
    kernel has no bounds check because real launches are padded the same way and cupy
    would fault; the serial launcher just needs the extra threads to be no-ops)."""

    def __init__(self, arr, mult):
        self.arr = arr
        self.shape = arr.shape
        self._scratch = np.full((arr.shape[1],), -1, dtype=arr.dtype)

    def __getitem__(self, i):
        return self.arr[i] if i < self.arr.shape[0] else self._scratch


class _PadVec:
    def __init__(self, arr, mult):
        self.arr = arr
        self.shape = arr.shape

    def __getitem__(self, i):
        return self.arr[i] if i < self.arr.shape[0] else -12345


def gen_sampled(jobs):
    """tracks_current at sampled ticks for many diverse (segment, pixel) pairs."""
    sets = (("module0", 41, 10, "golden", ""), ("2x2_no_modvar", 42, 6, "survey", ""), ("ndlar", 43, 6, "golden", ""),
            ("module0", 51, 10, "golden", "corners_"), ("ndlar", 53, 5, "golden", "corners_"))
    only = os.environ.get("GEN_SAMPLED_ONLY")            # e.g. "corners_" to make only the corner sets
    for cfg, seed, nseg, kind, tag in sets:
        if only is not None and tag != only:
            continue
        ref = Ref(cfg)
        seg = corner_segments(ref.detector, nseg, seed) if tag else hand_segments(ref.detector, nseg, seed, long_frac=0.3, steep_frac=0.35)
        if cfg == "2x2_no_modvar":                      # spill-style t0
            seg["t0"] = np.random.default_rng(seed).uniform(0, 10, nseg)
            seg["t0_start"] = seg["t0"]; seg["t0_end"] = seg["t0"]
        r = run_quench_drift(ref, to_ref(seg), ref.physics.BIRKS)
        keep = r["pixel_plane"] != ref.detector.DEFAULT_PLANE_INDEX
        r, seg = r[keep], seg[keep]
        pix = _pixel_stage(ref, r)
        T = pix["max_length"]
        # sampled ticks: a coarse comb + a dense comb where the synthetic response peaks
        K = 1950 if ref.detector.RESPONSE_SAMPLING >= 0.1 else 3800
        peak = int(round((K - 70) * ref.detector.RESPONSE_SAMPLING / ref.detector.TIME_SAMPLING
                         - (ref.detector.TIME_WINDOW - ref.detector.TIME_PADDING) / ref.detector.TIME_SAMPLING))
        ticks = sorted(set(list(range(3, T, 211)) + list(range(max(0, peak - 60), min(T, peak + 50), 4)) + [0, T - 1]))
        if tag:      # a segment along the drift axis costs the pure-Python launcher ~2 minutes per tick: a dozen ticks
            ticks = sorted(set(list(range(3, T, 811)) + list(range(max(0, peak - 48), min(T, peak + 40), 12)) + [0, T - 1]))
        with Pool(jobs) as pool:
            res = pool.map(_current_job, [(cfg, r, pix["neigh"], T, i, ticks, kind) for i in range(r.shape[0])])
        signals = np.zeros((r.shape[0], pix["neigh"].shape[1], len(ticks)), dtype=np.float32)
        for itrk, s in res:
            signals[itrk] = s[:, ticks]
        np.savez_compressed(os.path.join(GOLD, f"sampled_{tag}{cfg}.npz"), segments_in=seg, ticks=np.array(ticks),
                            signals=signals, response_kind=kind, **pix)
        print("sampled", tag + cfg, "pairs", int((pix["neigh"] >= 0).sum()), "ticks", len(ticks),
              "nonzero", int((signals != 0).sum()))


def gen_light():
    from larndsim_amd import synth
    for cfg, seed in (("module0", 51), ("2x2_no_modvar", 52)):
        ref = Ref(cfg)
        light = ref.light
        seg = hand_segments(ref.detector, 40, seed)
        seg["t0"] = np.random.default_rng(seed).uniform(0, 3, 40)
        seg["t0_start"] = seg["t0"]; seg["t0_end"] = seg["t0"]
        r = run_quench_drift(ref, to_ref(seg), ref.physics.BIRKS)
        n = r.shape[0]
        n_prof = 40
        lut = synth.make_lut((14, 26, 8), 48, n_prof, seed)
        n_op = light.N_OP_CHANNEL
        inc = np.zeros((n, n_op), dtype=[('segment_id', 'u4'), ('n_photons_det', 'f4'), ('t0_det', 'f4')])
        # f4 structured outputs: store through f8 mirrors to keep Numba's f64 arithmetic, then narrow
        inc8 = np.zeros((n, n_op), dtype=[('segment_id', 'u4'), ('n_photons_det', 'f8'), ('t0_det', 'f8')])
        lut8 = np.zeros(lut.shape, dtype=[('vis', 'f8'), ('t0', 'f8'), ('t0_avg', 'f8'), ('time_dist', 'f8', (n_prof,))])
        for f in lut.dtype.names:
            lut8[f] = lut[f]
        voxel = np.zeros((n, 3), dtype='i4')
        ref.lightLUT.calculate_light_incidence[max(1, -(-n // 256)), 256](r, lut8, inc8, voxel)
        inc['n_photons_det'] = inc8['n_photons_det']; inc['t0_det'] = inc8['t0_det']
        inc8['n_photons_det'] = inc['n_photons_det']; inc8['t0_det'] = inc['t0_det']     # narrowed values
        n_ticks, t_start = ref.light_sim.get_nticks(inc)
        n_ticks = min(n_ticks, 1200)
        op_channel = light.TPC_TO_OP_CHANNEL[:].ravel()
        n_det = op_channel.shape[0]
        sorted_indices = np.zeros((n_det, n), dtype=np.int32)
        for idet in range(n_det):
            sorted_indices[idet] = np.argsort(inc[:, idet]['n_photons_det'])[::-1]
        out_inc = np.zeros((n_det, n_ticks), dtype='f4')   # like the reference driver: f64 add, f4 store per update
        M = 4
        true_id = np.full((n_det, n_ticks, M), -1, dtype='i8')
        true_ph = np.zeros((n_det, n_ticks, M))
        ref.light_sim.sum_light_signals[(n_det, -(-n_ticks // 64)), (1, 64)](
            r, voxel, np.arange(n, dtype='i8'), inc8, op_channel, lut8, t_start, out_inc, true_id, true_ph,
            sorted_indices, n_prof)
        np.savez_compressed(os.path.join(GOLD, f"light_{cfg}.npz"), segments_in=seg, lut_seed=seed, n_prof=n_prof,
                            n_photons_det=inc['n_photons_det'], t0_det=inc['t0_det'], voxel=voxel,
                            n_ticks=n_ticks, t_start=t_start, light_sample_inc=out_inc, true_id=true_id.astype(np.int32),
                            true_photons=true_ph.astype(np.float32), sorted_indices=sorted_indices, op_channel=op_channel)
        print("light", cfg, "n_op", n_op, "ticks", n_ticks, "smearing", light.ENABLE_LUT_SMEARING,
              "sum", float(out_inc.sum()))


def gen_light_response():
    """light_sim.calc_scintillation_effect (:148-184) and calc_light_detector_response (:303-337) on small arrays.
    Inputs are f8 mirrors holding f4 values (Numba promotes f4 x float to f64, NumPy 2 does not), outputs are f4 so
    that every `+=` rounds like the real kernel's store.  LIGHT_WINDOW is shortened (the functions read it at call
    time) so that the lower bound max(itick - conv_ticks, 0) is exercised without a 9000-tick pure-Python loop."""
    cases = (("module0", 61, dict(LIGHT_WINDOW=(1.0, 1.4), SIPM_RESPONSE_MODEL=0)),
             ("2x2_no_modvar", 62, dict(LIGHT_WINDOW=(0.0, 0.25), SIPM_RESPONSE_MODEL=1, IMPULSE_TICK_SIZE=0.0025)))
    for cfg, seed, over in cases:
        ref = Ref(cfg)
        light, sim = ref.light, ref.sim
        rng = np.random.default_rng(seed)
        D, T, M = 6, 1300, 3
        for k, v in over.items():
            setattr(light, k, v)
        light.LIGHT_GAIN = -np.linspace(1.0, 3.5, light.N_OP_CHANNEL)          # row-indexed by the kernel: make rows differ
        if light.SIPM_RESPONSE_MODEL == 1:
            tt = np.arange(60) * light.IMPULSE_TICK_SIZE
            light.IMPULSE_MODEL = np.exp(-tt / 0.03) * np.sin(tt / 0.02)       # synthetic measured impulse
        conv_ticks = int(np.ceil((light.LIGHT_WINDOW[1] - light.LIGHT_WINDOW[0]) / light.LIGHT_TICK_SIZE))
        assert conv_ticks < T
        # sparse photon arrivals with a dense burst, f4 values
        inc = np.zeros((D, T), dtype='f4')
        hits = rng.random((D, T)) < 0.03
        inc[hits] = rng.uniform(0.5, 400.0, hits.sum()).astype('f4')
        inc[:, 200:230] = rng.uniform(1.0, 50.0, (D, 30)).astype('f4')
        inc[D - 1] = 0                                                          # an empty channel
        tid = np.full((D, T, M), -1, dtype='i8')
        tph = np.zeros((D, T, M))
        for d, t in zip(*np.nonzero(inc)):
            k = int(rng.integers(1, M + 1))
            tid[d, t, :k] = rng.choice(40, size=k, replace=False)
            tph[d, t, :k] = float(inc[d, t]) * rng.dirichlet(np.ones(k))
        grid = ((D, -(-T // 64)), (1, 64))
        scint = np.zeros((D, T), dtype='f4')
        s_tid = np.full((D, T, M), -1, dtype='i8'); s_tph = np.zeros((D, T, M))
        ref.light_sim.calc_scintillation_effect[grid[0], grid[1]](inc.astype('f8'), tid, tph, scint, s_tid, s_tph)
        # the driver feeds the Poisson-fluctuated array here (calc_stat_fluctuations, RNG); any array will do
        disc = np.rint(scint.astype('f8') * 8).astype('f4')
        resp = np.zeros((D, T), dtype='f4')
        r_tid = np.full((D, T, M), -1, dtype='i8'); r_tph = np.zeros((D, T, M))
        ref.light_sim.calc_light_detector_response[grid[0], grid[1]](disc.astype('f8'), s_tid, s_tph, resp, r_tid, r_tph)
        np.savez_compressed(
            os.path.join(GOLD, f"light_response_{cfg}.npz"), light_window=np.array(light.LIGHT_WINDOW),
            sipm_response_model=light.SIPM_RESPONSE_MODEL, impulse_tick_size=light.IMPULSE_TICK_SIZE,
            impulse_model=np.asarray(light.IMPULSE_MODEL, dtype='f8'), light_gain=light.LIGHT_GAIN,
            mc_truth_threshold=sim.MC_TRUTH_THRESHOLD, light_sample_inc=inc, true_id=tid.astype('i4'), true_photons=tph,
            scint=scint, scint_true_id=s_tid.astype('i4'), scint_true_photons=s_tph, disc=disc,
            response=resp, response_true_id=r_tid.astype('i4'), response_true_photons=r_tph)
        print("light_response", cfg, "conv_ticks", conv_ticks, "model", light.SIPM_RESPONSE_MODEL,
              "scint sum", float(scint.sum()), "response sum", float(resp.sum()),
              "truth slots used", int((s_tid >= 0).sum()), int((r_tid >= 0).sum()))


def det_phases(shape, seed):
    """Deterministic stand-in for cp.random.uniform(size=shape): a multiplicative hash of (row, column, seed) in [0, 1).
    tests/helpers.py holds the same formula."""
    shape = tuple(int(v) for v in np.atleast_1d(shape))
    i, k = np.meshgrid(np.arange(shape[0], dtype=np.uint64), np.arange(shape[1], dtype=np.uint64), indexing='ij')
    h = (i * np.uint64(7919) + k * np.uint64(104729) + np.uint64(seed)) * np.uint64(2654435761)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    return h.astype(np.float64) / 4294967296.0


class _GA(np.ndarray):
    """ndarray with cupy's .get()"""
    def get(self):
        return np.asarray(self)


def _ga(a):
    return np.asarray(a).view(_GA)


def gen_light_wvfm():
    """The second half of the light chain on small arrays: calc_stat_fluctuations (light_sim.py:186-238) with the restated
    xoroshiro128p generator supplied as numba.cuda.random (the generator itself is third-party and unpinned; this pins the
    Poisson logic around it), get_triggers (:339-443), gen_light_detector_noise (:445-478) with the uniform phases recorded,
    sim_triggers + digitize_signal (:480-619).  LIGHT_TRIG_WINDOW is shortened where the pure-Python grid walk of
    digitize_signal would otherwise take hours; the functions read it at call time."""
    import ctypes as C
    try:
        from oracle import oracle as O
    except ImportError:
        import oracle as O
    ol = O.lib()
    ol.o_rng_uniform_f32.restype = C.c_float
    ol.o_rng_normal_f32.restype = C.c_float

    def rng_fn(name):
        f = getattr(ol, name)
        return lambda states, i: float(f(C.c_void_p(states.ctypes.data + int(i) * states.dtype.itemsize)))

    cases = (("module0", 71, dict()),
             ("2x2_no_modvar", 72, dict(LIGHT_TRIG_MODE=0, LIGHT_TRIG_WINDOW=(0.2, 0.6))),
             ("2x2_no_modvar", 73, dict(LIGHT_TRIG_WINDOW=(0.1, 0.7))))
    for icase, (cfg, seed, over) in enumerate(cases):
        ref = Ref(cfg)
        light, sim, ls = ref.light, ref.sim, ref.light_sim
        crandom = sys.modules["numba.cuda.random"]
        crandom.xoroshiro128p_uniform_float32 = rng_fn("o_rng_uniform_f32")
        crandom.xoroshiro128p_normal_float32 = rng_fn("o_rng_normal_f32")
        for k, v in over.items():
            setattr(light, k, v)
        rng = np.random.default_rng(seed)
        out = dict(light_trig_mode=light.LIGHT_TRIG_MODE, light_trig_window=np.array(light.LIGHT_TRIG_WINDOW),
                   mc_truth_threshold=sim.MC_TRUTH_THRESHOLD)

        # -- calc_stat_fluctuations: means on both sides of 30, zeros, a negative value
        D0, T0 = 5, 700
        inc = np.zeros((D0, T0), dtype='f4')
        on = rng.random((D0, T0)) < 0.6
        inc[on] = (10 ** rng.uniform(1.0, 5.3, on.sum())).astype('f4')         # PE/us: mean per tick 0.01 .. 200
        inc[0, :5] = (-3.0, 0.0, 29999.0, 30000.0, 30001.0)
        states = O.rng_create_states(D0 * T0, 4242 + icase)
        out["fluct_states_before"] = states.copy().view('u8').reshape(-1, 2)
        disc = np.zeros((D0, T0), dtype='f4')
        ls.calc_stat_fluctuations[(D0, -(-T0 // 64)), (1, 64)](inc.astype('f8'), disc, states)
        out.update(fluct_inc=inc, fluct_disc=disc, fluct_states_after=states.view('u8').reshape(-1, 2))

        # -- a detector response with pulses: get_triggers
        op_channel = light.TPC_TO_OP_CHANNEL[:].ravel()
        nd = op_channel.shape[0]
        digit_ticks = int(np.ceil((light.LIGHT_TRIG_WINDOW[1] + light.LIGHT_TRIG_WINDOW[0]) / light.LIGHT_TICK_SIZE))
        T = 3 * digit_ticks + 1777
        Mt = 2
        resp = np.zeros((nd, T), dtype='f4')        # quiet background except in the pulsed groups: keeps the fixture small
        tid = np.full((nd, T, Mt), -1, dtype='i8'); tph = np.zeros((nd, T, Mt))
        per = light.OP_CHANNEL_PER_TRIG
        thr = np.repeat(np.asarray(light.LIGHT_TRIG_THRESHOLD)[..., None], per, axis=-1).ravel()[op_channel].copy()
        thr = thr.reshape(-1, per)[..., 0]
        groups = rng.choice(nd // per, size=min(6, nd // per), replace=False)
        pulse_at = [137, 137 + digit_ticks + 55, 2 * digit_ticks + 600, 3 * digit_ticks + 1200]
        for g in groups:
            if thr[g] < -1e6:
                continue
            resp[g * per:(g + 1) * per] = rng.normal(0, 2.0, (per, T)).astype('f4')
            for t0 in pulse_at[:int(rng.integers(2, 5))]:
                t0 = t0 + int(rng.integers(0, 40))
                w = int(rng.integers(25, 90))
                amp = thr[g] / per * rng.uniform(1.2, 3.0)
                rows = slice(g * per, (g + 1) * per)
                shape = np.exp(-np.arange(w) / (w / 3.0))
                resp[rows, t0:t0 + w] += (amp * shape).astype('f4')
                for r in range(g * per, (g + 1) * per):
                    for t in range(t0, min(t0 + w, T)):
                        tid[r, t, 0] = 1000 + g
                        tph[r, t, 0] = -float(resp[r, t]) * 0.7
                        if (t + r) % 3 == 0:
                            tid[r, t, 1] = 2000 + g
                            tph[r, t, 1] = -float(resp[r, t]) * 0.3 if t % 5 else 1e-9
        trig, trig_op, trig_type = ls.get_triggers(resp, thr, _ga(op_channel), 0)
        trig2 = ls.get_triggers(resp, thr, _ga(op_channel), 1)
        out.update(response=resp, response_true_id=tid.astype('i4'), response_true_photons=tph, group_threshold=thr,
                   op_channel=op_channel.astype('i4'), trigger_idx=np.asarray(trig), trigger_op_channel_idx=np.asarray(trig_op),
                   trigger_type=np.asarray(trig_type), n_trig_subbatch1=len(trig2[0]))
        print("light_wvfm", cfg, over, "triggers", np.asarray(trig).tolist(), "types", np.asarray(trig_type).tolist())

        # -- gen_light_detector_noise with recorded phases
        nbins = 257
        noise_tab = np.abs(rng.normal(0, 1.0, (light.N_OP_CHANNEL, nbins))) * np.linspace(6000.0, 400.0, nbins)
        rec = []

        def uniform(size=None):
            u = det_phases(size, 100 * seed + len(rec))      # a formula, so the fixture need not store them
            rec.append(u)
            return u
        sys.modules["cupy"].random = types.SimpleNamespace(uniform=uniform)
        for shp in ((4, 1500), (3, 1501)):        # shape[1] < 2 divides by an empty mean in the reference (NaN)
            nz = ls.gen_light_detector_noise(shp, noise_tab[:shp[0]])
            out[f"noise_{shp[1]}"] = nz
            out[f"noise_{shp[1]}_phase_seed"] = 100 * seed + len(rec) - 1
        out["noise_spectrum"] = noise_tab

        # -- sim_triggers: zero spectrum (deterministic), then a real one with recorded phases
        digit_samples = int(np.ceil((light.LIGHT_TRIG_WINDOW[1] + light.LIGHT_TRIG_WINDOW[0]) / light.LIGHT_DIGIT_SAMPLE_SPACING))
        if len(trig) == 0:
            raise RuntimeError("no trigger in the golden case")
        for tag, tab in (("quiet", np.zeros_like(noise_tab)), ("noisy", noise_tab)):
            del rec[:]
            # drop a few rows of the signal so that sim_triggers has to add "missing" channels
            keep = np.ones(nd, bool)
            keep[[1, nd // 2, nd - 1]] = False
            args = [a[keep] for a in (resp, op_channel, tid, tph)]
            dsig, dtid, dtph = ls.sim_triggers(
                (max(len(trig), 1), max(np.asarray(trig_op).shape[1], 1), -(-digit_samples // 64)), (1, 1, 64),
                args[0].copy(), _ga(args[1]), args[2].copy(), args[3].copy(), np.asarray(trig), np.asarray(trig_op),
                digit_samples, tab)
            out[f"wvfm_{tag}"] = dsig
            if tag == "quiet":
                out["wvfm_true_id"] = dtid.astype('i4'); out["wvfm_true_photons"] = dtph
            else:
                out["wvfm_noisy_phase_seeds"] = np.array([100 * seed + i for i in range(len(rec))])
            print("  sim_triggers", tag, dsig.shape, "nonzero", int((dsig != 0).sum()), "truth", int((dtid >= 0).sum()),
                  "noise calls", len(rec))
        out["wvfm_keep_rows"] = keep
        out["digit_samples"] = digit_samples
        np.savez_compressed(os.path.join(GOLD, f"light_wvfm_{cfg}_{icase}.npz"), **out)


# --------------------------------------------------------------------------
# light_wvfm_edges: get_triggers, gen_light_detector_noise and sim_triggers / digitize_signal at constants no shipped
# configuration has (non-integer LIGHT_DIGIT_SAMPLE_SPACING / LIGHT_TICK_SIZE, sample factors 1..128, tiny transforms, ...)
# --------------------------------------------------------------------------
LW_EDGE_MAX_BYTES = 256 * 1024
LW_EDGE_WINDOW = (0.02, 0.05)          # LIGHT_TRIG_WINDOW of most cases: 20 + 50 ticks of 1 ns


def _lw_edge_ref(cfg, over):
    """The reference loaded for `cfg` with the constants of `over` set on its modules (MC_TRUTH_THRESHOLD lives on sim, the
    others on light), cupy's round tapped and cupy's random.uniform replaced by det_phases (seed set through the tap)."""
    ref = Ref(cfg)
    for k, v in over.items():
        setattr(ref.sim if k == "MC_TRUTH_THRESHOLD" else ref.light, k, v)
    cupy = sys.modules["cupy"]
    tap = types.SimpleNamespace(rounded=[], seed=0, calls=0)

    def tapped_round(a, *args, **kw):
        tap.rounded.append(np.array(a, dtype=np.float64, copy=True))
        return np.round(a, *args, **kw)

    def uniform(size=None):
        u = det_phases(size, tap.seed + tap.calls)
        tap.calls += 1
        return u
    cupy.round = tapped_round
    cupy.random = types.SimpleNamespace(uniform=uniform)
    ref.tap = tap
    return ref


def _tie_margin(arrays):
    """smallest distance of any value from a rounding tie (x.5), in units of the rounding step"""
    return min(float(np.abs(a - np.floor(a) - 0.5).min()) for a in arrays)


def _lw_edge_save(case, cfg, over, out):
    """One fixture: the arrays, the configuration's name and the overridden constants as JSON (tests/helpers.py
    load_light_wvfm_edge_case sets them).  Every `reach_*` count must be non-zero: it says the case got where it was sent."""
    out = dict(out)
    for k, v in out.items():
        if k.startswith("reach_"):
            assert int(v) > 0, (case, k)
            out[k] = np.int64(v)
    out["cfg"] = np.array(cfg)
    out["const_json"] = np.array(json.dumps({k: (list(v) if isinstance(v, tuple) else v) for k, v in over.items()},
                                            sort_keys=True))
    path = os.path.join(GOLD, f"light_wvfm_edge_{case}.npz")
    save_npz_fixed(path, out)
    size = os.path.getsize(path)
    assert size < LW_EDGE_MAX_BYTES, (case, size)
    reach = " ".join(f"{k[6:]}={int(v)}" for k, v in sorted(out.items()) if k.startswith("reach_"))
    print(f"light_wvfm_edge {case:22s} {size:7d} bytes  {reach}")


def _gen_lw_edge_triggers():
    """get_triggers (light_sim.py:380-477), LIGHT_TRIG_MODE 0.  module0 cases: rows are channels 0..11 (groups 0 and 1 of
    OP_CHANNEL_PER_TRIG = 6, both of the one module), thresholds handed in."""
    ms = 0.001

    def pulses(T, spec, nd=12, per=6, sigma=0.05, seed=0):
        """f4 [nd][T]: a quiet background and, per (group, first tick, n ticks, value per row), a negative-going pulse"""
        rng = np.random.default_rng(9100 + seed)
        s = rng.normal(0, sigma, (nd, T)).astype('f4') if sigma else np.zeros((nd, T), dtype='f4')
        for g, t0, n, v in spec:
            s[g * per:(g + 1) * per, t0:t0 + n] = np.float32(v)
        return s

    W = LW_EDGE_WINDOW
    base = dict(LIGHT_TRIG_MODE=0, LIGHT_TRIG_WINDOW=W, LIGHT_TICK_SIZE=ms)
    thr0 = [[-50.0, -80.0]]
    cases = []      # (name, cfg, constants, signal, threshold sets, sample factor, check(triggers per set, signal))

    def add(name, over, sig, thr, sf, check, cfg="module0"):
        cases.append((name, cfg, dict(base, **over), sig, np.array(thr, dtype='f8'), sf, check))

    # sf = 1: 136 blocks, three workgroups of 64 with a ragged last one; a pulse in the first and one in the last
    add("trig_sf1", dict(LIGHT_DIGIT_SAMPLE_SPACING=ms), pulses(135, [(0, 3, 3, -20.0), (1, 130, 2, -20.0)], seed=1), thr0, 1,
        lambda t, s: dict(reach_blocks_past_128=int((t[0] >= 128).sum()), reach_triggers=len(t[0])))
    # sf = 7, T a multiple of 7: the reference pads a whole block of zeros; a pulse in the last real block
    add("trig_sf7_allpad", dict(LIGHT_DIGIT_SAMPLE_SPACING=7 * ms), pulses(84, [(1, 0, 7, -20.0), (0, 77, 7, -20.0)], seed=2),
        thr0, 7, lambda t, s: dict(reach_all_padding_block=int(s.shape[1] % 7 == 0), reach_last_block=int((t[0] == 77).sum())))
    add("trig_sf8", dict(LIGHT_DIGIT_SAMPLE_SPACING=8 * ms), pulses(100, [(1, 16, 8, -20.0), (0, 96, 4, -40.0)], seed=3), thr0, 8,
        lambda t, s: dict(reach_triggers=len(t[0]), reach_partial_block=int((t[0] == 96).sum())))
    # sf = 13: 4 real ticks of -24 (group sum) in the last block, 9 ticks of padding: mean -7.4 with the zeros, -24 without;
    # threshold -10.  It must not trigger; the pulse of group 1 shows the case is live.
    add("trig_sf13_tail", dict(LIGHT_DIGIT_SAMPLE_SPACING=13 * ms), pulses(95, [(1, 0, 13, -20.0), (0, 91, 4, -4.0)], seed=4),
        [[-10.0, -80.0]], 13,
        lambda t, s: dict(reach_triggers=int((t[0] == 0).sum()), reach_tail_quiet=int(len(t[0]) == 1),
                          reach_tail_below_unpadded=int(s[:6, 91:].astype('f8').sum(axis=0).mean() < -10.0)))
    add("trig_sf128", dict(LIGHT_DIGIT_SAMPLE_SPACING=128 * ms), pulses(300, [(0, 128, 128, -10.0), (1, 256, 44, -20.0)], seed=5),
        thr0, 128, lambda t, s: dict(reach_triggers=int((t[0] == 128).sum()), reach_tail_quiet=int((t[0] < 256).all())))
    # half-to-even: 2.5 -> 2, 3.5 -> 4.  The first pulse fills one block of the rounded factor with a group sum of -54
    # against -50: blocks of 3 (or of 3 and 5) ticks would hold it diluted to -36 (-36 and -43) and not cross
    add("trig_ratio_2p5", dict(LIGHT_DIGIT_SAMPLE_SPACING=0.0025), pulses(101, [(0, 10, 2, -9.0), (1, 100, 1, -30.0)], seed=6),
        thr0, 2, lambda t, s: dict(reach_triggers=int((t[0] == 10).sum()), reach_last_tick=int((t[0] == 100).sum())))
    add("trig_ratio_3p5", dict(LIGHT_DIGIT_SAMPLE_SPACING=0.0035), pulses(101, [(0, 16, 4, -9.0), (1, 92, 4, -14.0)], seed=7),
        thr0, 4, lambda t, s: dict(reach_triggers=int(list(t[0]) == [16, 92])))
    # a tick that is no power-of-ten fraction: 0.0021 / 0.0007 is 3.0 in f8 (5 * 0.0021 / 0.0007 is not 15: lerp_order)
    add("trig_tick_0p0007", dict(LIGHT_TICK_SIZE=0.0007, LIGHT_DIGIT_SAMPLE_SPACING=0.0021, LIGHT_TRIG_WINDOW=(0.014, 0.035)),
        pulses(100, [(0, 9, 3, -9.0), (1, 99, 1, -50.0)], seed=8), thr0, 3,
        lambda t, s: dict(reach_triggers=int(list(t[0]) == [9, 99])))
    # block mean == threshold: `<` is strict.  Group sums -3, -6, .. -30 over one block of 10: mean -16.5 exactly
    eq = np.zeros((12, 80), dtype='f4')
    eq[:6, 30:40] = -0.5 * np.arange(1, 11, dtype='f4')
    assert eq[:6, 30:40].astype('f8').sum(axis=0).mean() == -16.5
    add("trig_mean_eq_thr", dict(LIGHT_DIGIT_SAMPLE_SPACING=10 * ms), eq, [[-16.5, -80.0], [np.nextafter(-16.5, 0.0), -80.0]], 10,
        lambda t, s: dict(reach_equal_no_trigger=int(len(t[0]) == 0), reach_ulp_trigger=int(list(t[1]) == [30])))
    # f4 group sum in row order: 1e8 + -3 + -1e8 = 0 in f4, -3 in f8; threshold -1
    cancel = pulses(80, [(1, 50, 10, -20.0)], sigma=0)
    cancel[0, 20:30], cancel[1, 20:30], cancel[2, 20:30] = 1e8, -3.0, -1e8
    add("trig_f4_cancel", dict(LIGHT_DIGIT_SAMPLE_SPACING=10 * ms), cancel, [[-1.0, -80.0]], 10,
        lambda t, s: dict(reach_f4_sum_quiet=int(list(t[0]) == [50]),
                          reach_f8_sum_would=int(s[:6, 20:30].astype('f8').sum(axis=0).mean() < -1.0)))
    # five pulses in one module: the third trigger comes out at the reference's absolute-index re-slicing, not at a crossing
    add("trig_three_in_module", dict(LIGHT_DIGIT_SAMPLE_SPACING=10 * ms),
        pulses(700, [(0, 50, 10, -20.0), (0, 200, 10, -20.0), (1, 350, 10, -20.0), (1, 520, 10, -20.0), (1, 640, 10, -20.0)], seed=9),
        thr0, 10, lambda t, s: dict(reach_triggers=int(len(t[0]) >= 3),
                                    reach_off_crossing=int(sum(1 for i in t[0] if s[:, int(i)].min() > -10.0))))
    add("trig_last_tick", dict(LIGHT_DIGIT_SAMPLE_SPACING=2 * ms), pulses(81, [(0, 80, 1, -30.0)], seed=10), thr0, 2,
        lambda t, s: dict(reach_last_tick=int(list(t[0]) == [80])))
    # 2x2, groups of 64 rows: group 1 spans the second half of module 1's rows 0..95 and the first third of module 2's
    g64 = pulses(80, [(1, 32, 16, -100.0)], nd=384, per=64, sigma=0)
    g64[64:128] += np.random.default_rng(9111).normal(0, 0.05, (64, 80)).astype('f4')
    add("trig_2x2_group64", dict(LIGHT_DIGIT_SAMPLE_SPACING=0.016, OP_CHANNEL_PER_TRIG=64), g64, [[-4500.0] * 6], 16,
        lambda t, s: dict(reach_two_modules=int(list(t[0]) == [32, 32])), cfg="2x2_no_modvar")

    for name, cfg, over, sig, thr, sf, check in cases:
        ref = _lw_edge_ref(cfg, over)
        light = ref.light
        assert round(light.LIGHT_DIGIT_SAMPLE_SPACING / light.LIGHT_TICK_SIZE) == sf, (name, sf)
        nd = sig.shape[0]
        op_channel = (light.TPC_TO_OP_CHANNEL[:].ravel() if nd != 12 else np.arange(12)).astype('i4')
        assert op_channel.shape[0] == nd and thr.shape[1] * light.OP_CHANNEL_PER_TRIG == nd
        out = dict(signal=sig, op_channel=op_channel, group_threshold=thr, sample_factor=np.int64(sf))
        trigs = []
        for i, th in enumerate(thr):
            trig, trig_op, trig_type = ref.light_sim.get_triggers(sig.copy(), th.copy(), _ga(op_channel), 0)   # raising fails the run
            trig, trig_op = np.asarray(trig).astype('i8'), np.asarray(trig_op).astype('i4')
            assert len(trig) == 0 or trig_op.shape == (len(trig), 96)
            out[f"trigger_idx_{i}"], out[f"trigger_op_channel_idx_{i}"] = trig, trig_op
            out[f"trigger_type_{i}"] = np.asarray(trig_type).astype('i8')
            trigs.append(trig)
        if name == "trig_2x2_group64":          # modules 1 and 2 fired, with their own channels
            assert np.array_equal(out["trigger_op_channel_idx_0"], np.arange(192).reshape(2, 96))
        out.update(check(trigs, sig))
        _lw_edge_save(name, cfg, over, out)


def _gen_lw_edge_noise():
    """gen_light_detector_noise (light_sim.py:339-377) with det_phases for the uniform numbers, 3 rows each.  The phase seed
    moves on until no value of the inverse transform -- what the reference hands to its round -- lies within 1e-6 LSB of a
    tie: the device's sincos and twiddle rotation (at most 513 terms of up to ~2e4 LSB, error ~1e-9 LSB) cannot cross that."""
    ms = 0.001
    tiny = dict(LIGHT_TICK_SIZE=ms, LIGHT_DET_NOISE_SAMPLE_SPACING=ms)
    cases = (("noise_tiny", tiny, 9, (2, 3, 4, 16, 17), 81),
             ("noise_beyond_table", dict(LIGHT_TICK_SIZE=ms, LIGHT_DET_NOISE_SAMPLE_SPACING=0.004), 5, (64,), 82),
             ("noise_chunk", tiny, 9, (1026, 1027, 1028), 83))
    for name, over, nbins, sizes, seed in cases:
        ref = _lw_edge_ref("module0", over)
        light, tap = ref.light, ref.tap
        rng = np.random.default_rng(seed)
        spectrum = np.abs(rng.normal(0, 1.0, (3, nbins))) * np.linspace(6000.0, 400.0, nbins) + 50.0
        out = dict(noise_spectrum=spectrum, n_samples=np.array(sizes, dtype='i8'))
        seeds, margins = [], []
        noise_freq = np.fft.rfftfreq((nbins - 1) * 2, d=light.LIGHT_DET_NOISE_SAMPLE_SPACING)
        for n in sizes:
            for attempt in range(64):
                tap.seed, tap.calls = 1000 * seed + 64 * len(seeds) + attempt, 0
                del tap.rounded[:]
                nz = ref.light_sim.gen_light_detector_noise((3, n), spectrum)
                assert tap.calls == 1 and len(tap.rounded) == 1
                margin = _tie_margin(tap.rounded)
                if margin >= 1e-6:
                    break
            else:
                raise RuntimeError("no phase seed clear of a rounding tie")
            assert nz.shape == (3, n) and np.isfinite(nz).all() and (nz != 0).any()
            out[f"noise_{n}"] = nz
            seeds.append(tap.seed); margins.append(margin)
            desired = np.fft.rfftfreq(n, d=light.LIGHT_TICK_SIZE)
            exact = int(np.isin(desired, noise_freq).sum())
            out[f"exact_freq_{n}"] = np.int64(exact)
            out[f"beyond_table_{n}"] = np.int64((desired > noise_freq[-1]).sum())
            if name == "noise_tiny" and n in (2, 4, 16):          # every desired frequency is a table frequency, the last included
                assert exact == n // 2 + 1 and desired[-1] == noise_freq[-1]
                out[f"reach_all_exact_{n}"] = exact
            if n % 2:
                assert (nz[:, -1] == 0).all()
                out[f"reach_odd_zero_{n}"] = 1
            if name == "noise_beyond_table":
                out["reach_beyond_table"] = int((desired > noise_freq[-1]).sum() > len(desired) // 2)
            if name == "noise_chunk":
                out[f"reach_terms_{n}"] = (n - n % 2) // 2 - 1       # k = 1 .. N/2 - 1 of the inverse transform
        out["phase_seed"] = np.array(seeds, dtype='i8')
        out["noise_tie_margin"] = np.array(margins)
        print(f"  {name}: n_samples {list(sizes)} noise_tie_margin {['%.3g' % m for m in margins]}")
        _lw_edge_save(name, "module0", over, out)


def _lw_edge_padding(light, T, trig):
    """(front padding, padded length) the way sim_triggers pads (light_sim.py:574-592), for the branch counts only"""
    pre = int(np.ceil(light.LIGHT_TRIG_WINDOW[0] / light.LIGHT_TICK_SIZE))
    post = int(np.ceil(light.LIGHT_TRIG_WINDOW[1] / light.LIGHT_TICK_SIZE))
    n0 = max(pre - int(min(trig)), 0)
    Tp = T + n0
    return n0, Tp + max(post + int(max(trig)) + n0 - Tp, 0)


def _lw_edge_sample_counts(light, Tp, ns):
    """which branch of interp (light_sim.py:256-271) each of the ns sample ticks takes in a waveform of Tp ticks"""
    c = dict(on_tick=0, lerp=0, zero_past_end=0, zero_last_tick=0, off_grid=0)
    for i in range(ns):
        st = i * light.LIGHT_DIGIT_SAMPLE_SPACING / light.LIGHT_TICK_SIZE
        i0 = int(np.floor(st))
        if i0 > Tp - 1:
            c["zero_past_end"] += 1
        elif i0 == st:
            c["on_tick"] += 1
        elif i0 > Tp - 2:
            c["zero_last_tick"] += 1
        else:
            c["lerp"] += 1
        c["off_grid"] += int(st != i * round(light.LIGHT_DIGIT_SAMPLE_SPACING / light.LIGHT_TICK_SIZE, 1))
    return c


def _lw_edge_truth_counts(light, thr, tid, tph, n0, ns):
    """How often the truth walk of digitize_signal (light_sim.py:511-543) takes each of its ways, over the given rows and the
    ns sample ticks; the ticks are those of the padded frame, n0 in front."""
    R, T, Mt = tid.shape
    c = dict(same_slot=0, other_slot=0, no_match=0, below_threshold=0, minus1_end=0, all_full=0, frac_samples=0)
    for i in range(ns):
        st = i * light.LIGHT_DIGIT_SAMPLE_SPACING / light.LIGHT_TICK_SIZE
        t0, t1 = int(np.floor(st)) - n0, int(np.ceil(st)) - n0
        c["frac_samples"] += int(t0 != t1)
        if not 0 <= t0 < T:
            continue
        for r in range(R):
            for j in range(Mt):
                id0 = tid[r, t0, j]
                if id0 == -1:
                    c["minus1_end"] += 1
                    break
                if abs(tph[r, t0, j]) < thr:
                    c["below_threshold"] += 1
                    continue
                if t0 == t1 or not 0 <= t1 < T:
                    continue
                if tid[r, t1, j] == id0:
                    c["same_slot"] += 1
                elif id0 in tid[r, t1]:
                    c["other_slot"] += 1
                else:
                    c["no_match"] += 1
            else:
                c["all_full"] += 1
    return c


def _lw_edge_truth(rng, R, T, Mt):
    """truth slots [R][T][Mt]: 0..Mt ids per tick out of a pool of 5 per row (so the next tick often holds the same id, in the
    same slot or in another), a fifth of the photon numbers below MC_TRUTH_THRESHOLD"""
    tid = np.full((R, T, Mt), -1, dtype='i8')
    tph = np.zeros((R, T, Mt))
    for r in range(R):
        for t in range(T):
            k = int(rng.integers(0, Mt + 1)) if rng.random() < 0.7 else Mt
            tid[r, t, :k] = 100 * r + rng.choice(5, size=k, replace=False)
            tph[r, t, :k] = np.where(rng.random(k) < 0.2, rng.uniform(0.001, 0.09, k), rng.uniform(1.0, 50.0, k))
    return tid, tph


def _gen_lw_edge_digitiser():
    """sim_triggers / digitize_signal (light_sim.py:480-619), module0: the triggers read all 96 channels; the signal holds
    12 of them, in no order, unless noted (the reference appends the other 84 and sorts).  With truth slots every channel id
    must be a row of the padded array and every sample tick's ceil inside it: the pure-Python run raises where the kernel
    guards."""
    rows12 = np.array([50, 3, 95, 20, 7, 48, 33, 77, 10, 60, 47, 90], dtype='i4')
    all96 = np.arange(96, dtype='i4')
    r25 = dict(LIGHT_TICK_SIZE=0.001, LIGHT_DIGIT_SAMPLE_SPACING=0.0025, LIGHT_TRIG_WINDOW=LW_EDGE_WINDOW)

    def run(ref, sig, sop, tid, tph, trig, ns, tab):
        trig = np.array(trig, dtype='i8')
        top = np.stack([all96] * len(trig))
        d, dt, dp = ref.light_sim.sim_triggers((len(trig), 96, -(-ns // 64)), (1, 1, 64), sig.copy(), _ga(sop.copy()), tid.copy(),
                                              tph.copy(), trig, top, ns, tab)          # raising fails the run
        return np.asarray(d), np.asarray(dt), np.asarray(dp)

    def f4_values(rng, shape):
        """f4 numbers of mixed sign and magnitude 1e-3 .. 3e3: v1 - v0 is rarely exact in f4"""
        return (rng.choice([-1.0, 1.0], shape) * 10 ** rng.uniform(-3, 3.5, shape)).astype('f4')

    # -- lerp_2p5 and lerp_order: truth slots at non-integer sample ticks
    for name, over, Mt, T, ns, trig_sets, seed in (
            ("lerp_2p5", dict(r25, LIGHT_NBIT=16), 3, 120, 29, ([5, 60], [30, 60]), 91),
            ("lerp_order", dict(LIGHT_TICK_SIZE=0.0007, LIGHT_DIGIT_SAMPLE_SPACING=0.0021, LIGHT_TRIG_WINDOW=(0.014, 0.035),
                                LIGHT_NBIT=16), 2, 120, 24, ([30, 60],), 92)):
        ref = _lw_edge_ref("module0", over)
        light = ref.light
        rng = np.random.default_rng(seed)
        sig = f4_values(rng, (12, T))
        tid, tph = _lw_edge_truth(rng, 12, T, Mt)
        zero_tab = np.zeros((96, 9))
        out = dict(signal=sig, signal_op_channel=rows12, true_id=tid.astype('i4'), true_photons=tph, digit_samples=np.int64(ns),
                   trigger_sets=np.array(trig_sets, dtype='i8'), mc_truth_threshold=np.float64(ref.sim.MC_TRUTH_THRESHOLD))
        total = {}
        for i, trig in enumerate(trig_sets):
            n0, Tp = _lw_edge_padding(light, T, trig)
            d, dt, dp = run(ref, sig, rows12, tid, tph, trig, ns, zero_tab)
            out[f"wvfm_{i}"], out[f"wvfm_true_id_{i}"], out[f"wvfm_true_photons_{i}"] = d, dt.astype('i4'), dp
            out[f"padded_{i}"] = np.array([n0, Tp], dtype='i8')
            for k, v in {**_lw_edge_truth_counts(light, ref.sim.MC_TRUTH_THRESHOLD, tid, tph, n0, ns),
                         **_lw_edge_sample_counts(light, Tp, ns)}.items():
                total[k] = total.get(k, 0) + v
            assert (dt >= 0).any() and (d != 0).any()
        if name == "lerp_2p5":
            assert out["padded_0"][0] == 15 and out["padded_1"].tolist() == [0, T]        # front padding; none
            keys = ("same_slot", "other_slot", "no_match", "below_threshold", "minus1_end", "all_full", "frac_samples", "lerp")
        else:       # i * S / T falls short of the integer i * 3 for some i (14.999999999999998 at i = 5)
            assert 5 * light.LIGHT_DIGIT_SAMPLE_SPACING / light.LIGHT_TICK_SIZE == 14.999999999999998 and ns > 5
            keys = ("off_grid", "lerp", "same_slot", "other_slot", "no_match")
        out.update({"reach_" + k: total[k] for k in keys})
        _lw_edge_save(name, "module0", over, out)

    def guarded(ref, seed0, fn):
        """fn() (sim_triggers runs with a real spectrum: two noise calls each) under the first pair of phase seeds from seed0 on
        that keeps every value the reference rounds to noise at least 1e-6 LSB from a tie: (result, first seed, margin)"""
        tap = ref.tap
        for attempt in range(64):
            tap.seed = seed0 + 2 * attempt
            del tap.rounded[:]
            res = []
            for r in fn():
                tap.calls = 0
                res.append(r())
                assert tap.calls == 2
            assert len(tap.rounded) == 3 * len(res)                   # two noise calls, then the digitiser's own rounding
            margin = _tie_margin([a for i, a in enumerate(tap.rounded) if i % 3 != 2])
            if margin >= 1e-6:
                return res, tap.seed, margin
        raise RuntimeError("no phase seed clear of a rounding tie")

    # -- beyond_end: no truth slots, sample ticks past the waveform.  Unpadded (120 ticks) the ticks 120, 122.5 and 147.5 all
    # take interp's first zero branch (i0 > len - 1): multiples of 2.5 cannot reach the second (i0 > len - 2) in 120 ticks.
    # Triggers [30, 78] pad to 128 ticks and tick 127.5 takes it; there a real spectrum puts noise on tick 127, so that a
    # lerp in its place would show
    over = dict(r25, LIGHT_NBIT=16, LIGHT_DET_NOISE_SAMPLE_SPACING=0.001)
    ref = _lw_edge_ref("module0", over)
    rng = np.random.default_rng(93)
    T = 120
    sig = f4_values(rng, (12, T))
    no_id, no_ph = np.zeros((12, T, 0), dtype='i8'), np.zeros((12, T, 0))
    tab = np.abs(rng.normal(0, 1.0, (96, 9))) * np.linspace(6000.0, 400.0, 9) + 50.0
    sizes = (49, 50, 60)
    out = dict(signal=sig, signal_op_channel=rows12, digit_samples=np.array(sizes, dtype='i8'),
               trigger_sets=np.array([[30, 60], [30, 78]], dtype='i8'), noise_spectrum=tab, missing_rows=np.int64(84))
    total = {}
    for i, trig in enumerate(out["trigger_sets"]):
        n0, Tp = _lw_edge_padding(ref.light, T, trig)
        assert (n0, Tp) == ((0, 120), (0, 128))[i]
        out[f"padded_{i}"] = np.array([n0, Tp], dtype='i8')
        if i == 0:
            res = [run(ref, sig, rows12, no_id, no_ph, trig, ns, np.zeros((96, 9))) for ns in sizes]
        else:
            res, seed, margin = guarded(ref, 93000, lambda: [(lambda ns=ns: run(ref, sig, rows12, no_id, no_ph, trig, ns, tab))
                                                             for ns in sizes])
            out["phase_seeds"], out["noise_tie_margin"] = np.array([seed, seed + 1], dtype='i8'), np.float64(margin)
            out["noisy_set"] = np.int64(i)
            print(f"  beyond_end: noise_tie_margin {margin:.3g}")
        for ns, (d, dt, dp) in zip(sizes, res):
            assert (ns - 1) * 2.5 == {49: 120.0, 50: 122.5, 60: 147.5}[ns]
            past = int(np.ceil(Tp / 2.5))                               # first sample at or past the end of the waveform
            assert dt.shape[-1] == 0 and (d[:, rows12, :40] != 0).any() and (d[:, :, past:] == 0).all()
            if i == 1 and ns == 60:                                     # tick 127.5: zero between noise on ticks 125 and 127
                assert past == 52 and (d[:, :, 51] == 0).all() and (d[:, :, 50] != 0).mean() > 0.9
            out[f"wvfm_{i}_{ns}"] = d
            for k, v in _lw_edge_sample_counts(ref.light, Tp, ns).items():
                total[k] = total.get(k, 0) + v
    out.update({"reach_" + k: total[k] for k in ("zero_past_end", "zero_last_tick", "lerp", "on_tick")})
    _lw_edge_save("beyond_end", "module0", over, out)

    # -- all_rows_f4 / missing_rows_f4: LIGHT_NBIT = 40 puts the rounding step (2**-24) below what an f4 difference changes.
    # all_rows_f4: 96 f4 rows, nothing padded or appended -- the reference's array would stay f4 and numpy's scalar promotion
    # compute interp all-f4 (neither Numba's typing nor f64), so it is handed the f8 copy: the all-f64 mode.
    # missing_rows_f4: 12 f4 rows handed over as they are; appending the other 84 (:598-604) concatenates f8 noise rows, the
    # array digitize_signal receives is f8 and `v1 - v0` is an f8 difference whatever the mode.
    over = dict(r25, LIGHT_NBIT=40)
    for name, R, sop, seed in (("all_rows_f4", 96, all96, 94), ("missing_rows_f4", 12, rows12, 95)):
        ref = _lw_edge_ref("module0", over)
        rng = np.random.default_rng(seed)
        T, ns, trig = 120, 29, [30, 60]
        sig = f4_values(rng, (R, T))
        assert _lw_edge_padding(ref.light, T, trig) == (0, T)
        d, dt, dp = run(ref, sig.astype('f8') if name == "all_rows_f4" else sig, sop, np.zeros((R, T, 0), dtype='i8'),
                        np.zeros((R, T, 0)), trig, ns, np.zeros((96, 9)))
        c = _lw_edge_sample_counts(ref.light, T, ns)
        # samples where the f4 difference of the two neighbours is not the f8 difference (what option numba_f32 would change)
        i0 = np.array([int(np.floor(i * 2.5)) for i in range(ns) if i % 2])
        v0, v1 = sig[:, i0], sig[:, i0 + 1]
        inexact = int(((v1 - v0).astype('f8') != v1.astype('f8') - v0.astype('f8')).sum())
        out = dict(signal=sig, signal_op_channel=sop, digit_samples=np.int64(ns), trigger_sets=np.array([trig], dtype='i8'),
                   wvfm_0=d, reach_lerp=c["lerp"], reach_f4_difference_inexact=inexact, missing_rows=np.int64(96 - R))
        if R < 96:
            out["reach_missing_rows"] = 96 - R
        _lw_edge_save(name, "module0", over, out)

    # -- noisy_odd: a real spectrum, recorded phases of both noise calls; 115 ticks and triggers [30, 71] pad to 121, an odd
    # length: the inverse transform has 120 samples and the reference appends one zero, which sample 48 (tick 120.0) reads
    over = dict(r25, LIGHT_NBIT=10, LIGHT_DET_NOISE_SAMPLE_SPACING=0.004)
    ref = _lw_edge_ref("module0", over)
    rng = np.random.default_rng(96)
    T, ns, trig = 115, 49, [30, 71]
    n0, Tp = _lw_edge_padding(ref.light, T, trig)
    assert (n0, Tp) == (0, 121) and (ns - 1) * 2.5 == Tp - 1
    sig = f4_values(rng, (12, T))
    nbins = 17
    tab = np.abs(rng.normal(0, 1.0, (96, nbins))) * np.linspace(6000.0, 400.0, nbins) + 50.0
    res, seed, margin = guarded(ref, 96000, lambda: [lambda: run(ref, sig, rows12, np.zeros((12, T, 0), dtype='i8'),
                                                                 np.zeros((12, T, 0)), trig, ns, tab)])
    d = res[0][0]
    assert (d[:, :, ns - 1] == 0).all() and (d[:, :, :ns - 1] != 0).mean() > 0.9
    c = _lw_edge_sample_counts(ref.light, Tp, ns)
    print(f"  noisy_odd: noise_tie_margin {margin:.3g}")
    _lw_edge_save("noisy_odd", "module0", over, dict(
        signal=sig, signal_op_channel=rows12, digit_samples=np.int64(ns), trigger_sets=np.array([trig], dtype='i8'),
        noise_spectrum=tab, phase_seeds=np.array([seed, seed + 1], dtype='i8'), noise_tie_margin=np.float64(margin),
        noisy_set=np.int64(0),
        padded_0=np.array([n0, Tp], dtype='i8'), missing_rows=np.int64(84), wvfm_0=d, reach_lerp=c["lerp"],
        reach_odd_padded_length=Tp % 2, reach_reads_final_tick=int((ns - 1) * 2.5 == Tp - 1)))


def gen_light_wvfm_edges():
    """The reference's get_triggers, gen_light_detector_noise and sim_triggers / digitize_signal with LIGHT_TICK_SIZE,
    LIGHT_DIGIT_SAMPLE_SPACING, LIGHT_NBIT, OP_CHANNEL_PER_TRIG, LIGHT_DET_NOISE_SAMPLE_SPACING and LIGHT_TRIG_WINDOW set to what
    no shipped configuration has: tests/golden/light_wvfm_edge_<case>.npz, each with the overridden constants by name and
    value and `reach_*` counts of the branches the case is there for (asserted non-zero here and again by the tests)."""
    _gen_lw_edge_triggers()
    _gen_lw_edge_noise()
    _gen_lw_edge_digitiser()


# --------------------------------------------------------------------------
# light_edges: lightLUT.calculate_light_incidence, light_sim.get_nticks and light_sim.sum_light_signals where the kernels that
# stand for them are delicate: arrival times on the tick grid, truth-slot rules, voxel faces and clamps, channel slices, LUTs of
# 6 detectors, trigger mode 1, efficiencies that are zero / negative / NaN.  A fixture is a list of runs r0, r1, ...; the inputs
# travel in it in the form the stage reads (records, LUT, efficiencies, op_channel, sorted_indices, track ids).
# --------------------------------------------------------------------------
LE_MAX_BYTES = 256 * 1024
LE_SENT_NPH, LE_SENT_T0, LE_SENT_VOX = 123.0, -7.0, -5          # what the incidence outputs hold before the call
LE_INC8 = [('segment_id', 'u4'), ('n_photons_det', 'f8'), ('t0_det', 'f8')]      # f8 mirrors: Numba's f64 arithmetic
LE_INC4 = [('segment_id', 'u4'), ('n_photons_det', 'f4'), ('t0_det', 'f4')]
LE_REC_FIELDS = ("x", "y", "z", "t0", "n_photons", "pixel_plane")


def _le_ref(cfg, over):
    """The reference loaded for `cfg` with the constants of `over` set by name (MC_TRUTH_THRESHOLD on sim, the others on light;
    a list is an array)."""
    ref = Ref(cfg)
    for k, v in over.items():
        setattr(ref.sim if k == "MC_TRUTH_THRESHOLD" else ref.light, k, np.array(v, dtype=float) if isinstance(v, list) else v)
    return ref


def _le_lut(shape, ndet, n_prof, salt=0):
    """A hand-made LUT whose every value is dyadic: vis and time_dist powers of two, t0 and t0_avg whole nanoseconds; every
    voxel and detector differs from its neighbours."""
    nx, ny, nz = shape
    lut = np.zeros((nx, ny, nz, ndet), dtype=[('vis', 'f4'), ('t0', 'f4'), ('t0_avg', 'f4'), ('time_dist', 'f4', (n_prof,))])
    i, j, k, d = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), np.arange(ndet), indexing='ij')
    h = i * 5 + j * 3 + k * 7 + d + salt
    lut['vis'] = 2.0 ** -(1 + h % 4)
    lut['t0'] = (h * 3) % 5
    lut['t0_avg'] = (h * 7) % 12
    lut['time_dist'] = 2.0 ** -(1 + (h[..., None] + np.arange(n_prof)) % 4)
    return lut


def _le_lut8(lut):
    n_prof = lut['time_dist'].shape[-1]
    lut8 = np.zeros(lut.shape, dtype=[('vis', 'f8'), ('t0', 'f8'), ('t0_avg', 'f8'), ('time_dist', 'f8', (n_prof,))])
    for f in lut.dtype.names:
        lut8[f] = lut[f]
    return lut8


def _le_records(n):
    return np.zeros(n, dtype=REF_DTYPE)


def _le_inside(det, itpc, m, n):
    """a point well inside TPC `itpc`, different for every m of n"""
    b = det.TPC_BORDERS[itpc]
    u = np.array([((m * 7 + 3) % n + 0.37) / n, ((m * 11 + 1) % n + 0.61) / n, ((m * 5 + 2) % n + 0.23) / n])
    return [float(f4(b[a][0] + (b[a][1] - b[a][0]) * (0.05 + 0.9 * u[a]))) for a in range(3)]


def _le_incidence(ref, rec, lut, n_out):
    """The reference's calculate_light_incidence into arrays that hold the sentinels: (n_photons_det f4, t0_det f4, voxel i4)"""
    n = len(rec)
    inc8 = np.zeros((n, n_out), dtype=LE_INC8)
    inc8['n_photons_det'] = LE_SENT_NPH
    inc8['t0_det'] = LE_SENT_T0
    voxel = np.full((n, 3), LE_SENT_VOX, dtype='i4')
    with np.errstate(invalid='ignore'):
        ref.lightLUT.calculate_light_incidence[max(1, -(-n // 256)), 256](rec, _le_lut8(lut), inc8, voxel)
    return inc8['n_photons_det'].astype('f4'), inc8['t0_det'].astype('f4'), voxel


def _le_nticks(ref, nph, t0d):
    inc = np.zeros(nph.shape, dtype=LE_INC4)
    inc['n_photons_det'] = nph
    inc['t0_det'] = t0d
    n_ticks, start = ref.light_sim.get_nticks(inc)
    return int(n_ticks), float(start)          # (Numba types the scalar argument f64)


def _le_voxel_unclamped(ref, rec, shape):
    """get_voxel's three indices before the clamp and its fractions times n (lightLUT.py:39-57) for the records inside a TPC:
    (rows, int indices [m, 3], fractions [m, 3])"""
    rows, idx, fr = [], [], []
    for m, r in enumerate(rec):
        itpc = int(r['pixel_plane'])
        if itpc == ref.detector.DEFAULT_PLANE_INDEX:
            continue
        b = ref.detector.TPC_BORDERS[itpc]
        is_even = b[2][1] > b[2][0]
        x_min, x_max = b[0][0] - 2e-2, b[0][1] + 2e-2
        y_min, y_max = b[1][0] - 2e-2, b[1][1] + 2e-2
        z_min, z_max = b[2][0] - 2e-2, b[2][1] + 2e-2
        f = [(r['x'] - x_min) / (x_max - x_min) * shape[0] if is_even else (x_max - r['x']) / (x_max - x_min) * shape[0],
             (y_max - r['y']) / (y_max - y_min) * shape[1], (r['z'] - z_min) / (z_max - z_min) * shape[2]]
        rows.append(m); idx.append([int(v) for v in f]); fr.append(f)
    return np.array(rows), np.array(idx).reshape(-1, 3), np.array(fr).reshape(-1, 3)


def _le_save(case, cfg, over, out, bounds=None):
    """One fixture: arrays, configuration name, overridden constants as JSON.  Every `reach_*` count is non-zero, or at least the
    bound given for it."""
    out = dict(out)
    bounds = bounds or {}
    for k, v in out.items():
        if k.startswith("reach_"):
            assert int(v) >= bounds.get(k, 1), (case, k, int(v))
            out[k] = np.int64(v)
    out["cfg"] = np.array(cfg)
    out["const_json"] = np.array(json.dumps({k: (list(v) if isinstance(v, tuple) else v) for k, v in over.items()}, sort_keys=True))
    path = os.path.join(GOLD, f"light_edge_{case}.npz")
    save_npz_fixed(path, out)
    size = os.path.getsize(path)
    assert size < LE_MAX_BYTES, (case, size)
    reach = " ".join(f"{k[6:]}={int(v)}" for k, v in sorted(out.items()) if k.startswith("reach_"))
    print(f"light_edge {case:24s} {size:7d} bytes  {reach}")


def _le_put_records(out, pre, rec):
    for f in LE_REC_FIELDS:
        out[pre + f] = rec[f].copy()


def _le_put_lut(out, pre, lut):
    for f in lut.dtype.names:
        out[pre + "lut_" + f] = np.ascontiguousarray(lut[f])


def _le_incidence_run(ref, out, k, rec, lut, n_out, lut_key=None):
    """run k of an incidence fixture: records, LUT (or the key of a LUT stored once), output width, what the reference wrote and
    get_nticks of it.  Returns (n_photons_det, t0_det, voxel)."""
    assert len(rec) <= 64
    pre = f"r{k}_"
    nph, t0d, vox = _le_incidence(ref, rec, lut, n_out)
    _le_put_records(out, pre, rec)
    if lut_key is None:
        _le_put_lut(out, pre, lut)
    else:
        out[pre + "lut"] = np.array(lut_key)
    n_ticks, start = _le_nticks(ref, nph, t0d)
    out.update({pre + "n_out": np.int64(n_out), pre + "n_photons_det": nph, pre + "t0_det": t0d, pre + "voxel": vox,
                pre + "n_ticks": np.int64(n_ticks), pre + "start_time": np.float64(start)})
    out["n_runs"] = np.int64(k + 1)
    return nph, t0d, vox


def _le_face_points(b, a, n):
    """coordinates on axis a of a TPC with borders b for a LUT of n voxels along it: both borders, border -+ 1.9e-2 (inside
    get_voxel's 2e-2 margin), every interior voxel face min + k (max - min) / n in f64 with its two neighbours, and a point a
    voxel and a half beyond either end (clamped)"""
    lo, hi = b[a][0] - 2e-2, b[a][1] + 2e-2
    pts = [b[a][0], b[a][1], b[a][0] - 1.9e-2, b[a][0] + 1.9e-2, b[a][1] - 1.9e-2, b[a][1] + 1.9e-2,
           lo - 1.5 * (hi - lo) / n, hi + 1.5 * (hi - lo) / n]
    for k in range(1, n):
        face = lo + k * (hi - lo) / n
        pts += [face, np.nextafter(face, -np.inf), np.nextafter(face, np.inf)]
    return [float(p) for p in pts]


def _gen_le_faces(case, cfg, tpcs):
    ref = _le_ref(cfg, {})
    det = ref.detector
    n_out = ref.light.N_OP_CHANNEL
    out = {}
    reach = {f"reach_clamped_{s}_{ax}": 0 for s in ("low", "high") for ax in "xyz"}
    reach.update(reach_on_face=0, reach_untouched=0)
    k = 0
    for si, shape in enumerate(((1, 1, 1), (3, 5, 2), (14, 26, 8))):
        lut = _le_lut(shape, 4, 1, salt=si)
        _le_put_lut(out, f"s{si}_", lut)
        for itpc in tpcs:
            b = det.TPC_BORDERS[itpc]
            pts = [_le_face_points(b, a, shape[a]) for a in range(3)]
            total = max(len(p) for p in pts)
            for c0 in range(0, total, 60):
                ms = list(range(c0, min(c0 + 60, total)))
                rec = _le_records(len(ms) + 2)
                for q, m in enumerate(ms):
                    rec['x'][q], rec['y'][q], rec['z'][q] = (pts[a][m % len(pts[a])] for a in range(3))
                    rec['pixel_plane'][q] = itpc
                # two segments outside every TPC, at positions inside this one
                for q in (len(ms), len(ms) + 1):
                    rec['x'][q], rec['y'][q], rec['z'][q] = _le_inside(det, itpc, q, 64)
                    rec['pixel_plane'][q] = det.DEFAULT_PLANE_INDEX
                rec[[3, len(ms)]] = rec[[len(ms), 3]]           # (one of them inside the tile, not at its end)
                rec['n_photons'] = f4(1000.5 + 3 * np.arange(len(rec)))
                rec['t0'] = f4(0.25 + np.arange(len(rec)) / 64)
                nph, t0d, vox = _le_incidence_run(ref, out, k, rec, lut, n_out, lut_key=f"s{si}_")
                k += 1
                rows, idx, fr = _le_voxel_unclamped(ref, rec, shape)
                for a, ax in enumerate("xyz"):
                    reach[f"reach_clamped_low_{ax}"] += int((idx[:, a] < 0).sum())
                    reach[f"reach_clamped_high_{ax}"] += int((idx[:, a] > shape[a] - 1).sum())
                    inner = (fr[:, a] > 0.5) & (fr[:, a] < shape[a] - 0.5)
                    reach["reach_on_face"] += int((inner & (fr[:, a] == np.floor(fr[:, a]))).sum())
                reach["reach_untouched"] += int(((vox == LE_SENT_VOX).all(axis=1) & (nph == LE_SENT_NPH).all(axis=1) &
                                                 (t0d == LE_SENT_T0).all(axis=1)).sum())
    out.update(reach)
    _le_save(case, cfg, {}, out)


def _le_plain_records(ref, tpcs, n, n_default=1):
    """n records at interior points of the TPCs in turn, the last n_default of them outside every TPC"""
    det = ref.detector
    rec = _le_records(n)
    for m in range(n):
        itpc = tpcs[m % len(tpcs)]
        rec['x'][m], rec['y'][m], rec['z'][m] = _le_inside(det, itpc, m, n)
        rec['pixel_plane'][m] = itpc if m < n - n_default else det.DEFAULT_PLANE_INDEX
    rec['n_photons'] = f4(200.25 + 17 * np.arange(n))
    rec['t0'] = f4(0.125 + np.arange(n) / 32)
    return rec


def _gen_le_incidence_cases():
    _gen_le_faces("faces_module0", "module0", (0, 1))
    _gen_le_faces("faces_2x2", "2x2_no_modvar", (1, 4))

    # a LUT of 6 detectors (lut_index = o % 6; not a multiple of 4: the one-channel kernel) and its twin of 48
    ref = _le_ref("module0", {})
    rec = _le_plain_records(ref, (0, 1), 21)
    out = {}
    for k, ndet in enumerate((6, 48)):
        nph, _, _ = _le_incidence_run(ref, out, k, rec, _le_lut((3, 5, 2), ndet, 1, salt=2), ref.light.N_OP_CHANNEL)
        out[f"reach_lit_{ndet}"] = int(((nph > 0) & (nph != LE_SENT_NPH)).sum())
    _le_save("lut_6_detectors", "module0", {}, out)

    # one module's slice of the channels: the tables' offset follows the segment's module (lightLUT.py:120-123)
    ref = _le_ref("2x2_no_modvar", {})
    n_out = ref.light.N_OP_CHANNEL // 4
    rec = _le_plain_records(ref, (0, 1, 2, 5, 7), 26)
    out = {}
    nph, _, _ = _le_incidence_run(ref, out, 0, rec, _le_lut((3, 5, 2), 48, 1, salt=3), n_out)
    mods = np.unique(rec['pixel_plane'][rec['pixel_plane'] != ref.detector.DEFAULT_PLANE_INDEX] // 2)
    out["reach_modules"] = len(mods)
    out["reach_lit"] = int(((nph > 0) & (nph != LE_SENT_NPH)).sum())
    assert len(mods) == 4 and n_out < ref.light.N_OP_CHANNEL
    _le_save("module_slice_2x2", "2x2_no_modvar", {}, out, bounds=dict(reach_modules=4))

    # trigger mode 1: t0_det is not written, get_nticks returns the fixed window
    over = dict(LIGHT_TRIG_MODE=1)
    ref = _le_ref("module0", over)
    rec = _le_plain_records(ref, (0, 1), 19)
    out = {}
    nph, t0d, _ = _le_incidence_run(ref, out, 0, rec, _le_lut((3, 5, 2), 48, 1, salt=4), ref.light.N_OP_CHANNEL)
    assert (t0d == LE_SENT_T0).all()
    lw = ref.light.LIGHT_WINDOW
    assert int(out["r0_n_ticks"]) == int((lw[1] + lw[0]) / ref.light.LIGHT_TICK_SIZE) and float(out["r0_start_time"]) == 0.0
    out["reach_t0_untouched"] = int((t0d == LE_SENT_T0).sum())
    out["reach_lit"] = int(((nph > 0) & (nph != LE_SENT_NPH)).sum())
    _le_save("trig_mode_1", "module0", over, out)

    # efficiencies that are zero, negative and NaN: the reference writes NaN and -0.0 into the channels of other TPCs
    ref = _le_ref("module0", {})
    eff = np.asarray(ref.light.OP_CHANNEL_EFFICIENCY, dtype=float).copy()
    eff[[2, 49]] = 0.0
    eff[[4, 50]] = -0.25
    eff[[9, 60]] = np.nan
    over = dict(OP_CHANNEL_EFFICIENCY=[float(v) for v in eff])
    ref = _le_ref("module0", over)
    rec = _le_plain_records(ref, (0, 1), 23)
    rec['n_photons'][5] = 0.0
    out = {}
    nph, _, _ = _le_incidence_run(ref, out, 0, rec, _le_lut((3, 5, 2), 48, 1, salt=5), ref.light.N_OP_CHANNEL)
    out["reach_nan"] = int(np.isnan(nph).sum())
    out["reach_negative_zero"] = int(((nph == 0) & np.signbit(nph)).sum())
    out["reach_negative"] = int((nph < 0).sum())
    _le_save("efficiency_fallback", "module0", over, out)

    # no light: records without photons and voxels without visibility
    ref = _le_ref("module0", {})
    rec = _le_plain_records(ref, (0, 1), 22)
    rec['n_photons'][::3] = 0.0
    lut = _le_lut((3, 5, 2), 48, 1, salt=6)
    lut['vis'][1] = 0.0
    lut['vis'][:, :, :, ::5] = 0.0
    out = {}
    nph, _, vox = _le_incidence_run(ref, out, 0, rec, lut, ref.light.N_OP_CHANNEL)
    out["reach_no_photons"] = int((rec['n_photons'] == 0).sum())
    out["reach_dark_voxel"] = int((vox[:, 0] == 1).sum())
    out["reach_lit"] = int(((nph > 0) & (nph != LE_SENT_NPH)).sum())
    # ... and a run in which nothing is lit at all: get_nticks falls back to the fixed window
    rec2 = rec[rec['pixel_plane'] != ref.detector.DEFAULT_PLANE_INDEX].copy()
    rec2['n_photons'] = 0.0
    nph2, _, _ = _le_incidence_run(ref, out, 1, rec2, lut, ref.light.N_OP_CHANNEL)
    assert not (nph2 > 0).any() and float(out["r1_start_time"]) == 0.0
    _le_save("dark", "module0", {}, out)


# ---- photon sum ------------------------------------------------------------------------------------------------------------------------
LE_SUM_CHANNELS = (0, 1, 5, 47, 48, 50, 95, 7)          # detector rows of the photon-sum cases: both TPCs of module0, not in order


def _le_dyadic_eff(n):
    return [float(2.0 ** -(1 + c % 2)) for c in range(n)]


def _le_sum_records(ref, t0):
    """one record per entry of t0, alternating TPCs, distinct odd photon counts: with dyadic efficiencies and visibilities no two
    records give a detector the same photons"""
    n = len(t0)
    assert n <= 32
    rec = _le_records(n)
    for m in range(n):
        itpc = m % 2
        rec['x'][m], rec['y'][m], rec['z'][m] = _le_inside(ref.detector, itpc, m, n)
        rec['pixel_plane'][m] = itpc
    rec['n_photons'] = 2 * ((np.arange(n) * 5) % n) + 1
    rec['t0'] = t0
    return rec


def _le_deposits(ref, rec, nph, vox, lut, op_channel, order, start, n_ticks):
    """Every arrival of the photon sum by the reference's own expressions (light_sim.py:81-82, 90-93, 101-103, 116-121), in visiting
    order: rows (idet, visit rank, itrk, bin, arrival time, photons, ticks that admit it, ticks that would but for the pre-filter)
    and the deposits (idet, itick, visit rank, itrk, bin, photons)."""
    light, units = ref.light, ref.consts.units
    tick = light.LIGHT_TICK_SIZE
    n_prof = lut['time_dist'].shape[-1]
    st = np.arange(n_ticks) * tick + start
    en = st + tick
    lut8 = _le_lut8(lut)
    arrivals, deposits = [], []
    for idet, ch in enumerate(op_channel):
        for q, itrk in enumerate(order[idet]):
            ph = float(nph[itrk, ch])
            if not ph > 0:
                continue
            tt = float(rec['t0'][itrk])
            te = tt + n_prof * units.ns / units.mus
            keep = ~((te < st) | (tt > en))
            cell = lut8[vox[itrk, 0], vox[itrk, 1], vox[itrk, 2], ch % lut.shape[3]]
            if light.ENABLE_LUT_SMEARING:
                bins = [(ip, tt + ip * units.ns / units.mus, ph * float(cell['time_dist'][ip]) / tick) for ip in range(n_prof)]
            else:
                bins = [(0, tt + float(cell['t0_avg']) * units.ns / units.mus, ph / tick)]
            for ip, pt, photons in bins:
                inwin = (pt < en) & (pt > st)
                hit = np.flatnonzero(inwin & keep)
                arrivals.append((idet, q, itrk, ip, pt, photons, len(hit), int((inwin & ~keep).sum())))
                deposits += [(idet, int(it), q, itrk, ip, photons) for it in hit]
    return arrivals, deposits, st, en


def _le_sum_run(ref, rec, vox, track_id, nph, op_channel, lut, start, n_ticks, M, order, init=None, out_dtype='f4'):
    """The reference's sum_light_signals into zero / -1 arrays, or into copies of `init`: (light_sample_inc, ids i8, photons f8)"""
    n_det = len(op_channel)
    n_prof = lut['time_dist'].shape[-1]
    inc8 = np.zeros(nph.shape, dtype=LE_INC8)
    inc8['n_photons_det'] = nph
    if init is None:
        out = np.zeros((n_det, n_ticks), dtype=out_dtype)
        tid = np.full((n_det, n_ticks, M), -1, dtype='i8')
        tph = np.zeros((n_det, n_ticks, M))
    else:
        out, tid, tph = init[0].astype(out_dtype), init[1].copy(), init[2].copy()
    ref.light_sim.sum_light_signals[(n_det, -(-n_ticks // 64)), (1, 64)](
        rec, vox, track_id, inc8, op_channel, _le_lut8(lut), float(start), out, tid, tph, order, n_prof)
    return out, tid, tph


def _le_descending(nph, op_channel):
    """visiting order of the driver and of the resident sum: descending photons per detector, ties by descending index"""
    return np.ascontiguousarray(np.stack([np.argsort(nph[:, c], kind="stable")[::-1] for c in op_channel]), dtype=np.int32)


def _le_sum_fixture(case, over, rec, lut, track_id, runs, order=None, bounds=None, extra=None, want_resident=None):
    """One photon-sum fixture of module0.  runs: dicts (start: None = get_nticks' own, n_ticks, max_truth, init: None or a
    function of (deposits, n_det, n_ticks, M) that returns the arrays the sum adds into).  Returns what extra() needs."""
    ref = _le_ref("module0", over)
    op_channel = np.array(LE_SUM_CHANNELS, dtype=np.int32)
    n_out = ref.light.N_OP_CHANNEL
    nph, t0d, vox = _le_incidence(ref, rec, lut, n_out)
    assert not (vox == LE_SENT_VOX).any()
    own_ticks, own_start = _le_nticks(ref, nph, t0d)
    descending = _le_descending(nph, op_channel)
    order = descending if order is None else np.ascontiguousarray(order, dtype=np.int32)
    no_ties = all(len(np.unique(nph[:, c][nph[:, c] > 0])) == (nph[:, c] > 0).sum() for c in op_channel)
    out = {}
    _le_put_records(out, "", rec)
    _le_put_lut(out, "", lut)
    out.update(op_channel=op_channel, sorted_indices=order, track_id=np.asarray(track_id, dtype='i8'), n_photons_det=nph,
               t0_det=t0d, voxel=vox, n_prof=np.int64(lut['time_dist'].shape[-1]), own_start_time=np.float64(own_start),
               own_n_ticks=np.int64(own_ticks), n_runs=np.int64(len(runs)))
    reach = {}
    for k, run in enumerate(runs):
        start = own_start if run.get("start") is None else float(run["start"])
        n_ticks, M = int(run["n_ticks"]), int(run["max_truth"])
        arrivals, deposits, st, en = _le_deposits(ref, rec, nph, vox, lut, op_channel, order, start, n_ticks)
        init = run["init"](ref, deposits, track_id, len(op_channel), n_ticks, M) if run.get("init") else None
        res = _le_sum_run(ref, rec, vox, track_id, nph, op_channel, lut, start, n_ticks, M, order, init)
        # dyadic inputs: the same sum with an f8 array gives the same values, so no f4 addition rounded (24 bits held everything)
        res8 = _le_sum_run(ref, rec, vox, track_id, nph, op_channel, lut, start, n_ticks, M, order, init, out_dtype='f8')
        assert np.array_equal(res[0].astype('f8'), res8[0]) and np.array_equal(res[2], res8[2]), (case, k, "a sum left 24 bits")
        for _, _, _, _, _, photons, _, _ in arrivals:
            assert photons == float(np.float32(photons)), (case, photons)
        # every deposit the expressions admit is in the sum, and nothing else (the arrays a test compares are the reference's own)
        cells = np.zeros((len(op_channel), n_ticks))
        for idet, it, _, _, _, photons in deposits:
            cells[idet, it] += photons
        assert np.array_equal(cells + (0 if init is None else init[0].astype('f8')), res8[0]), (case, k)
        pre = f"r{k}_"
        out.update({pre + "start_time": np.float64(start), pre + "n_ticks": np.int64(n_ticks), pre + "max_truth": np.int64(M),
                    pre + "light_sample_inc": res[0], pre + "true_id": res[1], pre + "true_photons": res[2],
                    pre + "has_init": np.int64(init is not None)})
        if init is not None:
            out.update({pre + "init_inc": init[0], pre + "init_true_id": init[1], pre + "init_true_photons": init[2]})
        if k == 0:
            resident = int(run.get("start") is None and init is None and no_ties and np.array_equal(order, descending))
            out["resident"] = np.int64(resident)
            assert want_resident is None or resident == want_resident, (case, resident)
        arr = np.array([(a[6], a[7], a[4]) for a in arrivals], dtype=float).reshape(-1, 3)
        on_axis = (arr[:, 2] > st[0]) & (arr[:, 2] < en[-1])
        per_pair = {}
        for a in arrivals:
            per_pair[(a[0], a[2])] = per_pair.get((a[0], a[2]), 0) + a[6]
        r = dict(two_ticks=int((arr[:, 0] == 2).sum()), one_tick=int((arr[:, 0] == 1).sum()),
                 no_tick=int(((arr[:, 0] == 0) & (arr[:, 1] == 0) & on_axis).sum()), prefiltered=int((arr[:, 1] > 0).sum()),
                 before_axis=int((arr[:, 2] <= st[0]).sum()), past_axis=int((arr[:, 2] >= en[-1]).sum()),
                 records_per_pair_max=max(per_pair.values()) if per_pair else 0)
        assert (arr[:, 0] <= 2).all() and r["records_per_pair_max"] <= lut['time_dist'].shape[-1] + 2, (case, k, r)
        out[pre + "records_per_pair_max"] = np.int64(r["records_per_pair_max"])
        for name, v in r.items():
            reach[name] = reach.get(name, 0) + v if name != "records_per_pair_max" else max(reach.get(name, 0), v)
        if extra:
            for name, v in extra(ref, run, k, arrivals, deposits, init, res, st, en).items():
                reach[name] = reach.get(name, 0) + v
    wanted = set(bounds or {}) | {"records_per_pair_max"}
    out.update({"reach_" + name: v for name, v in reach.items() if name in wanted})
    _le_save(case, "module0", over, out, bounds={"reach_" + k: v for k, v in (bounds or {}).items()})


def _le_cells(deposits, thr):
    """deposits above the truth threshold per (idet, itick) cell, in the reference's visiting order (rank, then bin)"""
    cells = {}
    for idet, it, q, itrk, ip, photons in sorted(deposits, key=lambda d: (d[0], d[1], d[2], d[4])):
        if photons > thr:
            cells.setdefault((idet, it), []).append((itrk, photons))
    return cells


def _gen_le_sum_cases():
    n_prof = 16
    base = dict(LIGHT_TICK_SIZE=0.001, OP_CHANNEL_EFFICIENCY=_le_dyadic_eff(96))
    lut = _le_lut((2, 3, 2), 48, n_prof, salt=1)

    # on-grid times under LUT smearing: start_time = -1.0 from get_nticks itself, t0 = k / 1000 in f64
    over = dict(base, ENABLE_LUT_SMEARING=True)
    k_grid = [0] + [(m * 482) // 31 for m in range(1, 32)]
    rec = _le_sum_records(_le_ref("module0", over), np.array(k_grid) / 1000)
    lut_g = lut.copy()
    lut_g['t0'][tuple(_le_incidence(_le_ref("module0", over), rec[:1], lut, 96)[2][0])] = 0     # record 0 sees t0_det = 0
    ids = np.arange(len(rec)) // 2 * 3 + 1
    grid_bounds = dict(two_ticks=8, no_tick=8, one_tick=8)
    _le_sum_fixture("grid_smear", over, rec, lut_g, ids, [dict(n_ticks=1536, max_truth=2)], bounds=grid_bounds, want_resident=1)
    out = np.load(os.path.join(GOLD, "light_edge_grid_smear.npz"))
    assert float(out["r0_start_time"]) == -1.0 and int(out["own_n_ticks"]) > 1536

    # the same records from start times get_nticks would not give
    starts = (-0.75, 0.0, float(np.float32(-0.9)))
    _le_sum_fixture("grid_smear_free_start", over, rec, lut_g, ids, [dict(start=s, n_ticks=1536, max_truth=2) for s in starts],
                    bounds=dict(one_tick=8, no_tick=8, two_ticks=1), want_resident=0)

    # without smearing: one arrival per pair at t0 + t0_avg (whole ns); one t0_avg beyond the profile length is pre-filtered
    over_ns = dict(base, ENABLE_LUT_SMEARING=False)
    ref = _le_ref("module0", over_ns)
    lut_n = lut_g.copy()
    vox = _le_incidence(ref, rec, lut_n, 96)[2]
    for m in (2, 3):                                   # a record of either TPC, for the detector rows of its TPC
        lut_n['t0_avg'][vox[m, 0], vox[m, 1], vox[m, 2]] = n_prof + 4
    _le_sum_fixture("grid_no_smear", over_ns, rec, lut_n, ids, [dict(n_ticks=1536, max_truth=2)],
                    bounds=dict(prefiltered=1, one_tick=8, no_tick=1), want_resident=1)

    # the ends of the axis: arrivals before tick 0 and past the last tick, a record whose whole profile precedes the start,
    # axes of two ticks and of one
    t_half = float(rec['t0'][9]) - 0.0005

    def ends_extra(ref, run, k, arrivals, deposits, init, res, st, en):
        te = rec['t0'] + n_prof * ref.consts.units.ns / ref.consts.units.mus
        return dict(whole_profile_before=int((te < st[0]).sum()), short_axis_lit=int(run["n_ticks"] <= 2 and len(deposits) > 0))
    _le_sum_fixture("axis_ends", over, rec, lut_g, ids,
                    [dict(start=0.1005, n_ticks=200, max_truth=2), dict(start=0.1, n_ticks=200, max_truth=2),
                     dict(start=t_half, n_ticks=2, max_truth=2), dict(start=t_half, n_ticks=1, max_truth=2)],
                    bounds=dict(before_axis=8, past_axis=8, whole_profile_before=2, short_axis_lit=2, one_tick=8), extra=ends_extra,
                    want_resident=0)

    # truth slots: 2 slots, tracks shared by segments, more tracks than slots, an id of -1, photons at the threshold and a step
    # above, a visiting order that is not descending, arrays that already hold sums and a slot 0 owned by a later track
    thr = 187.5                                         # = 3 * 2^-4 / LIGHT_TICK_SIZE: photons of a record can equal it exactly
    over_t = dict(base, ENABLE_LUT_SMEARING=True, MC_TRUTH_THRESHOLD=thr)
    t0s = np.array([0.0105, 0.0105, 0.0105, 0.0105, 0.012, 0.012, 0.0105, 0.0105, 0.02, 0.02, 0.0125, 0.0125,
                    0.0105, 0.0105, 0.021, 0.021, 0.0105, 0.0105, 0.012, 0.012, 0.0305, 0.0305, 0.0105, 0.0105])
    rec_t = _le_sum_records(_le_ref("module0", over_t), t0s)
    rec_t['n_photons'] = [3, 4, 6, 12, 5, 7, 24, 3, 9, 11, 13, 6, 48, 10, 3, 4, 14, 20, 15, 17, 3, 4, 28, 22]
    ids_t = np.array([7, 7, 3, -1, 9, 3, 12, 12, -1, 9, 7, 5, 21, -1, 30, 30, 40, 41, 3, 9, 50, 51, 60, 61], dtype='i8')
    lut_t = lut.copy()
    lut_t['vis'] = 0.5
    order_t = np.stack([np.arange(len(rec_t)) if d % 2 == 0 else (np.arange(len(rec_t)) * 7 + 3) % len(rec_t)
                        for d in range(len(LE_SUM_CHANNELS))])

    def preowned(ref, deposits, track_id, n_det, n_ticks, M):
        """a non-zero sum in some cells, slot 0 owned by the track that comes last among those a cell meets, slot 1 by a stranger"""
        out = np.zeros((n_det, n_ticks), dtype='f4')
        tid = np.full((n_det, n_ticks, M), -1, dtype='i8')
        tph = np.zeros((n_det, n_ticks, M))
        cells = _le_cells(deposits, thr)
        picked = 0
        for (idet, it), recs in sorted(cells.items()):
            tracks = [int(track_id[r]) for r, _ in recs if track_id[r] != -1]
            if len(set(tracks)) >= 2 and tracks[0] != tracks[-1]:
                out[idet, it] = 250.0
                tid[idet, it, 0] = tracks[-1]
                tph[idet, it, 0] = 500.0
                if picked % 2:
                    tid[idet, it, 1] = 99
                    tph[idet, it, 1] = 125.0
                picked += 1
        out[0, 0] = 62.5                              # (a cell nothing arrives in keeps what it holds)
        return out, tid, tph

    def truth_extra(ref, run, k, arrivals, deposits, init, res, st, en):
        cells = _le_cells(deposits, thr)
        full = minus_one = pre = 0
        for (idet, it), recs in cells.items():
            tracks = [int(ids_t[r]) for r, _ in recs]
            full += len(set(t for t in tracks if t != -1)) > run["max_truth"]
            minus_one += any(t == -1 and any(u != -1 for u in tracks[i + 1:]) for i, t in enumerate(tracks))
            if init is not None and init[1][idet, it, 0] != -1:
                pre += tracks[0] != init[1][idet, it, 0] and int(init[1][idet, it, 0]) in tracks
        at = sum(1 for d in deposits if d[5] == thr)
        above = sum(1 for d in deposits if d[5] == thr * 4 / 3)
        return dict(full_cells=full, minus_one_taken_over=minus_one, preowned=pre, at_threshold=min(at, above))
    _le_sum_fixture("truth_slots", over_t, rec_t, lut_t, ids_t,
                    [dict(start=0.0, n_ticks=64, max_truth=2), dict(start=0.0, n_ticks=64, max_truth=2, init=preowned)],
                    order=order_t, bounds=dict(full_cells=1, minus_one_taken_over=1, at_threshold=1, preowned=1), extra=truth_extra,
                    want_resident=0)


def gen_light_edges():
    """The reference's calculate_light_incidence, get_nticks and sum_light_signals at their edges:
    tests/golden/light_edge_<case>.npz with the overridden constants by name and `reach_*` counts, computed from the reference's
    expressions on the inputs, of what each case is there for (asserted here and again by the tests)."""
    _gen_le_incidence_cases()
    _gen_le_sum_cases()


def gen_light_export():
    """light_sim.export_to_hdf5 / export_light_trig_to_hdf5 / export_light_wvfm_to_hdf5 / zero_suppress_waveform_truth
    (light_sim.py:621-757) with h5py.File replaced by an in-memory sink: what lands in light_trig, light_wvfm and
    light_wvfm_mc_assn after two appending calls (trigger mode 0) and after the separate calls of trigger mode 1."""
    class _DS:
        def __init__(self, data):
            self.a = np.array(data)

        shape = property(lambda self: self.a.shape)

        def resize(self, n, axis=0):
            assert axis == 0
            self.a = np.concatenate([self.a, np.zeros((n - self.a.shape[0],) + self.a.shape[1:], dtype=self.a.dtype)])

        def __setitem__(self, k, v):
            self.a[k] = v

        def __getitem__(self, k):
            return self.a[k]

    class _File:
        store = {}

        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def __contains__(self, name):
            return name in self.store

        def create_dataset(self, name, data=None, **k):
            self.store[name] = _DS(data)

        def __getitem__(self, name):
            return self.store[name]

    for cfg, seed in (("module0", 81), ("2x2_no_modvar", 82)):
        ref = Ref(cfg)
        ls, light, sim = ref.light_sim, ref.light, ref.sim
        sim.MAX_MC_TRUTH_IDS = 3
        sim.MOD2MOD_VARIATION = False            # the driver sets it (cli/simulate_pixels.py:387)
        ls.h5py = types.SimpleNamespace(File=_File)
        _File.store = {}
        rng = np.random.default_rng(seed)
        all_ch = light.TPC_TO_OP_CHANNEL[:].ravel()
        ndm = 96 if light.LIGHT_TRIG_MODE == 0 else all_ch.shape[0]
        ns, Mt = 24, 3
        out = dict(light_trig_mode=light.LIGHT_TRIG_MODE)
        event_times = np.array([1000.5, 3.3e5, 1.21e6, 2.6e6])
        calls = []
        for icall, ntrig in enumerate((2, 1)):
            ev = np.full(ntrig, 1 + icall)
            start = np.full(ntrig, 0.25 * icall - 1.0)
            tidx = np.sort(rng.integers(0, 9000, ntrig))
            opc = np.stack([all_ch[:ndm]] * ntrig)
            wv = (rng.integers(-2000, 50, (ntrig, ndm, ns)) * 4).astype('f8')
            tid = np.full((ntrig, ndm, ns, Mt), -1, dtype='i8'); tph = np.zeros((ntrig, ndm, ns, Mt))
            hit = rng.random((ntrig, ndm, ns)) < 0.02
            for it, ic, isamp in zip(*np.nonzero(hit)):
                k = int(rng.integers(1, Mt + 1))
                tid[it, ic, isamp, :k] = rng.integers(0, 500, k)
                tph[it, ic, isamp, :k] = rng.uniform(0.1, 30.0, k)
            uniq_times = event_times[np.unique(ev) % sim.MAX_EVENTS_PER_FILE]
            i_trig = 5 + icall
            if light.LIGHT_TRIG_MODE == 0:
                ls.export_to_hdf5(ev, start, tidx, opc, wv, "x.h5", uniq_times, tid, tph, i_trig, -1)
            else:
                ls.export_light_wvfm_to_hdf5(ev, wv, "x.h5", tid, tph, i_trig, -1)
            calls.append(dict(event_id=ev, start_times=start, trigger_idx=tidx, op_channel_idx=opc, waveforms=wv,
                              true_track_id=tid.astype('i4'), true_photons=tph, event_times=uniq_times, i_trig=i_trig))
        if light.LIGHT_TRIG_MODE == 1:          # the once-per-file call, cli/simulate_pixels.py:1252-1259
            lev = np.array([0, 1, 3])
            ls.export_light_trig_to_hdf5(lev, np.full(3, 0), np.full(3, 0), all_ch, "x.h5", lev * sim.SPILL_PERIOD)
            out.update(trig1_event_id=lev, trig1_event_times=lev * sim.SPILL_PERIOD)
        for i, c in enumerate(calls):
            for k, v in c.items():
                out[f"call{i}_{k}"] = v
        trig = _File.store["light_trig"].a
        out.update(light_trig_op_channel=trig["op_channel"], light_trig_ts_s=trig["ts_s"], light_trig_ts_sync=trig["ts_sync"],
                   light_wvfm=_File.store["light_wvfm"].a)
        assn = _File.store["light_wvfm_mc_assn"].a
        for f in assn.dtype.names:
            out["assn_" + f] = assn[f]
        out["assn_dtype"] = np.array(str(assn.dtype.descr))
        np.savez_compressed(os.path.join(GOLD, f"light_export_{cfg}.npz"), **out)
        print("light_export", cfg, "mode", light.LIGHT_TRIG_MODE, "light_trig", trig.shape, trig.dtype, "wvfm",
              _File.store["light_wvfm"].a.shape, "assn", assn.shape)


def gen_packets():
    """fee.export_to_hdf5 (fee.py:84-356) on the golden chain's ADC arrays, replicated over events.  larpix-control is a
    third-party package that is not installed: its packet classes are replaced by attribute bags that record what the
    reference assigns (no logic of their own; assign_parity is a no-op), hdf5format.to_file and h5py.File by sinks.  The
    fixture therefore pins the reference's own logic -- which slots become packets, time ticks and rollover, the pixel ->
    io_group / io_channel / chip / channel mapping, the inserted timestamp / sync / trigger packets, the association rows --
    and nothing of larpix-control's byte format."""
    class _Bag:
        def __init__(self, kind, **kw):
            self.kind = kind
            self.__dict__.update(kw)

    class Packet_v2(_Bag):
        def __init__(self):
            super().__init__("data")

        def assign_parity(self):
            pass

    class TimestampPacket(_Bag):
        def __init__(self, timestamp=None):
            super().__init__("timestamp", timestamp=timestamp)

    class SyncPacket(_Bag):
        def __init__(self, sync_type=None, timestamp=None, io_group=None):
            super().__init__("sync", sync_type=sync_type, timestamp=timestamp, io_group=io_group)

    class TriggerPacket(_Bag):
        def __init__(self, io_group=None, trigger_type=None, timestamp=None):
            super().__init__("trigger", io_group=io_group, trigger_type=trigger_type, timestamp=timestamp)

    class Key:
        def __init__(self, io_group, io_channel, chip_id):
            self.io_group, self.io_channel, self.chip_id = io_group, io_channel, chip_id

    class _Attrs(dict):
        pass

    class _Node:
        def __init__(self):
            self.attrs = _Attrs()

    class _File:
        store = {}

        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def keys(self):
            return self.store.keys()

        def create_dataset(self, name, data=None, **k):
            self.store[name] = data

        def __getitem__(self, name):
            return self.store.setdefault(name, _Node())

    chain = np.load(os.path.join(GOLD, "chain_module0.npz"))
    for cfg, case, t_events in (("module0", "a", (1000.0, 250000.0, 1.2e6)), ("2x2_no_modvar", "b", (0.0, 1.2e6, 2.4e6))):
        ref = Ref(cfg)
        fee = ref.fee
        fee.Packet_v2, fee.TimestampPacket, fee.SyncPacket, fee.TriggerPacket, fee.Key = (
            Packet_v2, TimestampPacket, SyncPacket, TriggerPacket, Key)
        fee.PacketCollection = lambda packets, read_id=0, message='': packets
        fee.hdf5format = types.SimpleNamespace(to_file=lambda *a, **k: None)
        _File.store = {}
        fee.h5py = types.SimpleNamespace(File=_File)
        U0 = chain["unique_pix"].shape[0]
        n_ev = len(t_events)
        rng = np.random.default_rng(71)
        adc = np.concatenate([chain["adc_digit_low"]] * n_ev)
        ticks = np.concatenate([chain["adc_ticks_low"]] * n_ev)
        frac = np.concatenate([chain["adc_fractions_low"]] * n_ev)
        upix = np.concatenate([chain["unique_pix"]] * n_ev)
        tpm = np.concatenate([chain["track_pixel_map"]] * n_ev)
        # segment ids / trajectory ids of the slots (the driver maps track_pixel_map through them, cli :1107-1113)
        seg_ids = np.where(tpm >= 0, 1000 + tpm, -1)
        traj_ids = np.where(tpm >= 0, 7 + tpm // 2, -1)
        ev = np.repeat(np.arange(n_ev), U0)
        event_id_list = np.repeat(ev[:, None], adc.shape[1], axis=1)
        event_times = np.array(t_events)
        bad = None
        if case == "a":      # one live channel of the golden set disabled through a bad-channels file
            import tempfile, yaml
            pk, _ = fee.export_to_hdf5(event_id_list, adc, ticks, upix, frac, seg_ids, traj_ids, "x.h5", event_times,
                                       light_trigger_times=np.zeros(n_ev), light_trigger_event_id=np.arange(n_ev),
                                       light_trigger_modules=np.ones(n_ev))
            first = [p for p in pk if p.kind == "data"][3]
            bad_dict = {first.chip_key: [int(first.channel_id)]}
            fd, bad = tempfile.mkstemp(suffix=".yaml")
            with os.fdopen(fd, "w") as fh:
                yaml.safe_dump(bad_dict, fh)
            _File.store = {}
        pk, assn = fee.export_to_hdf5(event_id_list, adc, ticks, upix, frac, seg_ids, traj_ids, "x.h5", event_times,
                                      light_trigger_times=np.zeros(n_ev) + 3.0, light_trigger_event_id=np.arange(n_ev),
                                      light_trigger_modules=np.ones(n_ev), bad_channels=bad)
        rows = np.zeros(len(pk), dtype=[("kind", "i4"), ("io_group", "i8"), ("io_channel", "i8"), ("chip_id", "i8"),
                                        ("channel_id", "i8"), ("timestamp", "f8"), ("dataword", "i8"),
                                        ("trigger_type", "i8"), ("receipt_timestamp", "i8"), ("first_packet", "i8")])
        for i, p in enumerate(pk):
            r = rows[i]
            if p.kind == "data":
                g, c, chip = (int(x) for x in p.chip_key.split("-"))
                r["kind"] = 0; r["io_group"] = g; r["io_channel"] = c; r["chip_id"] = chip
                r["channel_id"] = p.channel_id; r["timestamp"] = p.timestamp; r["dataword"] = p.dataword
                r["receipt_timestamp"] = p.receipt_timestamp; r["first_packet"] = p.first_packet
            elif p.kind == "timestamp":
                r["kind"] = 4; r["timestamp"] = float(p.timestamp); r["io_group"] = p.chip_key.io_group
            elif p.kind == "sync":
                r["kind"] = 6; r["timestamp"] = p.timestamp; r["io_group"] = p.io_group; r["trigger_type"] = p.sync_type[0]
            else:
                r["kind"] = 7; r["timestamp"] = p.timestamp; r["io_group"] = p.io_group; r["trigger_type"] = p.trigger_type[0]
        # the driver's own packets between events (cli/simulate_pixels.py:876-890): fee.export_sync_to_hdf5 and
        # fee.export_timestamp_trigger_to_hdf5, for all io groups (i_mod = -1) and for module 1's (i_mod = 1)
        extra = {}

        def bag_rows(pk):
            rr = np.zeros(len(pk), dtype=[("kind", "i4"), ("io_group", "i8"), ("timestamp", "f8"), ("trigger_type", "i8")])
            for i, p in enumerate(pk):
                if p.kind == "timestamp":
                    rr[i] = (4, p.chip_key.io_group, float(p.timestamp), 0)
                elif p.kind == "sync":
                    rr[i] = (6, p.io_group, p.timestamp, p.sync_type[0])
                else:
                    rr[i] = (7, p.io_group, p.timestamp, p.trigger_type[0])
            return rr
        period = ref.detector.CLOCK_RESET_PERIOD * ref.detector.CLOCK_CYCLE
        sync_times = np.array([period, period, 3 * period + 17.0])       # the last one is not a multiple: floored with a warning
        for i_mod in (-1, 1):
            import warnings
            saved = _File.store
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                _File.store = {}
                pk_s, as_s = fee.export_sync_to_hdf5("x.h5", sync_times, i_mod)
            _File.store = {}
            pk_t, as_t = fee.export_timestamp_trigger_to_hdf5("x.h5", event_times, i_mod)
            _File.store = saved
            extra[f"sync_rows_{i_mod}"] = bag_rows(pk_s)
            extra[f"tt_rows_{i_mod}"] = bag_rows(pk_t)
            extra[f"sync_assn_n_{i_mod}"] = len(as_s)
            assert (as_s["event_ids"] == -1).all() and (as_t["segment_ids"] == -1).all() and (as_t["fraction"] == 0).all()
        extra["sync_times"] = sync_times
        np.savez_compressed(os.path.join(GOLD, f"packets_{cfg}.npz"), event_id_list=event_id_list.astype("i4"), **extra,
                            adc=adc, ticks=ticks, fractions=frac, unique_pix=upix, segment_ids=seg_ids, traj_ids=traj_ids,
                            event_times=event_times, trig_times=np.zeros(n_ev) + 3.0,
                            bad_key=np.array(list(bad_dict.keys())[0] if bad else ""),
                            bad_channel=np.array(list(bad_dict.values())[0][0] if bad else -1),
                            rows=rows, assn_event_ids=assn["event_ids"], assn_segment_ids=assn["segment_ids"],
                            assn_fraction=assn["fraction"], assn_file_traj_ids=assn["file_traj_ids"],
                            assn_fraction_traj=assn["fraction_traj"],
                            config_attrs=np.array([_File.store["configs"].attrs[k] for k in
                                                   ("vdrift", "long_diff", "tran_diff", "lifetime", "drift_length")]))
        kinds = {k: int((rows["kind"] == k).sum()) for k in (0, 4, 6, 7)}
        print("packets", cfg, "trig mode", ref.light.LIGHT_TRIG_MODE, "packets", len(pk), kinds)


# --------------------------------------------------------------------------
# fee: the self-trigger scan on hand-made dense waveforms
# --------------------------------------------------------------------------
FEE_CONST_NAMES = ("BUFFER_RISETIME", "ADC_HOLD_DELAY", "ADC_BUSY_DELAY", "RESET_CYCLES", "MAX_ADC_VALUES",
                   "RESET_NOISE_CHARGE", "UNCORRELATED_NOISE_CHARGE", "DISCRIMINATOR_NOISE")
# what a variant sets on the reference's detector / sim modules (MAX_ADC_VALUES lives in sim); `noisy` keeps the shipped noise
FEE_VARIANTS = (("default", {}), ("no_risetime", {"BUFFER_RISETIME": 0}),
                ("long", {"ADC_HOLD_DELAY": 70, "ADC_BUSY_DELAY": 80, "RESET_CYCLES": 3}),
                ("cap", {"MAX_ADC_VALUES": 3}), ("noisy", {}))
FEE_SEED = 20261018
FEE_M = 3


def _fee_owner(ref, name):
    return ref.sim if name == "MAX_ADC_VALUES" else ref.detector


def _fee_prefix_charge(cur, dt, rt):
    """running sum of the buffer-convolved charge from tick 0 with no reset in between (fee.py:566-581 before any trigger),
    in plain numpy: where the generator expects the first threshold crossing of a row"""
    if rt > 0:
        ntap = int(np.ceil(10 * rt / dt))
        w = np.exp(-np.arange(ntap + 1) * dt / rt) * (1 - np.exp(-dt / rt))
        q = np.convolve(cur * dt, w)[:cur.shape[0]]
    else:
        q = cur * dt
    return np.cumsum(q)


def _fee_rows(NT, dt, rt, interval, busy_ticks, reset_ticks, thr0):
    """The rows of one variant: (name, threshold, components); a component is (per-tick charge [NT] in electrons, the three
    tracks' shares of it).  Spikes sit on single ticks so that the tick of every threshold crossing is known by construction."""
    def spike(t, q):
        a = np.zeros(NT)
        a[t] = q
        return a

    def plateau(t0, t1, q):
        a = np.zeros(NT)
        a[t0:t1] = q
        return a

    def gauss(c, sigma, q):
        t = np.arange(NT)
        a = np.where(np.abs(t - c) <= 4 * sigma, np.exp(-0.5 * ((t - c) / sigma) ** 2), 0.0)
        return a * (q / np.exp(-0.5 * (np.arange(-4 * sigma, 4 * sigma + 1) / sigma) ** 2).sum())

    one = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
    rows = []
    rows.append(("a_plain", thr0, [(spike(700, 20000.0), (0.7, 0.3, 0))]))
    rows.append(("a_gauss", thr0, [(gauss(1200, 6, 15000.0), one[0]), (gauss(1204, 5, 9000.0), one[1]),
                                   (gauss(1195, 8, 6000.0), one[2])]))
    rows.append(("b_start", thr0, [(spike(0, 4000.0), one[0]), (spike(1, 4000.0), one[1]), (spike(2, 4000.0), one[2])]))
    for name, t in (("c_lane63", 63), ("c_lane0", 64), ("c_lane63_second", 127), ("c_lane0_third", 128)):
        rows.append((name, thr0, [(spike(t - 3, 5000.0), one[0]), (spike(t, 5000.0), one[1])]))
    # d: +9000 crosses, -4000 inside the integration pulls the sum below the threshold: failed trigger.  3000 electrons on the
    # tick just before the moved last_reset (a tick the scan never visits) must not reach the clean pulse that follows.
    lead = spike(400, 9000.0)
    c = int(np.flatnonzero(_fee_prefix_charge(lead / dt, dt, rt) >= thr0)[0])
    moved = c + interval + 1 + reset_ticks
    rows.append(("d_failed", thr0, [(lead, one[0]), (spike(405, -4000.0), one[1]), (spike(moved - 1, 3000.0), one[2]),
                                    (spike(moved + 30, 20000.0), (0.6, 0.4, 0))]))
    rows.append(("e_plateau", thr0, [(plateau(300, 700, 1000.0), one[0]), (plateau(300, 500, 500.0), one[1]),
                                     (plateau(500, 700, 500.0), one[2])]))
    # second pulse three ticks after the reset of the first hit: crosses while the ADC is busy and has to wait
    rows.append(("e_busy_cross", thr0, [(spike(1000, 20000.0), one[0]),
                                        (spike(1000 + interval + 1 + reset_ticks + 3, 12000.0), one[1])]))
    rows.append(("f_end_interval", thr0, [(spike(NT - interval + 2, 20000.0), (0.5, 0.25, 0.25))]))
    rows.append(("f_end_ntap", thr0, [(spike(NT - 2, 20000.0), (0.5, 0.5, 0))]))
    rows.append(("f_end_gauss", thr0, [(gauss(NT - 4, 3, 30000.0), (0.2, 0.3, 0.5))]))
    rows.append(("g_cap", thr0, [(plateau(100, 1900, 1500.0), (0.6, 0.4, 0))]))
    rows.append(("h_cancel", thr0, [(spike(900, 40000.0), one[0]), (spike(900, -20000.0), one[1])]))
    # threshold below zero: triggers at tick 0 on no charge; the negative lobe makes true_q <= 0 at the hit
    rows.append(("h_negq", -3000.0, [(spike(5, -3000.0), one[0]), (spike(5, 1000.0), one[1]), (spike(1000, 15000.0), one[2])]))
    rows.append(("i_zero", thr0, []))
    rows.append(("i_below", thr0, [(spike(1000, 6800.0), (0.5, 0.5, 0))]))
    for name, thr in (("j_thr_low", 3000.0), ("j_thr_mid", 9000.0), ("j_thr_high", 12000.0), ("j_thr_zero", 0.0)):
        rows.append((name, thr, [(spike(500, 10000.0), (0.25, 0.25, 0.5))]))
    rows.append(("k_two_far", thr0, [(spike(200, 20000.0), one[0]), (spike(1500, 20000.0), one[1])]))
    rows.append(("l_negative", thr0, [(spike(800, -5000.0), one[2])]))
    rows.append(("m_wide", thr0, [(gauss(1000, 40, 60000.0), (0.5, 0.3, 0.2))]))
    return rows


def gen_fee():
    """fee.get_adc_values (fee.py:517-655) and fee.digitize on dense hand-made waveforms, one pixel per row, under five sets of
    constants -> tests/golden/fee_scan_<variant>.npz (inputs, the constants used, the reference's outputs, expect_* counts).
    The generator itself proves which branch each row reached (asserts + one printed line per row) and, for the noiseless
    variants, that no decision sits on the threshold (same hits and stamps with every threshold scaled by 1 +- 1e-9).
    `noisy`: the normals are the draws of the oracle's restated xoroshiro128p stream, so the reference's control flow
    consumes the numbers the HIP table path produces; the seed, the states after the call and the draw counts are recorded."""
    import contextlib
    import io
    import time
    try:
        from oracle import oracle as ORC
    except ImportError:
        import oracle as ORC
    for variant, over in FEE_VARIANTS:
        t_begin = time.time()
        noisy = variant == "noisy"
        draws = []

        def normal(states, ip):
            # a Python float: Numba types f32 * f64 as f64 (a NumPy f32 scalar would keep the products in f32)
            draws[ip] += 1
            return float(ORC.rng_normals(states, ip, 1)[0])
        ref = Ref("module0", noise_zero=not noisy, normal=normal if noisy else None)
        det, sim = ref.detector, ref.sim
        for k, v in over.items():
            setattr(_fee_owner(ref, k), k, v)
        dt, rt = det.TIME_SAMPLING, det.BUFFER_RISETIME
        # the reference's own expressions (fee.py:590,620,647)
        interval = round((3 * det.CLOCK_CYCLE + det.ADC_HOLD_DELAY * det.CLOCK_CYCLE) / det.TIME_SAMPLING)
        busy_ticks = round(det.ADC_BUSY_DELAY * det.CLOCK_CYCLE / det.TIME_SAMPLING)
        reset_ticks = round(det.RESET_CYCLES * det.CLOCK_CYCLE / det.TIME_SAMPLING)
        if variant == "long":
            assert interval > 64 and busy_ticks > 64 and reset_ticks > 1, (interval, busy_ticks, reset_ticks)
        NT = len(det.TIME_TICKS)
        A, M = sim.MAX_ADC_VALUES, FEE_M
        thr0 = det.DISCRIMINATION_THRESHOLD * ref.consts.units.e
        rows = _fee_rows(NT, dt, rt, interval, busy_ticks, reset_ticks, thr0)
        U = len(rows)
        names = [r[0] for r in rows]
        thresholds = np.array([r[1] for r in rows], dtype=np.float64)
        pts = np.zeros((U, NT, M))
        for u, (_, _, comps) in enumerate(rows):
            for charge, share in comps:
                for m in range(M):
                    pts[u, :, m] += charge / dt * share[m]          # e-/us
        ps = pts[:, :, 0] + pts[:, :, 1] + pts[:, :, 2]
        time_ticks = np.linspace(0, 1 * det.TIME_INTERVAL[1], NT + 1)

        def run(thr, states):
            adc = np.zeros((U, A)); ticks = np.zeros((U, A)); frac = np.zeros((U, A, M))
            del draws[:]
            draws.extend([0] * U)
            sink = io.StringIO()
            with contextlib.redirect_stdout(sink):       # (the reference prints a line per pixel that reaches the cap)
                ref.fee.get_adc_values[max(1, -(-U // 128)), 128](ps, pts, time_ticks, adc, ticks, 0, states, frac, thr)
            return adc, ticks, frac, sink.getvalue().count("More ADC values than possible")

        states = ORC.rng_create_states(U, FEE_SEED) if noisy else np.zeros(1)
        adc, ticks, frac, n_cap = run(thresholds, states)
        n_draws = np.array(draws, dtype=np.int64)
        digit = ref.fee.digitize(adc)
        # ---- margin: no decision on the threshold (device exp and libm differ in the last bit) ----
        # (with noise: the f32 normals differ in the last bit between device and host, 6e-8 of a few thousand electrons, so
        # the same check at 2e-7, the stream restarted: a flipped decision would also shift every later draw)
        for s in (1 + 1e-9, 1 - 1e-9) if not noisy else (1 + 2e-7, 1 - 2e-7):
            adc_s, ticks_s, _, _ = run(thresholds * s, ORC.rng_create_states(U, FEE_SEED) if noisy else np.zeros(1))
            for u in range(U):
                assert np.array_equal(adc_s[u] != 0, adc[u] != 0) and np.array_equal(ticks_s[u], ticks[u]), \
                    f"fee {variant} row {names[u]}: a decision sits on the threshold (scale {s!r}): reshape the row"
        # ---- coverage: what each row reached, from the reference's outputs ----
        hits = (adc != 0).sum(axis=1)
        slots = (ticks != 0).sum(axis=1)
        beyond = (ticks > time_ticks[-1]).sum(axis=1)
        first_cross = np.full(U, -1, dtype=np.int64)
        for u in range(U):
            above = np.flatnonzero(_fee_prefix_charge(ps[u], dt, rt) >= thresholds[u])
            first_cross[u] = above[0] if len(above) else -1

        def stamp(c):
            ic = c + interval + 1
            return time_ticks[min(ic, NT)] - 2 + max(ic - NT, 0)
        row = {n: u for u, n in enumerate(names)}
        if not noisy:
            for u, n in enumerate(names):
                if first_cross[u] < 0:
                    assert slots[u] == 0, (variant, n, "a hit without a crossing")
                elif n == "d_failed":
                    # the only hit is the clean pulse, 30 ticks after the reset that followed the failed trigger
                    assert hits[u] == 1 and ticks[u, 0] == stamp(first_cross[u] + interval + 1 + reset_ticks + 30), \
                        (variant, n, ticks[u, :3])
                    assert not np.any(ticks[u] == stamp(first_cross[u])), (variant, n, "the failed trigger left a hit")
                else:
                    assert ticks[u, 0] == stamp(first_cross[u]), (variant, n, first_cross[u], ticks[u, 0])
            for n, lane in (("c_lane63", 63), ("c_lane0", 64), ("c_lane63_second", 127), ("c_lane0_third", 128)):
                assert first_cross[row[n]] == lane, (variant, n, first_cross[row[n]])
            assert first_cross[row["b_start"]] <= 2 and hits[row["b_start"]] == 1
            assert hits[row["a_plain"]] == 1 and hits[row["h_cancel"]] == 1
            assert hits[row["e_plateau"]] >= 2 and hits[row["k_two_far"]] == 2
            # e_busy_cross: the second pulse crossed 3 ticks after the reset; its hit waited for the busy counter to run out
            u = row["e_busy_cross"]
            assert hits[u] == 2 and ticks[u, 1] == stamp(1000 + interval + 1 + reset_ticks + max(busy_ticks - 1, 3)), ticks[u, :3]
            for n in ("f_end_interval", "f_end_ntap", "f_end_gauss"):
                assert hits[row[n]] == 1 and beyond[row[n]] == 1, (variant, n, ticks[row[n], :2])
            # (with `long`'s 150-tick cycle the waveform ends before MAX_ADC_VALUES hits)
            full = A if variant != "long" else 10
            assert hits[row["g_cap"]] >= full and (n_cap >= 1 or variant == "long"), (variant, hits[row["g_cap"]], n_cap)
            if variant == "cap":
                assert A == 3 and hits[row["g_cap"]] == 3 and hits[row["e_plateau"]] == 3
            # h_cancel: normalised fractions of opposite sign; h_negq: true_q <= 0 at the first hit, fractions left as charges
            np.testing.assert_allclose(frac[row["h_cancel"], 0], (2.0, -1.0, 0.0), rtol=1e-12, atol=1e-12)
            u = row["h_negq"]
            assert adc[u, 0] < 0 and frac[u, 0, 0] < -1000 and frac[u, 0, 1] > 300, (adc[u, 0], frac[u, 0])
            assert slots[row["j_thr_zero"]] >= full and slots[u] >= full and ticks[row["j_thr_zero"], 0] == stamp(0)
            assert hits[row["j_thr_low"]] == 1 and hits[row["j_thr_mid"]] == 1 and hits[row["j_thr_high"]] == 0
            for n in ("i_zero", "i_below", "l_negative"):
                assert slots[row[n]] == 0, (variant, n)
        else:
            # every tick of the empty row drew its two normals, plus the one before the loop (fee.py:557,583-584)
            assert n_draws[row["i_zero"]] >= 1 + 2 * NT
            assert not np.array_equal(states.view("u8"), ORC.rng_create_states(U, FEE_SEED).view("u8"))
        for u, n in enumerate(names):
            print(f"fee {variant:11s} row {n:16s} thr {thresholds[u]:8.1f} hits {hits[u]:2d} slots {slots[u]:2d} "
                  f"first crossing {first_cross[u]:5d} first stamp {ticks[u, 0]:9.4f} beyond end {beyond[u]}"
                  + (f" draws {n_draws[u]}" if noisy else ""))
        out = dict(rows=np.array(names), pixels_signals=ps, pixels_signals_tracks=pts, thresholds=thresholds,
                   time_ticks_stop=np.float64(time_ticks[-1]), const_names=np.array(FEE_CONST_NAMES),
                   const_values=np.array([float(getattr(_fee_owner(ref, k), k)) for k in FEE_CONST_NAMES]),
                   interval=np.int64(interval), busy_ticks=np.int64(busy_ticks), reset_ticks=np.int64(reset_ticks),
                   adc_list=adc, adc_ticks_list=ticks, current_fractions=frac, adc_digit=digit,
                   expect_hits=hits, expect_slots=slots, expect_beyond_end=beyond, expect_first_crossing=first_cross,
                   expect_cap_breaks=np.int64(n_cap))
        if noisy:
            out.update(rng_seed=np.int64(FEE_SEED), rng_states_after=states.view("u8").reshape(-1, 2).copy(), n_draws=n_draws)
        path = os.path.join(GOLD, f"fee_scan_{variant}.npz")
        np.savez_compressed(path, **out)
        print(f"fee {variant}: interval {interval} busy_ticks {busy_ticks} reset_ticks {reset_ticks} rows {U} hits {int(hits.sum())} "
              f"slots {int(slots.sum())} cap breaks {n_cap} margin check passed "
              f"{os.path.getsize(path)} bytes {time.time() - t_begin:.1f} s")


# --------------------------------------------------------------------------
# mc: tracks_current_mc on the table streams this project defines
# --------------------------------------------------------------------------
MC_SEED = 20261020
MC_FRAGILE_MARGIN = 8.0      # spacings of float32 at the draw's Box-Muller radius (tests/test_gpu_mc_current.py)
MC_FRAGILE_CAP = 0.01
# end points: (x, y) in pixel pitches from the low corner of TPC 0's pixel plane, depth in cm from its anode (negative: from the
# cathode).  diag: the z_start < z_end branch, diag_swapped the other; steep: 3.5 cm along the drift, hundreds of steps; inside:
# ~300 um, wholly inside the impact circle (s_minus 0, s_plus 1, a few steps); tiny: round(length / MIN_STEP_SIZE) is 0 and the
# max(.., 1) acts; anode: the first ~1850 ticks have time_tick < 0; cathode: the longest drift, the last ticks of the window.
# No segment runs exactly along z: l == 0 divides by zero in the pure-Python run (the device's "no signal" there is the
# HIP-vs-oracle tests' business).
MC_SEGMENTS = {
    "diag": ((60.30, 120.40, 15.0), (60.90, 120.80, 15.4)),
    "diag_swapped": ((60.90, 120.80, 15.4), (60.30, 120.40, 15.0)),
    "steep": ((70.45, 130.50, 10.0), (70.62, 130.58, 13.5)),
    "inside": ((80.50, 140.50, 20.00), (80.55, 140.53, 20.02)),
    "tiny": ((85.500, 145.500, 18.000), (85.505, 145.503, 18.002)),
    "anode": ((90.30, 150.60, 0.4), (90.70, 150.35, 1.0)),
    "cathode": ((95.40, 155.30, -0.6), (95.65, 155.60, -0.2)),
    "short_a": ((60.50, 120.50, 25.00), (60.53, 120.52, 25.02)),
    "short_b": ((64.40, 124.45, 27.03), (64.47, 124.40, 27.00)),
}
MC_CASES = (
    ("module0_plain", "module0", "survey", {"MIN_STEP_SIZE": 0.01, "MC_SAMPLE_MULTIPLIER": 1},
     ("diag", "diag_swapped", "steep", "inside", "tiny", "anode", "cathode")),
    ("module0_multi", "module0", "golden", {"MIN_STEP_SIZE": 0.001, "MC_SAMPLE_MULTIPLIER": 3}, ("short_a", "short_b")),
    ("ndlar_plain", "ndlar", "golden", {"MIN_STEP_SIZE": 0.01, "MC_SAMPLE_MULTIPLIER": 1},
     ("diag", "diag_swapped", "steep", "anode")),
)


def mc_segments(det, names):
    from larndsim_amd.layout import segments_dtype
    B = np.asarray(det.TPC_BORDERS)[0]
    sgn = np.sign(B[2, 1] - B[2, 0])
    depth_max = abs(B[2, 1] - B[2, 0])
    seg = np.zeros(len(names), dtype=segments_dtype)
    for i, name in enumerate(names):
        for end, (px, py, depth) in zip(("start", "end"), MC_SEGMENTS[name]):
            seg["x_" + end][i] = B[0, 0] + px * det.PIXEL_PITCH
            seg["y_" + end][i] = B[1, 0] + py * det.PIXEL_PITCH
            seg["z_" + end][i] = B[2, 0] + sgn * (depth if depth >= 0 else depth_max + depth)
    if "diag" in names:     # whatever the sign of the drift axis, `diag` is the one with z_start < z_end
        i, j = names.index("diag"), names.index("diag_swapped")
        if not seg["z_start"][i] < seg["z_end"][i]:
            seg[[i, j]] = seg[[j, i]]
    for ax in "xyz":
        seg[ax] = 0.5 * (seg[ax + "_start"].astype(np.float64) + seg[ax + "_end"])
    d = np.stack([seg[ax + "_end"].astype(np.float64) - seg[ax + "_start"] for ax in "xyz"])
    seg["dx"] = np.sqrt((d * d).sum(axis=0))
    seg["dEdx"] = 2.1 + 0.2 * np.arange(len(names))
    seg["dE"] = seg["dEdx"].astype(np.float64) * seg["dx"]
    seg["segment_id"] = np.arange(len(names))
    return seg


def _mc_far_pixel(det, r, pid, impact):
    """a pixel of the plane of `pid` whose centre lies farther than `impact` from the line of segment record r (in x, y)"""
    N0, N1 = int(det.N_PIXELS[0]), int(det.N_PIXELS[1])
    plane, py0, px0 = pid // (N0 * N1), (pid // N0) % N1, pid % N0
    B = np.asarray(det.TPC_BORDERS)[plane]
    a = np.array([r["x_start"], r["y_start"]])
    v = np.array([r["x_end"], r["y_end"]]) - a
    v /= np.linalg.norm(v)
    for dx, dy in ((9, 0), (0, 9), (-9, 9), (9, 9), (-9, 0), (0, -9), (14, -7), (-7, 14)):
        px, py = px0 + dx, py0 + dy
        if not (0 <= px < N0 and 0 <= py < N1):
            continue
        p = np.array([px * det.PIXEL_PITCH + B[0, 0] + det.PIXEL_PITCH / 2, py * det.PIXEL_PITCH + B[1, 0] + det.PIXEL_PITCH / 2]) - a
        if abs(p[0] * v[1] - p[1] * v[0]) > 1.2 * impact:
            return px + N0 * (py + N1 * plane)
    raise AssertionError("no far pixel found")


def _mc_stream_state(ORC, states, index, it):
    """mc_stream_words (csrc/kernels_mc.hip) of table state `index` and tick `it`, restated: SplitMix64's output function of the
    two words offset by the tick"""
    M = (1 << 64) - 1

    def fin(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    z0 = fin((int(states["s0"][index]) + 0x9E3779B97F4A7C15 * (it + 1)) & M)
    z1 = fin(int(states["s1"][index]) ^ ((0xD1B54A32D192ED03 * (it + 1)) & M))
    if (z0 | z1) == 0:
        z0 = 1
    st = np.zeros(1, dtype=ORC.RNG_DTYPE)
    st["s0"], st["s1"] = z0, z1
    return st


def _mc_job(args):
    case, cfg, kind, over, r, pixels, T, itrk, bound = args
    from larndsim_amd import synth
    try:
        from oracle import oracle as ORC
    except ImportError:
        import oracle as ORC
    S, P = pixels.shape
    states = ORC.rng_create_states(S * P, MC_SEED)
    counts = np.zeros((P, T), dtype=np.int64)
    cur = {"pos": None, "buf": None, "d": 0}

    def normal(rng_state, index):
        # the state argument is ignored: draw d of thread (itrk, ipix, it) is draw d of the table-mode stream of that entry,
        # all fetched at the thread's first draw.  A Python float: Numba types f32 * f64 as f64.
        pos = _State.pos
        if pos != cur["pos"]:
            cur["pos"], cur["d"] = pos, 0
            cur["buf"] = ORC.rng_normals(_mc_stream_state(ORC, states, pos[0] + S * pos[1], pos[2]), 0, bound)
        v = float(cur["buf"][cur["d"]])
        cur["d"] += 1
        counts[pos[1], pos[2]] = cur["d"]
        return v
    ref = Ref(cfg, noise_zero=False, normal=normal)
    for k, v in over.items():
        setattr(ref.sim, k, v)
    response = synth.make_response(kind, response_sampling=ref.detector.RESPONSE_SAMPLING)
    # census of the look-ups: how many samples reached get_closest_waveform, how many of them past the table's last tick
    seen = {"lookups": 0, "k_past_end": 0}
    inner = ref.detsim.get_closest_waveform

    def counted(x, y, t, resp):
        seen["lookups"] += 1
        seen["k_past_end"] += round(t / ref.detector.RESPONSE_SAMPLING) >= resp.shape[2]
        return inner(x, y, t, resp)
    ref.detsim.get_closest_waveform = counted
    signals = np.zeros((S, P, T))
    _State.x_only = [itrk]
    ref.detsim.tracks_current_mc[(S, P, T), (1, 1, 1)](signals, pixels, r, response, states)
    _State.x_only = None
    return itrk, signals[itrk], counts, seen


def gen_mc(jobs):
    """detsim.tracks_current_mc (detsim.py:258-348) run thread by thread on hand-placed segments, its normals the draws of the
    table-mode streams (one per (segment, pixel, tick): csrc/kernels_mc.hip) -> tests/golden/mc_<case>.npz: the records after the
    reference's quench and drift, the pixel rows (get_pixels at radius 1, then per segment a pixel farther than the impact
    radius and a -1), T, seed, constants, the f64 signals and the draw count of every entry.  One census line per segment."""
    import time
    try:
        from oracle import oracle as ORC
    except ImportError:
        import oracle as ORC
    from larndsim_amd import consts as my_consts, synth
    for case, cfg, kind, over, names in MC_CASES:
        t_begin = time.time()
        ref = Ref(cfg, noise_zero=False)
        det = ref.detector
        for k, v in over.items():
            setattr(ref.sim, k, v)
        seg = mc_segments(det, list(names))
        r = run_quench_drift(ref, to_ref(seg), ref.physics.BIRKS)
        S = r.shape[0]
        assert (r["pixel_plane"] != det.DEFAULT_PLANE_INDEX).all()
        mp = np.array([0])
        ref.pixels_from_track.max_pixels[1, 128](r, mp)
        nmax = int(mp[0])
        P0 = 3 * nmax + 6                                                      # cli/simulate_pixels.py:928 at radius 1
        active = np.full((S, nmax), -1, dtype=np.int32)
        neigh = np.full((S, P0), -1, dtype=np.int32)
        nrad = np.full((S, P0), -1, dtype=np.int32)
        ref.pixels_from_track.get_pixels[1, 128](r, active, neigh, nrad, np.zeros(S), 1)
        shape = (45, 45)
        impact = np.sqrt(shape[0] ** 2 + shape[1] ** 2) * det.RESPONSE_BIN_SIZE
        far = np.array([_mc_far_pixel(det, r[i], int(neigh[i][neigh[i] >= 0][0]), impact) for i in range(S)], dtype=np.int32)
        pixels = np.concatenate([neigh, far[:, None], np.full((S, 1), -1, dtype=np.int32)], axis=1)
        P = pixels.shape[1]
        starts, tmax = np.empty(S), np.array([0])
        ref.detsim.time_intervals[1, 128](starts, tmax, r)
        T = int(tmax[0])
        length = np.sqrt((r["x_end"] - r["x_start"]) ** 2 + (r["y_end"] - r["y_start"]) ** 2 + (r["z_end"] - r["z_start"]) ** 2)
        mult = int(ref.sim.MC_SAMPLE_MULTIPLIER)
        bound = [3 * mult * (max(int(round(L / ref.sim.MIN_STEP_SIZE)), 1) + 1) for L in length]
        with Pool(min(jobs, S)) as pool:
            res = pool.map(_mc_job, [(case, cfg, kind, over, r, pixels, T, i, bound[i]) for i in range(S)], chunksize=1)
        signals = np.zeros((S, P, T))
        n_draws = np.zeros((S, P, T), dtype=np.int64)
        seen = {}
        for itrk, s, c, sn in res:
            signals[itrk], n_draws[itrk], seen[itrk] = s, c, sn
        # ---- the oracle on the same streams: margins (the share of fragile entries) ----
        my_consts.load_snapshot(cfg)
        for k, v in over.items():
            setattr(my_consts.sim, k, v)
        resp = synth.make_response(kind, response_sampling=det.RESPONSE_SAMPLING)
        assert resp.shape[:2] == shape
        o = ORC.tracks_current_mc_detail(r, pixels, T, resp, ORC.rng_create_states(S * P, MC_SEED))
        nz = signals != 0
        fragile = float((o["margin"][nz] < MC_FRAGILE_MARGIN).mean())
        assert fragile <= MC_FRAGILE_CAP, f"mc {case}: {fragile:.4f} of the non-zero entries are fragile: reshape the case"
        # ---- census: what each segment reached, from the reference's signals and draw counts ----
        for i, name in enumerate(names):
            real = np.flatnonzero(pixels[i, :P0] >= 0)
            cnt = n_draws[i]
            assert not cnt[P0].any() and not signals[i, P0].any() and cnt[real].any(), (case, name, "rr > impact row")
            assert not cnt[P0 + 1].any() and not cnt[:P0][pixels[i, :P0] < 0].any(), (case, name, "-1 slots")
            drew = cnt[real] > 0
            # a row's samples per tick: its all-one-draw ticks (the last ticks of T lie past every sample's window)
            nsamp = np.array([row[row > 0].min() if (row > 0).any() else 0 for row in cnt[real]])
            assert (cnt[real] <= 3 * nsamp[:, None]).all() and (nsamp % mult == 0).all()
            nstep = nsamp // mult
            first = drew.argmax(axis=1)[drew.any(axis=1)]
            one = int((drew & (cnt[real] == nsamp[:, None])).sum())
            three = int((drew & (cnt[real] == 3 * nsamp[:, None])).sum())
            mixed = int(drew.sum()) - one - three
            swapped = not r["z_start"][i] < r["z_end"][i]
            print(f"mc {case:14s} {name:13s} T {T} swapped {int(swapped)} rows {len(real)} nstep {nstep[nstep > 0].min()}"
                  f"..{nstep.max()} ticks before time 0 {first.min()}..{first.max()} entries with 1 draw/sample {one} with 3 {three} "
                  f"mixed {mixed} non-zero {int(nz[i].sum())} look-ups {seen[i]['lookups']} past the table's end "
                  f"{seen[i]['k_past_end']} draws {int(cnt.sum())} far pixel {pixels[i, P0]}")
            assert T > 256 and first.min() > 0 and one > 0 and three > 0
            if name == "diag":
                assert not swapped
            if name == "diag_swapped":
                assert swapped
            if name == "tiny":
                assert nstep.max() == 1
            if name == "inside":
                assert 2 <= nstep.max() <= 5 and nstep[nstep > 0].min() == nstep.max()
            if name == "steep":
                assert nstep.max() > 256
            if name == "anode":
                assert first.min() > 1500
        out = dict(case=np.array(case), cfg=np.array(cfg), response_kind=np.array(kind), segment_names=np.array(names),
                   segments_in=seg, tracks=r, pixels=pixels, n_neigh=np.int64(P0), T=np.int64(T), seed=np.int64(MC_SEED),
                   const_names=np.array(sorted(over)), const_values=np.array([float(over[k]) for k in sorted(over)]),
                   track_starts=starts, fragile_share=np.float64(fragile))
        out.update(sparse_fields("signals", signals))
        out.update(sparse_fields("n_draws", n_draws))
        path = os.path.join(GOLD, f"mc_{case}.npz")
        save_npz_fixed(path, out)
        print(f"mc {case}: S {S} P {P} T {T} non-zero {int(nz.sum())} draws {int(n_draws.sum())} largest count {int(n_draws.max())} "
              f"share of non-zero entries with margin < {MC_FRAGILE_MARGIN:g}: {fragile:.5f} (cap {MC_FRAGILE_CAP}) "
              f"{os.path.getsize(path)} bytes {time.time() - t_begin:.1f} s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="consts,qd,pixels,light,sampled,chain")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    if not os.path.isdir(REF):
        print("reference checkout not present; nothing to do")
        return 0
    os.makedirs(GOLD, exist_ok=True)
    for s in a.sets.split(","):
        {"consts": gen_consts, "qd": gen_qd, "pixels": gen_pixels, "light": gen_light, "light_response": gen_light_response,
         "sampled": lambda: gen_sampled(a.jobs), "chain": lambda: gen_chain(a.jobs), "packets": gen_packets, "light_wvfm": gen_light_wvfm, "light_wvfm_edges": gen_light_wvfm_edges, "light_edges": gen_light_edges, "light_export": gen_light_export, "fee": gen_fee,
         "pixels_wide": lambda: gen_pixels_wide(a.jobs), "mc": lambda: gen_mc(a.jobs)}[s]()
    return 0


if __name__ == "__main__":
    sys.exit(main())
