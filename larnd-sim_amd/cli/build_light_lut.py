#!/usr/bin/env python
"""
build_light_lut.py -- build a light look-up table by photon transport in a TPC box (larndsim_amd/lut_builder.py).

  build_light_lut.py --geometry box.json --vox_div 14 26 8 --photons 1000000 --seed 1 --output lightLUT.npz

The geometry file is JSON: {"box": [Lu, Lv, Lw], "detectors": [{"wall": "u0", "lo": [a, b], "hi": [a, b]}, ..]} (cm; walls u0 u1
v0 v1 w0 w1; lo / hi in the wall's in-plane coordinates in cyclic axis order).  The output .npz holds the table under `arr` --
what simulate_pixels.py --light_lut_filename loads -- and beside it the fate counters (`fates`: absorbed in the bulk, at a wall,
truncated, per voxel), the raw tallies (`count`, `tsum`) and the run's parameters (`params`, JSON).  With --voxel_range the table
covers that slice of the linear voxel indices only (shape (n voxels, n detectors)): slices built by separate processes, on
several GPUs, concatenate to the table of one run, bit for bit.
"""
import argparse
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

TRUNCATED_WARN = 1e-3


def _length(s):
    v = float(s)
    if not v > 0:
        raise argparse.ArgumentTypeError(f"{s}: a length > 0 in cm (inf allowed)")
    return v


def _parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--geometry", required=True, metavar="FILE.json", help="box and detector rectangles")
    ap.add_argument("--vox_div", required=True, nargs=3, type=int, metavar=("NX", "NY", "NZ"), help="voxels along u, v, w")
    ap.add_argument("--photons", required=True, type=int, metavar="N", help="photons per voxel (1 .. 2^31 - 1)")
    ap.add_argument("--seed", type=int, default=0, metavar="S", help="seed of the keyed streams (default 0)")
    ap.add_argument("--rayleigh_cm", type=_length, default=math.inf, help="Rayleigh scattering length (default inf)")
    ap.add_argument("--absorption_cm", type=_length, default=math.inf, help="bulk absorption length (default inf)")
    ap.add_argument("--group_velocity_cm_ns", type=_length, default=13.4, help="default 13.4 (128 nm in LAr, literature)")
    ap.add_argument("--wall_reflectivity", type=float, nargs="+", default=[0.0], metavar="RHO",
                    help="diffuse reflectivity in [0, 1): one value for all walls or six (u0 u1 v0 v1 w0 w1); default 0")
    ap.add_argument("--emit", choices=("volume", "centre"), default="volume",
                    help="volume: uniformly in the voxel (nearest-voxel lookup); centre: at its centre (light_lut_interpolation "
                         "trilinear)")
    ap.add_argument("--max_steps", type=int, default=1000, help="steps after which a walk is truncated (default 1000)")
    ap.add_argument("--nprof", type=int, default=100, help="1 ns bins of the arrival-time profile (default 100)")
    ap.add_argument("--voxel_range", type=int, nargs=2, default=None, metavar=("BEGIN", "END"),
                    help="build the linear voxel indices [BEGIN, END) only")
    ap.add_argument("--output", required=True, metavar="LUT.npz")
    return ap


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    if any(v < 1 for v in a.vox_div):
        ap.error("--vox_div: three counts >= 1")
    if not 1 <= a.photons <= 2 ** 31 - 1:
        ap.error("--photons: 1 .. 2^31 - 1 per voxel")
    if len(a.wall_reflectivity) not in (1, 6):
        ap.error("--wall_reflectivity: one value or six")
    nvox = a.vox_div[0] * a.vox_div[1] * a.vox_div[2]
    if a.voxel_range is not None and not 0 <= a.voxel_range[0] <= a.voxel_range[1] <= nvox:
        ap.error(f"--voxel_range: 0 <= BEGIN <= END <= {nvox}")
    if not a.output.endswith(".npz"):
        ap.error("--output: an .npz file name")
    from larndsim_amd import lut_builder as LB
    try:
        geometry = LB.read(a.geometry)
        p = LB.params(a.rayleigh_cm, a.absorption_cm, a.group_velocity_cm_ns,
                      a.wall_reflectivity[0] if len(a.wall_reflectivity) == 1 else a.wall_reflectivity, a.emit, a.max_steps,
                      a.nprof)
    except (OSError, ValueError) as e:
        ap.error(str(e))

    import numpy as np
    from larndsim_amd import consts, lib
    if not len(consts.detector.TPC_BORDERS):
        consts.load_snapshot("module0")            # (the context wants some constants; the builder reads none of them)
    ctx = lib.context()                            # (device: LOCAL_RANK, or 0)
    t = LB.build(geometry, a.vox_div, a.photons, a.seed, p, a.voxel_range, ctx)
    ms = LB.build_ms(ctx)
    whole = t["voxel_range"] == (0, nvox)
    lut = LB.to_lut(t, a.vox_div if whole else None)
    n_walked = a.photons * len(t["count"])
    truncated = float(t["fates"][:, 2].sum()) / max(n_walked, 1)
    run = dict(p, vox_div=list(a.vox_div), photons=a.photons, seed=a.seed, voxel_range=list(t["voxel_range"]),
               box=[float(v) for v in geometry["box"]], n_detectors=len(geometry["detectors"]))
    np.savez(a.output, arr=lut, fates=t["fates"], count=t["count"], tsum=t["tsum"], params=np.array(json.dumps(run)))
    print(f"{len(t['count'])} voxels x {len(geometry['detectors'])} detectors, {a.photons} photons per voxel: "
          f"{ms:.1f} ms on the GPU ({n_walked / max(ms, 1e-9) / 1e3:.1f} M photons/s)")
    print(f"detected {float(t['count'].sum()) / max(n_walked, 1):.4f}, absorbed in the bulk "
          f"{float(t['fates'][:, 0].sum()) / max(n_walked, 1):.4f}, at a wall {float(t['fates'][:, 1].sum()) / max(n_walked, 1):.4f}, "
          f"truncated share {truncated:.3e}")
    if truncated > TRUNCATED_WARN:
        print(f"WARNING: {truncated:.3e} of the walks were cut off after {a.max_steps} steps (more than {TRUNCATED_WARN:g}): "
              "the table misses their light; raise --max_steps", file=sys.stderr)
    print(f"wrote {a.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
