#!/usr/bin/env python
"""
build_response.py -- build a pixel field-response table by the Shockley-Ramo theorem (larndsim_amd/response_builder.py).

  build_response.py --config module0 --output response.npy
  build_response.py --config module0 --pad_size 0.35 --n_sub 8 --shape 45 45 1950 --output response.npy
  build_response.py --config module0 --twin --output response.npy          # numpy on the host, no GPU

The model: the anode is the plane z = 0, the pixel a square pad of side --pad_size (default: the pixel pitch) centred on its pitch
cell, all the rest of the plane grounded, the cathode far away, the drift field uniform.  The pad's weighting potential is the
solid angle it subtends over 2 pi; a table entry is the tick average of the current a unit charge induces while it drifts
straight down at V_DRIFT, averaged over --n_sub x --n_sub start points of the transverse bin.  The charge lands at the upper
edge of tick --arrival_tick (default floor(TIME_WINDOW / RESPONSE_SAMPLING) - 1, the last tick tracks_current reads for every
sub-tick phase).  With --pad_size below the pitch the charge that lands on the gaps between the pads is lost: field focusing
onto the pads is not modelled.

PIXEL_PITCH, RESPONSE_BIN_SIZE, V_DRIFT, RESPONSE_SAMPLING and TIME_WINDOW come from --config (a keyword) or from the three YAML
files.  The output is an .npy file of shape (I, J, K), f64: what simulate_pixels.py --response_file loads.
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="module0", help="configuration keyword (default module0)")
    ap.add_argument("--config_root", default=None, help="larnd-sim tree holding config/config.yaml and the YAML families "
                                                        "(default: $LARNDSIM_ROOT, else the built-in snapshot keywords)")
    for k in ("pixel_layout", "detector_properties", "simulation_properties"):
        ap.add_argument("--" + k, default=None, help="YAML file (all three together, instead of the keyword's)")
    ap.add_argument("--pad_size", type=float, default=None, metavar="CM",
                    help="side of the square pad in (0, PIXEL_PITCH] (default: the pitch; below it the charge over the gaps is lost)")
    ap.add_argument("--n_sub", type=int, default=4, help="sub-samples per transverse bin and axis, 1 .. 16 (default 4)")
    ap.add_argument("--shape", type=int, nargs=3, default=None, metavar=("I", "J", "K"),
                    help="bins along x, y and ticks (default 45 45 1950 at RESPONSE_SAMPLING >= 0.1 us, else 45 45 3800)")
    ap.add_argument("--arrival_tick", type=int, default=None,
                    help="tick at whose upper edge the charge lands (default floor(TIME_WINDOW / RESPONSE_SAMPLING) - 1)")
    ap.add_argument("--twin", action="store_true", help="build with the numpy restatement on the host: no GPU is touched")
    ap.add_argument("--output", required=True, metavar="response.npy")
    return ap


def _load_constants(ap, a):
    from larndsim_amd import config as cfgmod, consts
    files = (a.detector_properties, a.pixel_layout, a.simulation_properties)
    if any(files) and not all(files):
        ap.error("--pixel_layout, --detector_properties and --simulation_properties must be given together")
    try:
        if all(files):
            consts.load_properties(a.detector_properties, a.pixel_layout, a.simulation_properties)
            return
        cfg = cfgmod.get_config(a.config, a.config_root)
    except (KeyError, OSError) as e:
        ap.error(str(e.args[0] if isinstance(e, KeyError) else e))
    snapshot = cfg.get("SNAPSHOT")
    if snapshot is not None:
        consts.load_snapshot(snapshot[0] if isinstance(snapshot, list) else snapshot)
    else:
        layout = cfg["PIXEL_LAYOUT"]
        consts.load_properties(cfg["DET_PROPERTIES"], layout[0] if isinstance(layout, list) else layout, cfg["SIM_PROPERTIES"])


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    if not a.output.endswith(".npy"):
        ap.error("--output: an .npy file name")
    _load_constants(ap, a)
    import numpy as np
    from larndsim_amd import response_builder as RB
    try:
        p = RB.params(pad_size=a.pad_size, n_sub=a.n_sub, shape=a.shape, arrival_tick=a.arrival_tick)
    except RB.ResponseBuildError as e:
        ap.error(str(e))
    if a.twin:
        t0 = time.perf_counter()
        table = RB.twin(p)
        how = f"{time.perf_counter() - t0:.2f} s in numpy"
    else:
        from larndsim_amd import lib
        ctx = lib.context()                        # (device: LOCAL_RANK, or 0)
        table = RB.build(p, ctx)
        how = f"{RB.build_ms(ctx):.2f} ms on the GPU"
    np.save(a.output, table)
    dt, n = p["sampling"], RB.bins_over_pad(p)
    closure = table.sum(axis=-1) * dt
    print(f"({p['n_i']}, {p['n_j']}, {p['n_k']}) table, pad {p['pad_size']:g} cm of pitch {p['pitch']:g} cm, n_sub {p['n_sub']}, "
          f"arrival tick {p['arrival_tick']}: {how}")
    over = closure[:n, :n]
    print(f"peak {np.abs(table).max():.4g} per us; charge collected per unit charge: "
          + (f"{over.min():.6f} .. {over.max():.6f} over the pad ({n} x {n} bins), " if over.size else "")
          + f"{closure.min():.3e} at the least")
    if p["pad_size"] < p["pitch"]:
        print(f"pad_size {p['pad_size']:g} cm < pitch {p['pitch']:g} cm: charge over the gaps is lost (no field focusing)")
    print(f"wrote {a.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
