#!/usr/bin/env python
"""
build_field_map.py -- build a drift-field map from a space-charge density and wall potentials
(larndsim_amd/field_map_builder.py).

  build_field_map.py --config module0 --output field_map.npz                          # cosmic-ray space charge, every TPC
  build_field_map.py --config module0 --tpc 0 --pitch 0.5 --cosmic_rate 4e-16 --output field_map.npz
  build_field_map.py --config module0 --density rho.npz --boundary walls.npz --output field_map.npz
  build_field_map.py --config module0 --twin --output field_map.npz                   # numpy on the host, no GPU

The model: every TPC is a box with a node grid of about --pitch cm whose outer nodes lie on the walls.  The total field is the
nominal one plus -grad psi, laplace psi = -rho / eps inside, psi given on the six walls (0: conducting anode and cathode and an
ideally graded field cage; --boundary: anything else, a cage defect).  Electrons follow -mu(|E|) E from every node to the anode
(RK4, largest step --step); the map holds |E| at the node, where the path ends (dx, dy) and the shift of the equivalent drift
coordinate (dz).  Not modelled: the ions' effect on their own density, time dependence, dielectric walls, coupling between TPCs
through the cathode, changes of the diffusion along the path.

The source is the steady-state space charge of cosmic rays, rho(q) = rate q / (ion mobility E0), q the distance from the anode
(--cosmic_rate in C/cm^3/s, --ion_mobility in cm^2/V/s; the defaults are literature values for a detector at the surface,
parameters and no claims), or --density: an .npz with one array tpc<i>_rho (C/cm^3, [nx][ny][nz] of the TPC's grid) per TPC.
--boundary: an .npz with tpc<i>_psi (kV, same shape; only the wall nodes are read).  A TPC without an entry has no charge / walls
at 0.  The output is the .npz that simulate_pixels.py --field_map loads.
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from build_response import _load_constants  # noqa: E402  (the same constants options)


def _parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="module0", help="configuration keyword (default module0)")
    ap.add_argument("--config_root", default=None, help="larnd-sim tree holding config/config.yaml and the YAML families "
                                                        "(default: $LARNDSIM_ROOT, else the built-in snapshot keywords)")
    for k in ("pixel_layout", "detector_properties", "simulation_properties"):
        ap.add_argument("--" + k, default=None, help="YAML file (all three together, instead of the keyword's)")
    ap.add_argument("--tpc", type=int, action="append", default=None, help="TPC to build a map for (repeatable; default: all)")
    ap.add_argument("--pitch", type=float, default=1.0, metavar="CM", help="node pitch aimed at (default 1 cm)")
    ap.add_argument("--cosmic_rate", type=float, default=None, metavar="C/CM3/S",
                    help="ion charge cosmic rays leave per volume and time (default 2e-16, a literature value)")
    ap.add_argument("--ion_mobility", type=float, default=None, metavar="CM2/V/S",
                    help="mobility of the positive ions (default 1.6e-3, a literature value)")
    ap.add_argument("--density", default=None, metavar="FILE.npz", help="charge density per TPC instead of the cosmic profile")
    ap.add_argument("--boundary", default=None, metavar="FILE.npz", help="wall potentials per TPC (default 0)")
    ap.add_argument("--tol", type=float, default=1e-12, help="relative residual the solve ends at (default 1e-12)")
    ap.add_argument("--step", type=float, default=None, metavar="CM", help="largest RK4 step along the drift (default hz / 2)")
    ap.add_argument("--twin", action="store_true", help="build with the numpy restatement on the host: no GPU is touched")
    ap.add_argument("--output", required=True, metavar="field_map.npz")
    return ap


def _entry(ap, path, key, p):
    """array `key` of the .npz `path`, or None"""
    import numpy as np
    try:
        with np.load(path, allow_pickle=False) as f:
            return np.asarray(f[key], dtype=np.float64) if key in f.files else None
    except (OSError, ValueError) as e:
        ap.error(f"{path}: {e}")


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    if not a.output.endswith(".npz"):
        ap.error("--output: an .npz file name")
    if a.density is not None and (a.cosmic_rate is not None or a.ion_mobility is not None):
        ap.error("--density and --cosmic_rate / --ion_mobility exclude each other")
    _load_constants(ap, a)
    import numpy as np
    from larndsim_amd import consts, field_map, field_map_builder as FB
    n_tpc = len(consts.detector.TPC_BORDERS)
    tpcs = sorted(set(a.tpc)) if a.tpc else list(range(n_tpc))
    ctx = None
    if not a.twin:
        from larndsim_amd import lib
        ctx = lib.context()                        # (device: LOCAL_RANK, or 0)
    maps = {}
    for tpc in tpcs:
        try:
            p = FB.params(**FB.box_from_consts(tpc, a.pitch), tol=a.tol, step=a.step)
            if a.density is not None:
                rho = _entry(ap, a.density, f"tpc{tpc}_rho", p)
                source = np.zeros(p["dims"]) if rho is None else FB.source_from_density(FB._array(p, rho, f"tpc{tpc}_rho"))
            else:
                source = FB.cosmic_source(p, FB.COSMIC_ION_RATE if a.cosmic_rate is None else a.cosmic_rate,
                                          FB.ION_MOBILITY if a.ion_mobility is None else a.ion_mobility)
            boundary = None if a.boundary is None else _entry(ap, a.boundary, f"tpc{tpc}_psi", p)
            info = {}
            t0 = time.perf_counter()
            if a.twin:
                m = FB.build_twin(p, source, boundary, info=info)
                how = f"{time.perf_counter() - t0:.2f} s in numpy (direct solve)"
            else:
                m = FB.build(p, source, boundary, ctx, info=info)
                ms = FB.build_ms(ctx)
                how = f"{info['iterations']} iterations; solve {ms[0]:.2f} ms, field {ms[1]:.3f} ms, trace {ms[2]:.2f} ms on the GPU"
        except (FB.FieldMapBuildError, RuntimeError) as e:     # (RuntimeError: the library's refusals, lib.LdsimError)
            ap.error(f"TPC {tpc}: {e}")
        maps[tpc] = m
        r = m["E"] / p["E0"]
        print(f"TPC {tpc}: {p['dims'][0]} x {p['dims'][1]} x {p['dims'][2]} nodes, drift direction n = {FB.drift_sign(p):+.0f}, "
              f"relative residual {info['residual']:.3e}, {how}")
        print(f"TPC {tpc}: E / E0 {r.min():.6f} .. {r.max():.6f}; dx {m['dx'].min():+.4f} .. {m['dx'].max():+.4f} cm, "
              f"dy {m['dy'].min():+.4f} .. {m['dy'].max():+.4f} cm, dz {m['dz'].min():+.4f} .. {m['dz'].max():+.4f} cm; "
              f"{int(info['flags'].sum())} nodes whose charge reaches the field cage")
    field_map.validate(maps, n_tpc)
    field_map.save(a.output, maps)
    print(f"wrote {a.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
