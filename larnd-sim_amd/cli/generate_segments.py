#!/usr/bin/env python
"""
generate_segments.py -- make an edep-sim style input file by transporting muons, pions or protons through liquid argon
(larndsim_amd/track_generator.py).

  generate_segments.py --config module0 --source gun --pdg 13 --energy 100 --position 10 0 0 --direction 0 -1 0 \\
                       --tracks_per_event 8 --n_events 2 --seed 1 --output muons.npz
  generate_segments.py --config module0 --source gun --pdg 2212 --energy 30 200 --isotropic --n_events 100 --output protons.npz
  generate_segments.py --config module0 --source cosmics --energy 1000 100000 --tracks_per_event 5 --n_events 10 --output cosmics.h5
  generate_segments.py --config module0 --source gun --twin --output muons.npz        # numpy on the host, no GPU
  generate_segments.py --config module0 --source gun --pdg -13 --energy 100 --secondaries --decays --output michel.npz

The model: heavy charged particles (pdg 13, -13, 211, -211, 2212) in uniform LAr inside a world box -- the hull of the
configuration's TPCs plus --margin cm --, Bethe energy loss with restricted mean below --t_cut, Gaussian soft fluctuation and
sampled hard collisions above it (--no_straggling: the mean alone), Highland multiple scattering (--no_mcs: straight tracks), one
segment per step of at most --step cm.  Not modelled: decays, hadronic interactions, bremsstrahlung, separate delta-ray tracks.
Positions, directions and the output are in the input file's frame (the drift axis in x, y vertical): what simulate_pixels.py
reads.  Every number is a pure function of the primaries, the parameters and --seed.

--secondaries (larndsim_amd/track_cascade.py): hard collisions from --t_track MeV on leave the parent's segment as delta-ray
electrons with tracks of their own, electrons (--pdg 11, -11) are transported under Moller loss and collisions, and with --decays
a stopped muon emits its Michel electron (mu- only where it is not captured: --capture_fraction, --mu_minus_lifetime).  What is
emitted is walked in turn, for at most --max_generations generations; `trajectories` then has one row per particle with
`parent_id` pointing at the parent's row.  Still not modelled: pion decay, capture products, bremsstrahlung, photons,
annihilation, polarisation -- a Michel electron loses energy by collisions only and travels further than a real one.

The output holds `segments`, `trajectories` (one row per primary) and `vertices` (one row per event): HDF5 when h5py is
importable and the name does not end in .npz, else an .npz with the same dataset names (simulate_pixels.py reads both).
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
    ap.add_argument("--source", choices=("gun", "cosmics"), default="gun")
    ap.add_argument("--pdg", type=int, default=13, help="13, -13, 211, -211 or 2212 (default 13); 11 and -11 only together with --secondaries")
    ap.add_argument("--energy", type=float, nargs="+", default=None, metavar="MEV",
                    help="kinetic energy: one value, or LOW HIGH for a log-uniform draw (default: gun 100, cosmics 1000 100000)")
    ap.add_argument("--position", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="gun: start point, file frame, cm (default: the centre of the first TPC)")
    ap.add_argument("--direction", type=float, nargs=3, default=None, metavar=("DX", "DY", "DZ"),
                    help="gun: direction, file frame (default 0 -1 0: downwards)")
    ap.add_argument("--isotropic", action="store_true", help="gun: isotropic directions instead of --direction")
    ap.add_argument("--tracks_per_event", type=int, default=1)
    ap.add_argument("--n_events", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0, help="seed of the keyed streams (default 0)")
    ap.add_argument("--margin", type=float, default=10.0, metavar="CM", help="world box: the TPCs' hull plus this (default 10)")
    ap.add_argument("--step", type=float, default=0.1, metavar="CM", help="largest step = segment length (default 0.1)")
    ap.add_argument("--t_cut", type=float, default=0.1, metavar="MEV", help="collisions above it are sampled singly (default 0.1)")
    ap.add_argument("--max_steps", type=int, default=100000, help="steps after which a walk is truncated (default 100000)")
    ap.add_argument("--no_straggling", action="store_true", help="mean energy loss only")
    ap.add_argument("--no_mcs", action="store_true", help="no multiple scattering")
    ap.add_argument("--secondaries", action="store_true",
                    help="delta rays above --t_track as tracks of their own, electrons transported (allows --pdg 11, -11)")
    ap.add_argument("--t_track", type=float, default=1.0, metavar="MEV",
                    help="--secondaries: hard collisions from here on become tracks (default 1; at least --t_cut and 0.5)")
    ap.add_argument("--decays", action="store_true", help="--secondaries: stopped muons emit their Michel electron")
    ap.add_argument("--max_generations", type=int, default=4,
                    help="--secondaries: generations walked; the last one emits nothing (default 4)")
    ap.add_argument("--capture_fraction", type=float, default=0.76,
                    help="--decays: fraction of stopped mu- captured in argon, which emit nothing (default 0.76)")
    ap.add_argument("--mu_minus_lifetime", type=float, default=0.537, metavar="US",
                    help="--decays: lifetime of a stopped mu- in argon (default 0.537)")
    ap.add_argument("--twin", action="store_true", help="walk with the numpy restatement on the host: no GPU is touched")
    ap.add_argument("--output", required=True, metavar="FILE", help=".h5 / .hdf5 (needs h5py) or .npz")
    return ap


def _write(path, datasets):
    """HDF5 when h5py is importable and the name allows it, else .npz with the same dataset names; returns the name written"""
    import numpy as np
    h5py = None
    if not path.endswith(".npz"):
        try:
            import h5py
        except ImportError:
            path = os.path.splitext(path)[0] + ".npz"
            print(f"h5py is not importable: writing {path} instead", file=sys.stderr)
    if h5py is not None:
        with h5py.File(path, "w") as f:
            for k, v in datasets.items():
                f.create_dataset(k, data=v)
    else:
        np.savez(path, **datasets)
    return path


def _cascade(a, prim, p):
    """--secondaries: the generations of the primaries (track_cascade.cascade / cascade_twin) to the same three datasets"""
    import numpy as np
    from larndsim_amd import track_cascade as TC, track_generator as TG
    cp = TC.cascade_params(t_track=a.t_track, decays=a.decays, max_generations=a.max_generations,
                           capture_fraction=a.capture_fraction, mu_minus_lifetime=a.mu_minus_lifetime)
    t0 = time.perf_counter()
    if a.twin:
        gens = TC.cascade_twin(prim, p, cp, a.seed)
        how = f"{time.perf_counter() - t0:.2f} s in numpy"
    else:
        from larndsim_amd import lib
        gens = TC.cascade(prim, p, cp, a.seed, lib.context())
        how = f"{time.perf_counter() - t0:.2f} s with the walks on the GPU"
    seg, traj, vert = TC.to_datasets(gens)
    st = traj["end_state"]
    proc = np.concatenate([g["particles"]["process"] for g in gens])
    print(f"{len(prim)} primaries in {len(vert)} events -> {len(traj)} particles in {len(gens)} generations "
          f"({int((proc == TC.DELTA_RAY).sum())} delta rays, {int((proc == TC.DECAY).sum())} decay electrons), {len(seg)} segments "
          f"({how}): {int((st == TG.STOPPED).sum())} stopped, {int((st == TG.EXITED).sum())} left the world box, "
          f"{int((st == TG.TRUNCATED).sum())} truncated after {p['max_steps']} steps")
    if (st == TG.TRUNCATED).any():
        print("WARNING: truncated walks miss the rest of their track; raise --max_steps", file=sys.stderr)
    print(f"deposited {float(seg['dE'].astype(np.float64).sum()):.3f} MeV over {float(seg['dx'].astype(np.float64).sum()):.2f} cm")
    print(f"wrote {_write(a.output, {'segments': seg, 'trajectories': traj, 'vertices': vert})}")
    return 0


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    if a.energy is not None and len(a.energy) not in (1, 2):
        ap.error("--energy: one value, or LOW HIGH")
    if a.source == "cosmics" and (a.position or a.direction or a.isotropic):
        ap.error("--position, --direction and --isotropic belong to --source gun")
    if a.isotropic and a.direction:
        ap.error("--isotropic and --direction exclude each other")
    if a.decays and not a.secondaries:
        ap.error("--decays belongs to --secondaries")
    _load_constants(ap, a)
    import numpy as np
    from larndsim_amd import consts, track_generator as TG
    try:
        world = TG.default_world(a.margin)
        p = TG.params(world, step=a.step, t_cut=a.t_cut, straggling=not a.no_straggling, mcs=not a.no_mcs, max_steps=a.max_steps,
                      min_step=min(1e-4, a.step))
        if a.source == "gun":
            e = a.energy or [100.0]
            if a.position is None:
                b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[0].mean(axis=1)
                a.position = [float(b[2]), float(b[1]), float(b[0])]
            prim = TG.gun_primaries(a.pdg, a.position, None if a.isotropic else (a.direction or [0.0, -1.0, 0.0]),
                                    e[0] if len(e) == 1 else e, a.tracks_per_event, a.n_events, a.seed)
        else:
            e = a.energy or [1000.0, 100000.0]
            prim = TG.cosmic_primaries(world, e[0] if len(e) == 1 else e, a.tracks_per_event, a.n_events, a.seed, pdg=a.pdg)
        t0 = time.perf_counter()
        if a.secondaries:
            return _cascade(a, prim, p)
        if a.twin:
            gen = TG.generate_twin(prim, p, a.seed)
            how = f"{time.perf_counter() - t0:.2f} s in numpy"
        else:
            from larndsim_amd import lib
            ctx = lib.context()                    # (device: LOCAL_RANK, or 0)
            gen = TG.generate(prim, p, a.seed, ctx)
            how = f"write pass {TG.generate_ms(ctx):.3f} ms on the GPU"
    except (TG.TrackGenError, RuntimeError) as e:          # (RuntimeError: the library's refusals, lib.LdsimError)
        ap.error(str(e))
    seg, traj, vert = TG.to_datasets(prim, gen)
    st = np.asarray(gen["end_state"])
    print(f"{len(prim)} primaries in {len(vert)} events -> {len(seg)} segments ({how}): "
          f"{int((st == TG.STOPPED).sum())} stopped, {int((st == TG.EXITED).sum())} left the world box, "
          f"{int((st == TG.TRUNCATED).sum())} truncated after {p['max_steps']} steps")
    if (st == TG.TRUNCATED).any():
        print("WARNING: truncated walks miss the rest of their track; raise --max_steps", file=sys.stderr)
    print(f"deposited {float(seg['dE'].astype(np.float64).sum()):.3f} MeV over {float(seg['dx'].astype(np.float64).sum()):.2f} cm")
    print(f"wrote {_write(a.output, {'segments': seg, 'trajectories': traj, 'vertices': vert})}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
