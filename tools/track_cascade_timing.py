"""The track cascade (ldsim_track_cascade, csrc/kernels_trackgen.hip cas_kernel) on the track generator's two timing workloads in
module0's world box (tools/track_gen_timing.py: 1 GeV muons crossing from the top; 100 MeV muons stopping, isotropic from a TPC's
centre), delta rays above t_track as tracks, decays on, up to four generations, steps of 0.1 cm.

Per generation and in total: particles, segments, secondaries and the write pass's HIP-event time (cas_kernel<true>,
ldsim_track_cascade_ms) as the median of 5 cascades after 2 warm-ups, a new seed every cascade, with the spread min .. max.  Beside
it, measured in the same run on the same primaries: the track generator's own write pass (gen_kernel<true>, which deposits the
delta rays in the parent's segments), the ratio of the two, and the kernels' registers, scratch and occupancy as the compiler
reports them.
python tools/track_cascade_timing.py [--primaries N] [--repeats R] [--t_track MEV] [--out FILE]
(default: 16384 primaries, t_track 1 MeV, profiles/track_cascade_timing.log)"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tools")):
    sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--primaries", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--t_track", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_cascade_timing.log"))
    a = ap.parse_args(argv)
    import numpy as np
    from larndsim_amd import consts, lib
    from larndsim_amd import track_cascade as TC, track_generator as TG
    from track_gen_timing import resource_usage
    consts.load_snapshot("module0")
    ctx = lib.context()
    world = TG.default_world()
    p = TG.params(world)
    cp = TC.cascade_params(t_track=a.t_track, decays=True, max_generations=4)
    c = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[0].mean(axis=1)
    n, warm = a.primaries, 2
    top = TG.cosmic_primaries(world, 1000.0, 8, (n + 7) // 8, 1)[:n]
    top["dir"] = [0.0, -1.0, 0.0]
    workloads = {"crossing (1 GeV muons, top to bottom)": top,
                 "stopping (100 MeV muons from a TPC's centre)": TG.gun_primaries(13, [c[2], c[1], c[0]], None, 100.0, 8, (n + 7) // 8, 1)[:n]}
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def spread(v):
        return f"{float(np.median(v)):.2f} ms ({min(v):.2f} .. {max(v):.2f})"

    say(f"track cascade: world box {np.round(world[0], 2).tolist()} .. {np.round(world[1], 2).tolist()} cm, {n} primaries, step "
        f"{p['step']} cm, t_cut {p['t_cut']} MeV, t_track {cp['t_track']} MeV, decays on, at most {cp['max_generations']} generations; "
        f"median of {a.repeats} after {warm} warm-ups, a new seed every pass")
    for name, prim in workloads.items():
        part = TC.particles(prim)
        ms, rows, old = [], None, []
        for k in range(warm + a.repeats):
            per, gens, cur = [], [], part
            for g in range(cp["max_generations"]):
                out = TC.walk_generation(cur, p, cp, 1 + k, g + 1 < cp["max_generations"], ctx)
                per.append(TC.walk_generation_ms(ctx))
                gens.append((len(cur), len(out["dx"]), len(out["secondaries"])))
                cur = out["secondaries"]
                if not len(cur):
                    break
            TG.generate(prim, p, 1 + k, ctx)
            if k >= warm:
                ms.append(per)
                old.append(TG.generate_ms(ctx))
                rows = gens
        depth = min(len(m) for m in ms)
        say(f"{name}:")
        for g in range(depth):
            say(f"    generation {g}: {rows[g][0]} particles, {rows[g][1]} segments, {rows[g][2]} secondaries (last pass), write pass "
                + spread([m[g] for m in ms]))
        tot = [sum(m) for m in ms]
        say(f"    all generations: {sum(r[0] for r in rows)} particles, {sum(r[1] for r in rows)} segments, write passes " + spread(tot))
        say(f"    the track generator on the same primaries (delta rays deposited in the parent's segments): write pass " + spread(old))
        say(f"    ratio cascade / generator: {float(np.median(tot)) / float(np.median(old)):.2f} in total, "
            f"{float(np.median([m[0] for m in ms])) / float(np.median(old)):.2f} for generation 0 alone")
    for k, v in resource_usage().items():
        say(f"{k}: " + ", ".join(f"{a_} {b_}" for a_, b_ in v.items()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
