"""The track generator (ldsim_track_gen, csrc/kernels_trackgen.hip) on two workloads in module0's world box (the TPCs' hull plus
10 cm), straggling and scattering on, steps of 0.1 cm:

* crossing: 1 GeV muons from the top face, straight down -- every walk leaves through the bottom, some 1500 segments each;
* stopping: 100 MeV muons from the centre of the first TPC, isotropic -- every walk ends inside, some 350 segments each.

Each as the median of 5 write passes after 2 warm-ups (HIP-event time of gen_kernel<true>, ldsim_track_gen_ms; a new seed every
pass, so the count pass runs every time and its wall time is given beside it), with the spread min .. max: primaries/s and
segments/s.  Then the effect of track_gen_group_primaries on the stopping workload.  Beside it, for scale: the numpy twin's rate
on the host (256 primaries of each workload), and the kernels' registers, scratch and occupancy as the compiler reports them
(-Rpass-analysis=kernel-resource-usage on kernels_trackgen.hip with the Makefile's flags).
python tools/track_gen_timing.py [--primaries N] [--repeats R] [--workload both|crossing|stopping] [--out FILE]
(default: 16384 primaries, both workloads, profiles/track_gen_timing.log)"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO):
    sys.path.insert(0, p)


def resource_usage():
    """{kernel: {VGPRs, ScratchSize, Occupancy, ..}} of kernels_trackgen.hip from the compiler's remarks"""
    src = os.path.join(REPO, "larnd-sim_amd", "csrc", "kernels_trackgen.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "k.o")],
                           capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            kernel = "cas_kernel" if "cas_kernel" in m.group(1) else "gen_kernel"
            name = kernel + "<true>" if "ILb1E" in m.group(1) else kernel + "<false>" if "ILb0E" in m.group(1) else m.group(1)
            out[name] = {}
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--primaries", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workload", choices=("both", "crossing", "stopping"), default="both",
                    help="a larger --primaries fits the host's memory with the stopping workload alone (136 bytes per segment)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_gen_timing.log"))
    a = ap.parse_args(argv)
    import numpy as np
    from larndsim_amd import consts, lib
    from larndsim_amd import track_generator as TG
    consts.load_snapshot("module0")
    ctx = lib.context()
    world = TG.default_world()
    p = TG.params(world)
    lo, hi = np.array(world[0]), np.array(world[1])
    c = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[0].mean(axis=1)
    n = a.primaries
    ev, tr = np.arange(n) // 8, np.arange(n) % 8
    top = TG.cosmic_primaries(world, 1000.0, 8, (n + 7) // 8, 1)[:n]
    top["dir"] = [0.0, -1.0, 0.0]
    workloads = {"crossing (1 GeV muons, top to bottom)": top,
                 "stopping (100 MeV muons from a TPC's centre)": TG.gun_primaries(13, [c[2], c[1], c[0]], None, 100.0, 8, (n + 7) // 8, 1)[:n]}
    assert (top["event_id"] == ev).all() and (top["track_in_event"] == tr).all()
    if a.workload != "both":
        workloads = {k: v for k, v in workloads.items() if k.startswith(a.workload)}
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(prim, reps=a.repeats, warm=2):
        ms, wall, g = [], [], None
        for k in range(warm + reps):
            t0 = time.perf_counter()
            cnt = TG.count(prim, p, 1 + k, ctx)
            t1 = time.perf_counter()
            g = TG.generate(prim, p, 1 + k, ctx)
            if k >= warm:
                ms.append(TG.generate_ms(ctx))
                wall.append((t1 - t0) * 1e3)
            assert np.array_equal(cnt["counts"], g["counts"])
        return ms, wall, g

    def report(name, prim, ms, wall, g):
        med, nseg = float(np.median(ms)), len(g["dx"])
        st = g["end_state"]
        say(f"{name}: write pass {med:.2f} ms ({min(ms):.2f} .. {max(ms):.2f}), {len(prim) / med / 1e3:.3f} M primaries/s, "
            f"{nseg / med / 1e3:.1f} M segments/s; {nseg / len(prim):.1f} segments per primary ({g['counts'].min()} .. "
            f"{g['counts'].max()}); count pass with upload, scan and download {float(np.median(wall)):.2f} ms of wall time")
        say(f"    stopped {int((st == TG.STOPPED).sum())}, left the box {int((st == TG.EXITED).sum())}, truncated "
            f"{int((st == TG.TRUNCATED).sum())}; {nseg * 136 / med / 1e6:.1f} GB/s of column stores (15 f64 + 4 i32 per segment)")

    say(f"track generator: world box {np.round(lo, 2).tolist()} .. {np.round(hi, 2).tolist()} cm, {n} primaries, step {p['step']} cm, "
        f"t_cut {p['t_cut']} MeV, straggling and scattering on; median of {a.repeats} after 2 warm-ups")
    for name, prim in workloads.items():
        report(name, prim, *timed(prim))
    stop = workloads.get("stopping (100 MeV muons from a TPC's centre)")
    try:
        for group in (64, 256, 1024, 4096) if stop is not None else ():
            lib.set_option("track_gen_group_primaries", group, ctx)
            report(f"  stopping, track_gen_group_primaries {group}", stop, *timed(stop))
    finally:
        lib.set_option("track_gen_group_primaries", 0, ctx)
    for name, prim in workloads.items():
        t0 = time.perf_counter()
        g = TG.generate_twin(prim[:256], p, 1)
        dt = time.perf_counter() - t0
        say(f"numpy twin on the host, {name}: 256 primaries, {len(g['dx'])} segments in {dt:.2f} s = {256 / dt:.0f} primaries/s, "
            f"{len(g['dx']) / dt / 1e3:.1f} k segments/s")
    for k, v in resource_usage().items():
        say(f"{k}: " + ", ".join(f"{a_} {b_}" for a_, b_ in v.items()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
