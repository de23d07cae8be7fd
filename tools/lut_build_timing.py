"""The light LUT builder (ldsim_light_lut_build, csrc/kernels_lutbuild.hip) at the size of a module0 table: (14, 26, 8) voxels x
48 detectors (lut_builder.tile_wall, 6 x 4 tiles on each of the two v walls of module0's padded TPC box), 10^5 photons per voxel,
100 bins.

Two physics settings -- pure geometry (no scattering, black walls: one step per photon) and Rayleigh 60 cm with wall reflectivity
0.3 -- each as the median of 5 builds after 2 warm-ups (HIP-event time of lut_build_kernel, ldsim_light_lut_build_ms), with the
spread min .. max.  Photons/s is exact; steps/s uses the mean step count of a traced sample (ldsim_light_lut_trace, 4096 photons
from each of 16 voxels spread over the grid), since the build does not count steps.  Then, on the scattering setting: the effect
of lut_build_group_photons at 1024 and 16384 against the default 4096, and the LDS-tile path against the global-atomic path
(option lut_build_lds_tile 0).  Beside it, for scale: the numpy twin's photons/s on the host (20 000 photons of one voxel), and
the kernels' registers, scratch and occupancy as the compiler reports them (-Rpass-analysis=kernel-resource-usage on
kernels_lutbuild.hip with the Makefile's flags).
python tools/lut_build_timing.py [--photons N] [--repeats R] [--out FILE]   (default: profiles/lut_build_timing.log)"""
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

GRID, NPROF = (14, 26, 8), 100


def resource_usage():
    """{kernel: {VGPRs, ScratchSize, Occupancy, SGPRs, LDS}} of kernels_lutbuild.hip from the compiler's remarks"""
    src = os.path.join(REPO, "larnd-sim_amd", "csrc", "kernels_lutbuild.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "k.o")],
                           capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_Z\d+", "", m.group(1)).split("7LutGeom")[0].split("Pjmj")[0]
            out[name] = {}
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--photons", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lut_build_timing.log"))
    a = ap.parse_args(argv)
    import numpy as np
    from larndsim_amd import consts, lib
    from larndsim_amd import lut_builder as LB
    consts.load_snapshot("module0")
    ctx = lib.context()
    box = LB.box_from_consts(0)
    geo = {"box": box, "detectors": LB.tile_wall("v0", 6, 4, box, gap=0.3) + LB.tile_wall("v1", 6, 4, box, gap=0.3)}
    nvox = GRID[0] * GRID[1] * GRID[2]
    n_walked = nvox * a.photons
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(p, reps=a.repeats, warm=2):
        ms = []
        for k in range(warm + reps):
            t = LB.build(geo, GRID, a.photons, 1 + k, p, ctx=ctx)
            if k >= warm:
                ms.append(LB.build_ms(ctx))
        return ms, t

    def mean_steps(p):
        vox = np.linspace(0, nvox - 1, 16).astype(int)
        return float(np.mean([LB.trace(geo, GRID, int(v), (0, 4096), 1, p, ctx=ctx)["steps"].mean() for v in vox]))

    def report(name, ms, steps):
        med = float(np.median(ms))
        say(f"{name}: {med:.1f} ms ({min(ms):.1f} .. {max(ms):.1f}), {n_walked / med / 1e6:.2f} G photons/s, "
            f"{n_walked * steps / med / 1e6:.2f} G steps/s at {steps:.2f} steps per photon (traced sample)")
        return med

    say(f"light LUT build: box {box[0]:.2f} x {box[1]:.2f} x {box[2]:.2f} cm, grid {GRID}, {len(geo['detectors'])} detectors, "
        f"{a.photons} photons per voxel = {n_walked:.3e} walks, {NPROF} bins; median of {a.repeats} after 2 warm-ups")
    settings = {"pure geometry": LB.params(nprof=NPROF),
                "Rayleigh 60 cm, reflectivity 0.3": LB.params(rayleigh_cm=60, wall_reflectivity=0.3, nprof=NPROF)}
    for name, p in settings.items():
        ms, t = timed(p)
        steps = mean_steps(p)
        report(name, ms, steps)
        tot = float(n_walked)
        say(f"    detected {t['count'].sum() / tot:.4f}, absorbed at a wall {t['fates'][:, 1].sum() / tot:.4f}, truncated "
            f"{t['fates'][:, 2].sum() / tot:.2e}; lit cells {(t['count'] > 0).mean():.3f}")
    p = settings["Rayleigh 60 cm, reflectivity 0.3"]
    steps = mean_steps(p)
    try:
        for group in (1024, 4096, 16384):
            lib.set_option("lut_build_group_photons", group, ctx)
            report(f"  lut_build_group_photons {group}", timed(p)[0], steps)
        lib.set_option("lut_build_group_photons", 4096, ctx)
        for tile in (1, 0):
            lib.set_option("lut_build_lds_tile", tile, ctx)
            report("  LDS tile, non-zero cells flushed" if tile else "  global atomics per arrival", timed(p)[0], steps)
    finally:
        lib.set_option("lut_build_group_photons", 4096, ctx)
        lib.set_option("lut_build_lds_tile", 1, ctx)
    t0 = time.perf_counter()
    LB.trace_twin(geo, GRID, nvox // 2, (0, 20_000), 1, p)
    dt = time.perf_counter() - t0
    say(f"numpy twin on the host, one voxel: 20000 photons in {dt * 1e3:.0f} ms = {20_000 / dt / 1e6:.3f} M photons/s")
    for k, v in resource_usage().items():
        say(f"{k}: " + ", ".join(f"{a_} {b_}" for a_, b_ in v.items()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
