"""The drift-field map builder (ldsim_field_map_solve / _trace, csrc/kernels_fmapbuild.hip) on module0's box at 1 cm pitch,
63 x 125 x 31 nodes, under the cosmic-ray space charge: HIP-event times of the solve, the field kernel and the trace kernel as the
median of 5 builds after 2 warm-ups (min .. max), the iterations used and the time per iteration, and the solve again at
fmap_build_wgs 1 and 7 (the same bytes).  Beside it the wall time of the numpy twin's direct solve and paths on the same machine.
With --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 20 --warmup 5 on this tree and on the parent,
alternating in fresh processes, twice each; the builder is not in the flagship workload, so the expectation is no difference
beyond the parent runs' own spread.
python tools/field_map_build_timing.py [--repeats R] [--out FILE] [--parent DIR [--ab_out FILE]]
  (defaults: profiles/field_map_build_timing.log, profiles/field_map_build_bench_ab.log)"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO):
    sys.path.insert(0, p)


def _bench(tree):
    """the JSON result line of bench.py run in `tree`, in a fresh process"""
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, env=env,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} ended with {r.returncode}: {r.stderr[-1500:]}")
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError(f"bench.py in {tree} printed no JSON line")


def bench_ab(parent, out):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("python bench.py --gpus 1 --steps 20 --warmup 5, fresh processes alternating: this tree (with the drift-field map builder), "
        "the parent commit's tree, twice each; the builder is not part of the workload")
    res = {"this": [], "parent": []}
    for rep in range(2):
        for name, tree in (("this", REPO), ("parent", parent)):
            j = _bench(tree)
            res[name].append(j)
            say(f"run {rep + 1} {name:6s}: {j['ms_per_step']:.3f} ms per step, {j['value']:.0f} {j['unit']}")
    numeric = [k for k, v in res["this"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)
               and all(isinstance(r.get(k), (int, float)) for r in res["this"] + res["parent"])]
    for k in numeric:
        a, b = [r[k] for r in res["this"]], [r[k] for r in res["parent"]]
        if a[0] == a[1] == b[0] == b[1]:
            continue
        say(f"{k}: this {a[0]:.6g}, {a[1]:.6g}; parent {b[0]:.6g}, {b[1]:.6g}; difference of the means "
            f"{(sum(a) - sum(b)) / 2:+.4g}, the parent's own spread {abs(b[0] - b[1]):.4g}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "field_map_build_timing.log"))
    ap.add_argument("--parent", default=None, help="built checkout of the parent commit, for the bench.py A/B")
    ap.add_argument("--ab_out", default=os.path.join(REPO, "profiles", "field_map_build_bench_ab.log"))
    ap.add_argument("--ab_only", action="store_true", help="skip the builder's timing")
    a = ap.parse_args(argv)
    if not a.ab_only:
        import numpy as np
        from larndsim_amd import consts, field_map_builder as FB, lib
        consts.load_snapshot("module0")
        ctx = lib.context()
        lines = []

        def say(s=""):
            print(s, flush=True)
            lines.append(s)

        p = FB.params(**FB.box_from_consts(0, 1.0))
        s = FB.cosmic_source(p)
        ms, it, res = [], 0, 0.0
        for k in range(2 + a.repeats):
            info = {}
            m = FB.build(p, s, ctx=ctx, info=info)
            it, res = info["iterations"], info["residual"]
            if k >= 2:
                ms.append(FB.build_ms(ctx))
        ms = np.asarray(ms)
        med = np.median(ms, axis=0)
        nodes = int(np.prod(p["dims"]))
        steps = int(sum(max(1, int(np.ceil(q / p["step"]))) for q in FB.drift_coordinate(p) if q > 0)) * p["dims"][0] * p["dims"][1]
        say(f"module0 TPC 0, {p['dims'][0]} x {p['dims'][1]} x {p['dims'][2]} = {nodes} nodes, cosmic profile, tol {p['tol']:.0e}, "
            f"check_every {p['check_every']}, step {p['step']:.4f} cm; median of {a.repeats} after 2 warm-ups (min .. max)")
        say(f"solve: {med[0]:.3f} ms ({ms[:, 0].min():.3f} .. {ms[:, 0].max():.3f}), {it} iterations, {med[0] * 1e3 / max(it, 1):.2f} us per "
            f"iteration (two launches), relative residual {res:.3e}")
        say(f"field: {med[1]:.4f} ms ({ms[:, 1].min():.4f} .. {ms[:, 1].max():.4f})")
        say(f"trace: {med[2]:.3f} ms ({ms[:, 2].min():.3f} .. {ms[:, 2].max():.3f}), {steps} RK4 steps, {steps * 4 / med[2] / 1e6:.2f} G field "
            f"evaluations/s")
        ref = info["psi"].tobytes()
        for wgs in (1, 7):
            lib.set_option("fmap_build_wgs", wgs, ctx)
            w = []
            for k in range(2 + a.repeats):
                psi = FB.solve(p, s, ctx=ctx)[0]
                if k >= 2:
                    w.append(FB.build_ms(ctx)[0])
            say(f"solve at fmap_build_wgs {wgs}: {float(np.median(w)):.3f} ms ({min(w):.3f} .. {max(w):.3f}), the same bytes: "
                f"{psi.tobytes() == ref}")
        lib.set_option("fmap_build_wgs", 0, ctx)
        t0 = time.perf_counter()
        tpsi = FB.solve_twin(p, s)
        t1 = time.perf_counter()
        twin = FB.trace_twin(p, tpsi)
        t2 = time.perf_counter()
        say(f"numpy twin on the host: direct solve {t1 - t0:.3f} s, field and paths {t2 - t1:.2f} s; max |kernels - twin|: "
            + ", ".join(f"{c} {np.abs(m[c] - twin[c]).max():.3e}" for c in ("E", "dx", "dy", "dz")))
        say(f"map: E / E0 {m['E'].min() / p['E0']:.6f} .. {m['E'].max() / p['E0']:.6f}, |dx| <= {np.abs(m['dx']).max():.4f} cm, |dy| <= "
            f"{np.abs(m['dy']).max():.4f} cm, dz {m['dz'].min():+.5f} .. {m['dz'].max():+.5f} cm, {int(info['flags'].sum())} flagged nodes")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        lib.destroy_context()
    if a.parent:
        bench_ab(os.path.abspath(a.parent), a.ab_out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
