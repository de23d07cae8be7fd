"""The module0 chain on 100 k segments with a drift-field map of 1 cm node pitch on every TPC (smooth E, dx, dy, dz) against the
same chain without a map: wall time of quench_drift alone and of quench_drift + one chain launch (median of the repeats after
2 warm-ups).  Each mode runs in a fresh process.
python tools/field_map_timing.py [n_segments] [repeats]"""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def _maps(consts, np):
    maps = {}
    for t, b in enumerate(np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)):
        lo, hi = b.min(axis=1) - 1, b.max(axis=1) + 1
        shape = tuple(int(v) for v in np.ceil(hi - lo) + 1)             # 1 cm pitch
        g = np.meshgrid(*[np.linspace(0, 1, s) for s in shape], indexing="ij")
        wave = np.sin(3 * g[0]) * np.cos(2 * g[1]) * np.sin(4 * g[2])
        maps[t] = dict(origin=lo, spacing=np.ones(3), E=consts.detector.E_FIELD * (1 + 0.1 * wave), dx=0.3 * wave,
                       dy=-0.2 * wave, dz=0.5 * wave)
    return maps


def child(mode, n, reps):
    import numpy as np
    import helpers as H
    from larndsim_amd import batching, consts, synth
    from larndsim_amd.chain import ChargeChain
    H.load_cfg("module0")
    seg = synth.make_segments(n, seed=synth.SEED_BASE + 2, segs_per_event=5000)
    batching.swap_coordinates(seg)
    bid, order, _ = batching.assign_batches(seg)
    seg, bid = seg[order], bid[order]
    ch = ChargeChain(H.response_for("survey"))
    nodes = 0
    if mode == "map":
        maps = _maps(consts, np)
        ch.set_field_map(maps)
        nodes = int(sum(m["E"].size for m in maps.values()))
    ch.upload(seg, bid)
    qd, launch = [], []
    for i in range(reps + 2):
        ch.reset()
        ch.synchronize()
        t0 = time.perf_counter()
        ch.quench_drift()
        ch.synchronize()
        t1 = time.perf_counter()
        ch.run(0, len(seg), want_fractions=True)
        ch.synchronize()
        t2 = time.perf_counter()
        if i >= 2:
            qd.append(1e3 * (t1 - t0))
            launch.append(1e3 * (t2 - t0))
    d = ch.download()
    print("RESULT " + json.dumps(dict(mode=mode, n_segments=n, map_nodes=nodes, map_mb=nodes * 32 / 1e6,
                                      unique_pixels=int(len(d["unique_pix"])), hits=int((d["adc_list"] != 0).sum()),
                                      quench_drift_ms=float(np.median(qd)), launch_ms=float(np.median(launch)),
                                      repeats=reps)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    res = {}
    for mode in ("none", "map"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, str(n), str(reps)], capture_output=True,
                           timeout=600)
        if r.returncode:
            sys.stderr.write(r.stderr.decode()[-3000:])
            sys.exit(r.returncode)
        res[mode] = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][0][7:])
        print(json.dumps(res[mode]), flush=True)
    print(f"map - none: quench_drift {res['map']['quench_drift_ms'] - res['none']['quench_drift_ms']:+.3f} ms, "
          f"quench_drift + launch {res['map']['launch_ms'] - res['none']['launch_ms']:+.3f} ms "
          f"({res['map']['launch_ms'] / res['none']['launch_ms']:.3f}x)")
