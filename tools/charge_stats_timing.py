"""The module0 quench_drift on 100 k segments with charge statistics on (quench_drift_stat_kernel: keyed binomial recombination
and attachment) against off (quench_drift_kernel): wall time of quench_drift alone (median of the repeats after 2 warm-ups),
both in keyed mode with batch keys set.  Each mode runs in a fresh process.
python tools/charge_stats_timing.py [n_segments] [repeats]"""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def child(mode, n, reps):
    import numpy as np
    import helpers as H
    from larndsim_amd import batching, synth
    from larndsim_amd.chain import ChargeChain
    H.load_cfg("module0")
    seg = synth.make_segments(n, seed=synth.SEED_BASE + 2, segs_per_event=5000)
    batching.swap_coordinates(seg)
    bid, order, table = batching.assign_batches(seg)
    seg, bid = seg[order], bid[order]
    ch = ChargeChain()
    ch.seed_keyed(7)
    ch.set_charge_statistics(mode == "on")
    ch.upload(seg, bid)
    ch.set_batch_keys(table, 1)
    qd = []
    for i in range(reps + 2):
        ch.reset()
        ch.synchronize()
        t0 = time.perf_counter()
        ch.quench_drift()
        ch.synchronize()
        t1 = time.perf_counter()
        if i >= 2:
            qd.append(1e3 * (t1 - t0))
    out = ch.download_segments(seg.copy())
    ch.set_charge_statistics(False)
    sim = bid >= 0
    print("RESULT " + json.dumps(dict(mode=mode, n_segments=n, n_simulated=int(sim.sum()), n_batches=len(table),
                                      electrons=float(out["n_electrons"][sim].astype(np.float64).sum()),
                                      quench_drift_ms=float(np.median(qd)), quench_drift_ms_all=[round(v, 4) for v in qd],
                                      repeats=reps)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    res = {}
    for mode in ("off", "on"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, str(n), str(reps)], capture_output=True,
                           timeout=600)
        if r.returncode:
            sys.stderr.write(r.stderr.decode()[-3000:])
            sys.exit(r.returncode)
        res[mode] = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][0][7:])
        print(json.dumps(res[mode]), flush=True)
    print(f"on - off: quench_drift {res['on']['quench_drift_ms'] - res['off']['quench_drift_ms']:+.3f} ms "
          f"({res['on']['quench_drift_ms'] / res['off']['quench_drift_ms']:.2f}x); electrons on / off "
          f"{res['on']['electrons'] / res['off']['electrons']:.6f}")
