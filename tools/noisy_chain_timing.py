"""The module0 chain step on 100 k segments with FEE noise at the reference defaults (RESET_NOISE_CHARGE 900 e,
UNCORRELATED_NOISE_CHARGE 500 e, DISCRIMINATOR_NOISE 650 e), table mode against keyed mode: wall time of a launch (median of
the repeats, after warm-up), the FEE stage's kernel time, and the device memory the process holds after the runs (the chain's
scratch: table mode adds the pre-drawn normals, U x draws-per-pixel floats).  Each mode runs in a fresh process.
python tools/noisy_chain_timing.py [n_segments] [repeats]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def _used_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def child(mode, n, reps):
    import numpy as np
    import helpers as H
    from larndsim_amd import batching, consts, lib, synth
    from larndsim_amd.chain import ChargeChain
    H.load_cfg("module0", noise_zero=False)
    assert consts.detector.RESET_NOISE_CHARGE == 900 and consts.detector.DISCRIMINATOR_NOISE == 650
    seg = synth.make_segments(n, seed=synth.SEED_BASE + 2, segs_per_event=5000)
    batching.swap_coordinates(seg)
    bid, order, table = batching.assign_batches(seg)
    seg, bid = seg[order], bid[order]
    ch = ChargeChain(H.response_for("survey"))
    ch.upload(seg, bid)
    ch.quench_drift()
    base = _used_bytes()
    if mode == "keyed":
        ch.seed_keyed(7)
        ch.set_batch_keys(table, 1)
    else:
        ch.seed_rng(7)
    wall, adc = [], []
    for i in range(reps + 2):
        ch.synchronize()
        t0 = time.perf_counter()
        ch.run(0, len(seg), want_fractions=True)
        ch.synchronize()
        if i >= 2:
            wall.append(1e3 * (time.perf_counter() - t0))
            adc.append(ch.kernel_ms()["adc_ms"])
    d = ch.download()
    print("RESULT " + json.dumps(dict(mode=mode, n_segments=n, unique_pixels=int(len(d["unique_pix"])),
                                      hits=int((d["adc_list"] != 0).sum()), wall_ms=float(np.median(wall)),
                                      adc_ms=float(np.median(adc)), scratch_bytes_over_upload=int(_used_bytes() - base),
                                      repeats=reps)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    res = {}
    for mode in ("table", "keyed"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, str(n), str(reps)], capture_output=True,
                           timeout=600)
        if r.returncode:
            sys.stderr.write(r.stderr.decode()[-3000:])
            sys.exit(r.returncode)
        res[mode] = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][0][7:])
        print(json.dumps(res[mode]), flush=True)
    print(f"keyed / table wall time: {res['keyed']['wall_ms'] / res['table']['wall_ms']:.3f}; FEE stage "
          f"{res['keyed']['adc_ms'] / res['table']['adc_ms']:.3f}; scratch {res['table']['scratch_bytes_over_upload'] / 2**20:.0f} "
          f"MiB -> {res['keyed']['scratch_bytes_over_upload'] / 2**20:.0f} MiB")
