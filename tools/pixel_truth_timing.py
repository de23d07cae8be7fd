"""The module0 chain step on 100 k segments (noise off: the set-up record as two lists) with and without the pixel-truth pass
(ldsim_chain_pixel_truth at min_abs_charge 0) behind it: wall time of the pass, and of the chain launch in rounds that run the
pass after it and in rounds that do not, alternating in one process (median of the repeats after 2 warm-ups of each kind, with
the spread min .. max).  The pass reads the written window of every per-pair current row once from HBM (and once more from
cache for the pixel sums): those bytes are counted on the device (ldsim_chain_pixel_truth_row_samples) and reported with the
set-up record's bytes and the bytes of the dense arrays the pass clears and writes, next to the rows' bound n_pairs * T * 4.
python tools/pixel_truth_timing.py [n_segments] [repeats] [--launch_only]
--launch_only: no pass at all (the same loop runs on a library without the feature: the reference for "unchanged")"""
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

HBM_PEAK = 8.0e12          # bytes/s, MI355X data sheet


def main(n, reps, launch_only):
    import numpy as np
    import helpers as H
    from larndsim_amd import batching, lib, synth
    from larndsim_amd.chain import ChargeChain
    H.load_cfg("module0")
    seg = synth.make_segments(n, seed=synth.SEED_BASE + 2, segs_per_event=5000)
    batching.swap_coordinates(seg)
    bid, order, table = batching.assign_batches(seg)
    seg, bid = seg[order], bid[order]
    ch = ChargeChain(H.response_for("survey"))
    ch.upload(seg, bid)
    ch.quench_drift()
    L = lib.load()
    sizes = (C.c_int64 * 2)()
    launch = {False: [], True: []}          # wall time of the chain launch, by whether the round runs the pass behind it
    pass_ms = []
    st = None
    for i in range(2 * (reps + 2)):
        with_pass = bool(i & 1) and not launch_only
        ch.synchronize()
        t0 = time.perf_counter()
        st = ch.run(0, len(seg), want_fractions=True)
        ch.synchronize()
        t1 = time.perf_counter()
        if with_pass:
            lib.check(L.ldsim_chain_pixel_truth(ch.ctx, C.c_double(0.0), sizes))
            ch.synchronize()
        t2 = time.perf_counter()
        if i >= 4:
            launch[with_pass].append(1e3 * (t1 - t0))
            if with_pass:
                pass_ms.append(1e3 * (t2 - t1))
    med = lambda v: float(np.median(v)) if len(v) else None          # noqa: E731
    res = dict(n_segments=n, n_pairs=int(st.n_pairs), unique_pixels=int(st.n_unique), max_length=int(st.max_length),
               repeats=reps, launch_only=bool(launch_only),
               launch_ms=med(launch[False]), launch_ms_all=[round(v, 3) for v in launch[False]],
               launch_before_pass_ms=med(launch[True]), launch_before_pass_ms_all=[round(v, 3) for v in launch[True]])
    if pass_ms:
        from larndsim_amd import consts
        U, M = int(st.n_unique), consts.sim.MAX_TRACKS_PER_PIXEL
        rows_bytes = 4 * ch.pixel_truth_row_samples()                       # the windows pass A streams
        record_bytes = 64 * U + 16 * int(sizes[1])                          # a header per pixel, a slot row per filled slot
        dense_bytes = 2 * (U * (2 + M) * 8 + U * 4)                         # cleared, then written
        compact_bytes = 48 * int(sizes[0]) + 16 * int(sizes[1])
        moved = rows_bytes + record_bytes + dense_bytes + compact_bytes
        res.update(pass_ms=med(pass_ms), pass_ms_all=[round(v, 3) for v in pass_ms], kept_pixels=int(sizes[0]),
                   track_entries=int(sizes[1]), rows_bytes=rows_bytes, rows_bytes_bound=int(st.n_pairs) * int(st.max_length) * 4,
                   record_bytes=record_bytes, dense_bytes=dense_bytes, compact_bytes=compact_bytes,
                   bandwidth_TBps=moved / (med(pass_ms) * 1e-3) / 1e12, hbm_fraction=moved / (med(pass_ms) * 1e-3) / HBM_PEAK)
    print(json.dumps(res), flush=True)
    if pass_ms:
        a, b = launch[False], launch[True]
        print(f"pass {res['pass_ms']:.3f} ms ({min(pass_ms):.3f} .. {max(pass_ms):.3f}); chain launch alone {med(a):.3f} ms "
              f"({min(a):.3f} .. {max(a):.3f}), before a pass {med(b):.3f} ms ({min(b):.3f} .. {max(b):.3f}): difference "
              f"{med(b) - med(a):+.3f} ms; rows {rows_bytes / 2**20:.0f} MiB of {res['rows_bytes_bound'] / 2**20:.0f} MiB, record "
              f"{record_bytes / 2**20:.0f} MiB, dense arrays {dense_bytes / 2**20:.0f} MiB, compact form {compact_bytes / 2**20:.0f} MiB "
              f"-> {res['bandwidth_TBps']:.2f} TB/s over the whole pass = {100 * res['hbm_fraction']:.0f} % of the HBM peak")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(int(args[0]) if len(args) > 0 else 100000, int(args[1]) if len(args) > 1 else 5, "--launch_only" in sys.argv[1:])
