"""The pixel-waveform pass (ldsim_chain_pixel_waveforms) behind the module0 chain step on 100 k segments with the survey response
(noise off: the set-up record as two lists): HIP-event times of the count kernel and of the fill kernel
(ldsim_chain_pixel_waveforms_ms), and the time of the whole call -- count pass, two scans, the one size read-back, fill pass -- by
a host clock around the call and a stream synchronise; medians of the repeats after 2 warm-ups, with the spread min .. max.
Settings: threshold 0 and the 0.99 quantile of the non-zero |S| (estimated from the dense rows of 2000 pixels), pad 0 and 16.  The
pixel-truth pass is timed on the same launch in the same process as the yardstick: it reads the same rows once from HBM (and once
more from cache).  Bytes: each of count and fill reads the written windows of the rows once (pixel_truth_row_samples x 4) and the
set-up record; the fill pass writes 32 bytes per span and 4 per sample.
python tools/pixel_waveforms_timing.py [n_segments] [repeats]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

HBM_PEAK = 8.0e12          # bytes/s, MI355X data sheet


def main(n, reps):
    import numpy as np
    import helpers as H
    from larndsim_amd import batching, synth
    from larndsim_amd.chain import ChargeChain
    H.load_cfg("module0")
    seg = synth.make_segments(n, seed=synth.SEED_BASE + 2, segs_per_event=5000)
    batching.swap_coordinates(seg)
    bid, order, table = batching.assign_batches(seg)
    seg, bid = seg[order], bid[order]
    ch = ChargeChain(H.response_for("survey"))
    ch.upload(seg, bid)
    ch.quench_drift()
    st = ch.run(0, len(seg), want_fractions=True)
    U = int(st.n_unique)
    part = ch.pixel_waveforms(dense=True, rows=(0, min(U, 2000)))
    q99 = float(np.quantile(np.abs(part[part != 0]).astype(np.float64), 0.99))
    del part
    rows_bytes = 4 * ch.pixel_truth_row_samples()
    n_slots = int(ch.pixel_truth(0.0)["pixels"]["n_tracks"].sum())
    record_bytes = 64 * U + 16 * n_slots

    def timed(fn):
        v = []
        for i in range(reps + 2):
            ch.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ch.synchronize()
            if i >= 2:
                v.append(1e3 * (time.perf_counter() - t0))
        return out, v

    med = lambda v: float(np.median(v))          # noqa: E731
    import ctypes as C
    from larndsim_amd import lib
    L = lib.load()
    sizes2, sizes3 = (C.c_int64 * 2)(), (C.c_int64 * 3)()
    _, truth = timed(lambda: lib.check(L.ldsim_chain_pixel_truth(ch.ctx, C.c_double(0.0), sizes2)))
    res = dict(n_segments=n, n_pairs=int(st.n_pairs), unique_pixels=U, n_ticks=None, repeats=reps, rows_bytes=rows_bytes,
               record_bytes=record_bytes, pixel_truth_ms=med(truth), pixel_truth_ms_all=[round(x, 3) for x in truth], settings=[])
    print(f"pixel truth pass (yardstick) {med(truth):.3f} ms ({min(truth):.3f} .. {max(truth):.3f}); rows {rows_bytes / 2**20:.0f} MiB, "
          f"record {record_bytes / 2**20:.0f} MiB", flush=True)

    events = []                                   # (count kernel, fill kernel) ms of every call of wave()

    def wave(thr, pad):
        lib.check(L.ldsim_chain_pixel_waveforms(ch.ctx, C.c_double(thr), C.c_int32(pad), C.c_int32(0), sizes3))
        events.append(ch.pixel_waveforms_ms())
        return tuple(int(x) for x in sizes3)

    _, count = timed(lambda: wave(1e300, 0))
    res["count_only_ms"], res["count_only_ms_all"] = med(count), [round(x, 3) for x in count]
    print(f"whole call with no tick active (count pass, scans, read-back) {med(count):.3f} ms ({min(count):.3f} .. {max(count):.3f})",
          flush=True)
    for name, thr in (("0", 0.0), ("q99", q99)):
        for pad in (0, 16):
            del events[:]
            (n_spans, n_samples, nt), v = timed(lambda: wave(thr, pad))
            ck, fk = [e[0] for e in events[2:]], [e[1] for e in events[2:]]
            res["n_ticks"] = nt
            written = 32 * n_spans + 4 * n_samples
            moved = 2 * (rows_bytes + record_bytes) + written
            res["settings"].append(dict(threshold=thr, threshold_name=name, pad=pad, spans=n_spans, samples=n_samples, ms=med(v),
                                        ms_all=[round(x, 3) for x in v], count_kernel_ms=med(ck), fill_kernel_ms=med(fk),
                                        count_kernel_ms_all=[round(x, 3) for x in ck], fill_kernel_ms_all=[round(x, 3) for x in fk],
                                        written_bytes=written, moved_bytes=moved, bandwidth_TBps=moved / (med(v) * 1e-3) / 1e12))
            print(f"threshold {name} ({thr:.4g}) pad {pad}: call {med(v):.3f} ms ({min(v):.3f} .. {max(v):.3f}); count kernel "
                  f"{med(ck):.3f} ms ({min(ck):.3f} .. {max(ck):.3f}) = {(rows_bytes + record_bytes) / (med(ck) * 1e-3) / 1e12:.2f} TB/s "
                  f"read; fill kernel {med(fk):.3f} ms ({min(fk):.3f} .. {max(fk):.3f}) = "
                  f"{(rows_bytes + record_bytes + written) / (med(fk) * 1e-3) / 1e12:.2f} TB/s read and written if it read every row (it skips the pixels without a span); {n_spans} spans, {n_samples} samples ({written / 2**20:.0f} MiB written, dense form "
                  f"{U * nt * 8 / 2**30:.1f} GiB f64); rows read twice -> {moved / (med(v) * 1e-3) / 1e12:.2f} TB/s over the whole call = "
                  f"{100 * moved / (med(v) * 1e-3) / HBM_PEAK:.0f} % of the HBM peak", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(int(args[0]) if len(args) > 0 else 100000, int(args[1]) if len(args) > 1 else 7)
