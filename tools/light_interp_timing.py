"""What the trilinear LUT interpolation (context option light_lut_interp, simulate_pixels.py --light_lut_interpolation trilinear)
costs on the light incidence stage.  Workloads: module0 and 2x2 (384 channels), 100 k segments each, (14, 26, 8) x 48 LUT.  In
one process: the HIP-event time of the incidence launch (ldsim_light_kernel_ms) with the option at 0, at 1 and at 0 again
(median of the repeats after 2 warm-ups, with the spread min .. max), then the wall time of the whole light leg of one batch --
incidence of the resident segments, photon sum, scintillation + fluctuations + SiPM response of the first batch -- both ways.
The bytes the stage writes (n x n_out x 4, twice under the threshold trigger) give the effective write bandwidth.
python tools/light_interp_timing.py [n_segments] [repeats] [--nearest_only]
--nearest_only: the option is never named (the same loop runs on a library without the feature: the reference for "unchanged")"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main(n, reps, nearest_only):
    import numpy as np
    import helpers as H
    from larndsim_amd import batching, consts, lib, synth
    from larndsim_amd.chain import ChargeChain
    lut = synth.make_lut((14, 26, 8), 48, 100, 7)
    for cfg in ("module0", "2x2_no_modvar"):
        H.load_cfg(cfg)
        light = consts.light
        seg = synth.make_segments(n, seed=synth.SEED_BASE + 2, segs_per_event=5000, spill=bool(consts.sim.IS_SPILL_SIM))
        if consts.sim.IS_SPILL_SIM:                 # the driver removes the spill offset
            loc = seg["event_id"] % consts.sim.MAX_EVENTS_PER_FILE
            for f in ("t0", "t0_start", "t0_end"):
                seg[f] = seg[f] - loc * consts.sim.SPILL_PERIOD
        batching.swap_coordinates(seg)
        bid, order, table = batching.assign_batches(seg)
        seg, bid = np.ascontiguousarray(seg[order]), bid[order]
        ch = ChargeChain()
        ch.upload(seg, bid)
        ch.quench_drift()
        ch.seed_rng(1)
        n_out = int(light.N_OP_CHANNEL)
        opc = light.TPC_TO_OP_CHANNEL[:].ravel().astype(np.int32)
        nsim = int((bid >= 0).sum())
        edges = np.flatnonzero(np.r_[True, bid[1:nsim] != bid[:nsim - 1], True])
        b0, b1 = int(edges[0]), int(edges[1])

        def option(v):
            if not nearest_only:
                lib.set_option("light_lut_interp", v)

        def incidence_ms():
            got = []
            for i in range(reps + 2):
                ch.light_incidence(lut)
                if i >= 2:
                    got.append(ch.light_kernel_ms()["incidence_ms"])
            return got

        def leg_ms():
            got = []
            for i in range(reps + 2):
                ch.synchronize()
                t0 = time.perf_counter()
                ch.light_incidence(lut)
                n_ticks, _ = ch.sum_light(b0, b1, opc, segment_track_id=np.arange(b0, b1, dtype=np.int64))
                ch.extend_rng(len(opc) * n_ticks, 7)
                ch.light_response(fluctuate=True)
                ch.synchronize()
                if i >= 2:
                    got.append(1e3 * (time.perf_counter() - t0))
            return got

        rounds = [("nearest", 0)] if nearest_only else [("nearest", 0), ("trilinear", 1), ("nearest_again", 0)]
        res = dict(cfg=cfg, n_segments=len(seg), n_out=n_out, light_trig_mode=int(light.LIGHT_TRIG_MODE), repeats=reps,
                   first_batch_segments=b1 - b0, nearest_only=bool(nearest_only))
        written = len(seg) * n_out * 4 * (2 if light.LIGHT_TRIG_MODE == 0 else 1)
        try:
            for name, v in rounds:
                option(v)
                ms = incidence_ms()
                res[name] = dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms),
                                 write_TBps=written / (float(np.median(ms)) * 1e-3) / 1e12)
            for name, v in rounds[:2]:
                option(v)
                ms = leg_ms()
                res["leg_" + name] = dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms))
        finally:
            option(0)
        print(json.dumps(res), flush=True)
        line = f"{cfg}: {len(seg)} segments x {n_out} channels: incidence " + ", ".join(
            f"{name} {res[name]['median_ms']:.3f} ms ({res[name]['min_ms']:.3f} .. {res[name]['max_ms']:.3f}; "
            f"{res[name]['write_TBps']:.2f} TB/s written)" for name, _ in rounds)
        if not nearest_only:
            line += (f"; trilinear / nearest {res['trilinear']['median_ms'] / res['nearest']['median_ms']:.2f}; light leg of a "
                     f"{b1 - b0}-segment batch {res['leg_nearest']['median_ms']:.2f} -> {res['leg_trilinear']['median_ms']:.2f} ms")
        print(line, flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(int(args[0]) if len(args) > 0 else 100000, int(args[1]) if len(args) > 1 else 7, "--nearest_only" in sys.argv[1:])
