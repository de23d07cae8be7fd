"""The fluctuation stage of the resident light response (ldsim_dev_light_response, light_response_ms()["fluctuations"]) with the
SiPM correlated noise off and on, on the 2x2 light leg: 2x2_no_modvar (384 rows x 16 000 ticks), one (event, TPC group) batch of
5000 segments, the synthetic LUT (14, 26, 8) x 48 channels per TPC, the shipped windows, keyed streams.

One mode per process: off (the plain keyed kernel), on (crosstalk 0.2, afterpulse 0.03, afterpulse_tau 0.1 us, no dark counts),
on_dark (the same with 1 dark count per us and row).  Prints the medians of the repeats after 3 warm-ups, the spread min .. max,
and the stage's share of the light response (scintillation + fluctuations + detector response), then one JSON line.
python tools/sipm_noise_timing.py [off|on|on_dark] [--segments N] [--repeats R]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

MODES = {"off": None, "on": dict(crosstalk=0.2, afterpulse=0.03, afterpulse_tau=0.1, dark_rate=0.0),
         "on_dark": dict(crosstalk=0.2, afterpulse=0.03, afterpulse_tau=0.1, dark_rate=1.0)}
WARMUP = 3


def main(mode, n_seg, reps, cfg="2x2_no_modvar"):
    import numpy as np
    import helpers as H
    from larndsim_amd import batching, consts, synth
    from larndsim_amd import rng as lrng
    from larndsim_amd.chain import ChargeChain
    med = lambda v: float(np.median(v))          # noqa: E731
    H.load_cfg(cfg)
    consts.sim.MAX_MC_TRUTH_IDS = 0
    light = consts.light
    seg = synth.make_segments(n_seg, seed=5, segs_per_event=n_seg, spill=cfg != "module0")
    batching.swap_coordinates(seg)
    seg = seg[batching.select_active_volume(seg, consts.detector.TPC_BORDERS)]
    bid, order, table = batching.assign_batches(seg)
    seg, bid = np.ascontiguousarray(seg[order]), bid[order]
    nsim = int((bid >= 0).sum())
    edges = np.flatnonzero(np.r_[True, bid[1:nsim] != bid[:nsim - 1], True])
    ch = ChargeChain()
    ch.upload(seg, bid)
    ch.quench_drift(consts.physics.BIRKS)
    ch.light_incidence(synth.make_lut((14, 26, 8), 48, 100, 3))
    opc = light.TPC_TO_OP_CHANNEL[:].ravel().astype(np.int32)
    n_ticks, _ = ch.sum_light(int(edges[0]), int(edges[1]), opc)
    ch.seed_keyed(1)
    ch.set_rng_key(lrng.call_key(1, 0, 0, 0))
    if MODES[mode] is not None:
        ch.set_sipm_noise(**MODES[mode])
    ms = []
    for i in range(reps + WARMUP):
        ch.light_response(fluctuate=True)
        if i >= WARMUP:
            ms.append(ch.light_response_ms())
    scint, disc, _, _, _ = ch.download_light_response(stages=True)
    if MODES[mode] is not None:
        ch.set_sipm_noise(enable=False)
    stage = {k: med([m[k] for m in ms]) for k in ms[0]}
    fl = [m["fluctuations"] for m in ms]
    tick = light.LIGHT_TICK_SIZE
    res = dict(mode=mode, cfg=cfg, rows=int(opc.shape[0]), n_ticks=int(n_ticks), segments=int(edges[1] - edges[0]), repeats=reps,
               params=MODES[mode], stage_ms=stage, fluct_ms=med(fl), fluct_min=min(fl), fluct_max=max(fl),
               share=stage["fluctuations"] / sum(stage.values()), lit_fraction=float((scint > 0).mean()),
               mean_pe_per_lit_tick=float(scint[scint > 0].mean() * tick) if (scint > 0).any() else 0.0,
               brightest_pe_per_tick=float(scint.max() * tick), avalanches=float(disc.astype(np.float64).sum() * tick))
    print(f"{cfg} {mode}: {res['rows']} rows x {n_ticks} ticks, {res['segments']} segments, {100 * res['lit_fraction']:.1f} % of the "
          f"elements lit (mean {res['mean_pe_per_lit_tick']:.3g}, brightest {res['brightest_pe_per_tick']:.3g} PE per tick): "
          f"fluctuations {res['fluct_ms']:.4f} ms ({res['fluct_min']:.4f} .. {res['fluct_max']:.4f}) = {100 * res['share']:.1f} % of "
          + " + ".join(f"{k} {v:.3f}" for k, v in stage.items()) + " ms", flush=True)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = {"--segments": 5000, "--repeats": 20}
    for k in list(opt):
        if k in argv:
            i = argv.index(k)
            opt[k] = int(argv[i + 1])
            del argv[i:i + 2]
    if len(argv) > 1 or (argv and argv[0] not in MODES):
        raise SystemExit(__doc__)
    main(argv[0] if argv else "off", opt["--segments"], opt["--repeats"])
