"""The light universes pass (ldsim_dev_light_universes) behind the light response of one (event, TPC group) batch at the reference
driver's sizes: module0 (96 rows) and 2x2_no_modvar (384 rows x 16 000 ticks), 5000 segments, the shipped windows, keyed streams.

For K = 1, 2, 4 and 8 distinct tables at a stage -- K scintillation tables over the one photon sum (universes that differ in TAU_T),
K response tables over the one fluctuated array (universes that differ in LIGHT_GAIN_SCALE) -- the HIP-event time of that stage
(ldsim_light_universes_ms) with light_plain_kernel over 2, 3 and 4 tables at a time, against K launches of its single-table
instance in the same session (option light_universes_nu 1: what the launch itself runs, the yardstick).  Then a typical
9-universe file (nominal and +- one knob each: PHOTON_SCALE, TAU_T, SINGLET_FRACTION, LIGHT_GAIN_SCALE) against nine times the
launch's own light_response_ms.  Medians of the repeats after 2 warm-ups, with the spread min .. max.
python tools/light_universes_timing.py [cfg ...] [--segments N] [--repeats R]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main(cfgs, n_seg, reps):
    import numpy as np
    import helpers as H
    from larndsim_amd import batching, consts, lib, synth
    from larndsim_amd import light_universes as LU
    from larndsim_amd import rng as lrng
    from larndsim_amd.chain import ChargeChain
    med = lambda v: float(np.median(v))          # noqa: E731
    spread = lambda v: f"{med(v):.3f} ms ({min(v):.3f} .. {max(v):.3f})"          # noqa: E731
    out = []
    for cfg in cfgs:
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
        launch = []
        for i in range(reps + 2):
            ch.light_response(fluctuate=True)
            if i >= 2:
                launch.append(ch.light_response_ms())
        l_ms = {k: med([m[k] for m in launch]) for k in launch[0]}
        l_sum = sum(l_ms.values())
        res = dict(cfg=cfg, rows=int(opc.shape[0]), n_ticks=int(n_ticks), conv_ticks=LU.conv_ticks(), segments=int(edges[1] - edges[0]),
                   repeats=reps, launch_ms=l_ms, stages=[])
        print(f"{cfg}: {res['rows']} rows x {n_ticks} ticks, C = {res['conv_ticks']}, batch of {res['segments']} segments; launch: "
              + ", ".join(f"{k} {v:.3f}" for k, v in l_ms.items()) + f" ms (sum {l_sum:.3f})", flush=True)
        nominal = LU.nominal()

        def measure(vs, stage):
            ms = []
            for i in range(reps + 2):
                ch.light_universes(vs, fluctuate=True)
                if i >= 2:
                    ms.append(ch.light_universes_ms())
            return [m[stage] for m in ms] if stage else ms

        for stage, field, label in (("scintillation", "tau_t", "scintillation tables over one photon sum"),
                                    ("detector_response", "gain_scale", "response tables over one fluctuated array")):
            for K in (1, 2, 4, 8):
                vs = [dict(nominal, **{field: nominal[field] * (1.0 + 0.05 * k)}) for k in range(K)]
                row = dict(stage=stage, K=K, by_nu={})
                for nu in (1, 2, 3, 4):
                    if nu > 1 and K == 1:
                        continue
                    lib.set_option("light_universes_nu", nu)
                    t = measure(vs, stage)
                    row["by_nu"][nu] = dict(median=med(t), all=[round(x, 4) for x in t])
                lib.set_option("light_universes_nu", 4)
                res["stages"].append(row)
                base = row["by_nu"][1]["median"]
                print(f"  K = {K} {label}: K launches of one table {spread(row['by_nu'][1]['all'])}"
                      + "".join(f"; {nu} at a time {spread(row['by_nu'][nu]['all'])} = {row['by_nu'][nu]['median'] / base:.2f} x"
                                for nu in (2, 3, 4) if nu in row["by_nu"]), flush=True)
        nine = [nominal]
        for f, d in (("photon_scale", 0.1), ("tau_t", 0.1), ("singlet_fraction", 0.1), ("gain_scale", 0.05)):
            nine += [dict(nominal, **{f: nominal[f] * (1 - d)}), dict(nominal, **{f: nominal[f] * (1 + d)})]
        for nu in (1, 4):
            lib.set_option("light_universes_nu", nu)
            ms = measure(nine, None)
            tot = [sum(m.values()) for m in ms]
            res[f"nine_nu{nu}"] = dict(total=med(tot), all=[round(x, 3) for x in tot], stages={k: med([m[k] for m in ms]) for k in ms[0]})
            print(f"  9-universe file (nominal, +- PHOTON_SCALE, TAU_T, SINGLET_FRACTION, LIGHT_GAIN_SCALE), {nu} table(s) at a time: "
                  f"{spread(tot)} = {med(tot) / l_sum:.2f} x the launch's light response (9 runs: 9.00 x); stages "
                  + ", ".join(f"{k} {v:.3f}" for k, v in res[f'nine_nu{nu}']['stages'].items()), flush=True)
        lib.set_option("light_universes_nu", 4)
        out.append(res)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = {"--segments": 5000, "--repeats": 5}
    for k in list(opt):
        if k in argv:
            i = argv.index(k)
            opt[k] = int(argv[i + 1])
            del argv[i:i + 2]
    main(argv or ["module0", "2x2_no_modvar"], opt["--segments"], opt["--repeats"])
