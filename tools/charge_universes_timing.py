"""The charge universes pass (ldsim_chain_universes) behind the module0 chain step on 100 k segments with the survey response:
HIP-event times of charge_weights_kernel (ldsim_chain_universes_weights_ms) and of the weighted instance of
pixel_adc_universes_kernel (ldsim_chain_fee_universes_ms) for 1, 4 and 8 universes with distinct charge variations (lifetimes
spread over 0.1 .. 1 times the nominal one, nominal front end: one wave scans per group while three wait), for 8 universes in 2
charge groups (four thresholds each), and, for comparison, the unweighted instance with 8 FEE universes -- beside the same
launch's adc_ms (ldsim_chain_kernel_ms) and the launch's own time; medians of the repeats after 2 warm-ups, with the spread
min .. max.
python tools/charge_universes_timing.py [n_segments] [repeats]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main(n_seg, reps):
    import numpy as np
    import helpers as H
    from larndsim_amd import batching, synth
    from larndsim_amd import charge_universes as CU
    from larndsim_amd import fee_universes as FU
    from larndsim_amd.chain import ChargeChain
    H.load_cfg("module0")
    seg = synth.make_segments(n_seg, seed=synth.SEED_BASE + 2, segs_per_event=5000)
    batching.swap_coordinates(seg)
    bid, order, table = batching.assign_batches(seg)
    seg, bid = seg[order], bid[order]
    resp = H.response_for("survey")
    med = lambda v: float(np.median(v))          # noqa: E731
    res = dict(n_segments=n_seg, repeats=reps, rows=[])
    ch = ChargeChain(resp)
    ch.upload(seg, bid)
    ch.quench_drift()
    ch.run(0, len(seg), want_fractions=True)                    # (the first launch grows the buffers)
    st = ch.run(0, len(seg), want_fractions=True)
    k_ms = ch.kernel_ms()
    res.update(unique_pixels=int(st.n_unique), n_pairs=int(st.n_pairs), adc_ms=k_ms["adc_ms"], launch_total_ms=k_ms["total_ms"])
    print(f"launch: {st.n_pairs} pairs, {st.n_unique} unique pixels, adc_ms {k_ms['adc_ms']:.3f}, total_ms {k_ms['total_ms']:.3f}",
          flush=True)

    def measure(what, fee, charge):
        weights, scan, call = [], [], []
        for i in range(reps + 2):
            ch.synchronize()
            t0 = time.perf_counter()
            us = ch.universes(fee=fee, charge=charge)
            ch.synchronize()
            if i >= 2:
                call.append(1e3 * (time.perf_counter() - t0))
                scan.append(ch.fee_universes_ms())
                weights.append(ch.universes_weights_ms() if charge is not None else 0.0)
        row = dict(what=what, n=len(us), weights_ms=med(weights), weights_ms_all=[round(x, 4) for x in weights], scan_ms=med(scan),
                   scan_ms_all=[round(x, 3) for x in scan], call_ms=med(call), hits=[u["n_hits"] for u in us],
                   unweightable=[u.get("n_unweightable", 0) for u in us])
        res["rows"].append(row)
        print(f"{what}: n = {len(us)}  weights kernel {med(weights):.4f} ms ({min(weights):.4f} .. {max(weights):.4f}); scan kernel "
              f"{med(scan):.3f} ms ({min(scan):.3f} .. {max(scan):.3f}) = {med(scan) / k_ms['adc_ms']:.2f} x adc_ms; whole call "
              f"{med(call):.1f} ms", flush=True)

    nom_c, nom_f = CU.nominal(CU.BIRKS), FU.nominal()
    for n in (1, 4, 8):
        scale = [0.5] if n == 1 else list(np.geomspace(0.1, 1.0, n))
        measure("distinct charge variations", None, [CU.variation(nom_c, electron_lifetime=float(s) * nom_c["electron_lifetime"])
                                                     for s in scale])
    thr = [FU.variation(nom_f, discrimination_threshold=float(s) * nom_f["discrimination_threshold"]) for s in (0.5, 0.8, 1.25, 2.0)]
    two = [CU.variation(nom_c, electron_lifetime=0.5 * nom_c["electron_lifetime"]), CU.variation(nom_c, recomb_mode=CU.BOX)]
    measure("8 universes in 2 charge groups", thr + thr, [two[0]] * 4 + [two[1]] * 4)
    measure("8 FEE universes, no charge variation", thr + [FU.variation(v, adc_hold_delay=7) for v in thr], None)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(int(args[0]) if len(args) > 0 else 100000, int(args[1]) if len(args) > 1 else 5)
