"""The FEE universes pass (ldsim_chain_fee_universes) behind the module0 chain step on 100 k segments with the survey response:
HIP-event time of pixel_adc_universes_kernel (ldsim_chain_fee_universes_ms) for n = 1, 4, 8 and 16 noise-free universes
(thresholds spread over 0.5 .. 2 times the nominal one) beside the same launch's adc_ms (ldsim_chain_kernel_ms: fee_setup_kernel +
the pixel_adc kernels), and the time of the whole call -- tap tables, the kernel, n scans, the size read-back, n compactions -- by
a host clock; medians of the repeats after 2 warm-ups, with the spread min .. max.  Last, in keyed mode, 4 universes with the
shipped noise charges halved, whole, doubled and off over the noisy launch: a universe with noise walks every tick.
python tools/fee_universes_timing.py [n_segments] [repeats]"""
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

    def measure(ch, what, vs):
        kernel, call = [], []
        for i in range(reps + 2):
            ch.synchronize()
            t0 = time.perf_counter()
            us = ch.fee_universes(vs)
            ch.synchronize()
            if i >= 2:
                call.append(1e3 * (time.perf_counter() - t0))
                kernel.append(ch.fee_universes_ms())
        adc_ms = ch.kernel_ms()["adc_ms"]
        row = dict(what=what, n=len(vs), adc_ms=adc_ms, fee_universes_ms=med(kernel), fee_universes_ms_all=[round(x, 3) for x in kernel],
                   call_ms=med(call), call_ms_all=[round(x, 3) for x in call], hits=[u["n_hits"] for u in us])
        res["rows"].append(row)
        print(f"{what}: n = {len(vs):2d}  kernel {med(kernel):.3f} ms ({min(kernel):.3f} .. {max(kernel):.3f}) = "
              f"{med(kernel) / adc_ms:.2f} x adc_ms {adc_ms:.3f}; whole call with downloads of the hit rows {med(call):.3f} ms "
              f"({min(call):.3f} .. {max(call):.3f})", flush=True)

    ch = ChargeChain(resp)
    ch.upload(seg, bid)
    ch.quench_drift()
    st = ch.run(0, len(seg), want_fractions=True)
    res.update(unique_pixels=int(st.n_unique), n_pairs=int(st.n_pairs))
    nom = FU.nominal()
    for n in (1, 4, 8, 16):
        scale = [1.0] if n == 1 else list(np.geomspace(0.5, 2.0, n))
        measure(ch, "noise off", [FU.variation(nom, discrimination_threshold=float(s) * nom["discrimination_threshold"]) for s in scale])
    # keyed noise: the launch and the universes walk every tick
    H.load_cfg("module0", noise_zero=False)
    try:
        noisy = ChargeChain(resp)
        noisy.seed_keyed(7)
        noisy.upload(seg, bid)
        noisy.set_batch_keys(table, -1)
        noisy.quench_drift()
        noisy.run(0, len(seg), want_fractions=True)
        nom = FU.nominal()
        vs = [FU.variation(nom, **{f: s * nom[f] for f in FU.NOISE_FIELDS}) for s in (0.5, 1.0, 2.0, 0.0)]
        measure(noisy, "keyed noise x0.5, x1, x2, off", vs)
    finally:
        H.load_cfg("module0")
        ChargeChain(resp).seed_rng(1, n_states=64)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(int(args[0]) if len(args) > 0 else 100000, int(args[1]) if len(args) > 1 else 5)
