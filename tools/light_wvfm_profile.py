"""Time of the device-resident light waveform chain per (event, TPC group) batch at the reference driver's sizes:
photon sum -> scintillation -> Poisson -> SiPM response -> triggers -> digitised waveforms (with a noise spectrum).
usage: python tools/light_wvfm_profile.py [cfg] [n_segments] [max_truth] [light_truth_lds]
light_truth_lds 0: the truth slots of the response stages on the rows in memory (light_truth_rows_kernel) instead of in LDS."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'larnd-sim_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'tests'))
import numpy as np  # noqa: E402
import helpers as H  # noqa: E402
from larndsim_amd import batching, consts, lib, light_sim, synth  # noqa: E402
from larndsim_amd.chain import ChargeChain  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "2x2_no_modvar"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
H.load_cfg(cfg)
if len(sys.argv) > 3:
    consts.sim.MAX_MC_TRUTH_IDS = int(sys.argv[3])
light, sim = consts.light, consts.sim
seg = synth.make_segments(n, seed=5, segs_per_event=n)
seg = seg[batching.select_active_volume(seg, consts.detector.TPC_BORDERS)]
bid, order, table = batching.assign_batches(seg)
seg, bid = np.ascontiguousarray(seg[order]), bid[order]
lut = synth.make_lut((14, 26, 8), 48, 100, 3)
ch = ChargeChain()
if len(sys.argv) > 4:
    lib.set_option("light_truth_lds", int(sys.argv[4]))
ch.upload(seg, bid)
ch.quench_drift(consts.physics.BIRKS)
ch.light_incidence(lut)
opc = light.TPC_TO_OP_CHANNEL[:].ravel().astype(np.int32)
nd = opc.shape[0]
ns = int(np.ceil((light.LIGHT_TRIG_WINDOW[1] + light.LIGHT_TRIG_WINDOW[0]) / light.LIGHT_DIGIT_SAMPLE_SPACING))
noise = np.abs(np.random.default_rng(3).normal(0, 300.0, (light.N_OP_CHANNEL, 129)))
thr = np.repeat(np.array(light.LIGHT_TRIG_THRESHOLD)[..., None], light.OP_CHANNEL_PER_TRIG, axis=-1).ravel()[opc]
thr = thr.reshape(-1, light.OP_CHANNEL_PER_TRIG)[..., 0].copy()
nsim = int((bid >= 0).sum())
edges = np.flatnonzero(np.r_[True, bid[1:nsim] != bid[:nsim - 1], True])
print(f"{cfg}: {nsim} segments in {len(table)} batches, {nd} channels, truth slots {sim.MAX_MC_TRUTH_IDS}, {ns} samples per waveform")
ch.seed_rng(1)
for rep in range(2):
    for ib in range(min(len(table), 2)):
        b0, b1 = int(edges[ib]), int(edges[ib + 1])
        t = [time.perf_counter()]
        n_ticks, t_start = ch.sum_light(b0, b1, opc, segment_track_id=np.arange(b0, b1, dtype=np.int64)); t.append(time.perf_counter())
        ch.extend_rng(nd * n_ticks, 7); t.append(time.perf_counter())
        ch.light_response(fluctuate=True); t.append(time.perf_counter())
        trig, top, typ = light_sim.get_triggers(None, thr, opc, 0); t.append(time.perf_counter())
        wv, wt, wp = light_sim.sim_triggers(None, None, None, opc, None, None, trig, top, ns, noise); t.append(time.perf_counter())
        d = np.diff(t) * 1e3
        print(f"  rep {rep} batch {ib}: {b1 - b0} segments, {n_ticks} ticks, {len(trig)} triggers | sum {d[0]:.1f}  rng-table {d[1]:.1f}  "
              f"response {d[2]:.1f} {ch.light_response_ms()}  triggers {d[3]:.1f}  sim_triggers {d[4]:.1f} ms "
              f"| kernel ms: sum {ch.light_kernel_ms()}")
        print("     wvfm", wv.shape, "nonzero", float((wv != 0).mean()), "truth", int((wt >= 0).sum()))
