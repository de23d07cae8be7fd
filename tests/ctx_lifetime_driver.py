"""
Runs one case of tests/test_gpu_ctx_lifetime.py in a process of its own (so that the suite's process-wide context is left
alone) and writes what it counted to a JSON file; the assertions are the test's.

  python tests/ctx_lifetime_driver.py <case> <out.json>

Every count is ``ldsim_debug_live_objects``: [device buffers, streams, events] the library holds in this process.

Workload: module0, 1200 synthetic segments in two events (the chain splits a launch into two pair ranges from 8192
(segment, pixel) pairs on; 600 segments give 6639), 8 light detectors, 3000 light ticks, a 2x2x2 uniform field map on
TPC 0.  A pass runs every path of the library that makes a resident resource on first use.  It launches the charge chain
twice with an overlapped download after each: the first overlapped download switches the chain to two alternating sets of
output buffers, so both sets exist at the end of the first pass already.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "larnd-sim_amd"), HERE]

import helpers as H                                              # noqa: E402
from larndsim_amd import batching, consts, detsim, fee, lib, light_sim, synth     # noqa: E402
from larndsim_amd.chain import ChargeChain                       # noqa: E402

N_DET, MAX_TICKS, MAX_TRUTH = 8, 3000, 2


def counts():
    c = (C.c_int64 * 3)()
    lib.check(lib.load().ldsim_debug_live_objects(c))
    return [int(v) for v in c]


def configure():
    H.load_cfg("module0")
    consts.light.LIGHT_WINDOW = (0.5, 2.7)           # more than MAX_TICKS ticks per photon sum, 2200-tick convolutions
    seg = synth.make_segments(1200, seed=21, segs_per_event=600)
    batching.swap_coordinates(seg)
    bid, order, table = batching.assign_batches(seg)
    assert len(table) >= 2
    return np.ascontiguousarray(seg[order]), bid[order].astype(np.int32)


def new_chain(response):
    """a ChargeChain on a context of its own: ``lib`` keeps one context per process, detached here (the caller destroys it
    with ``ldsim_ctx_destroy``) together with what ``lib`` remembers about the tables it last sent"""
    lib._ctx = None
    lib._resp_token = lib._lut_token = None
    return ChargeChain(response)


def destroy(ch):
    lib.check(lib.load().ldsim_ctx_destroy(ch.ctx))
    if lib._ctx is ch.ctx:
        lib._ctx = None


def map_tpc0():
    b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[0]
    lo, hi = b.min(axis=1), b.max(axis=1)
    shape = (2, 2, 2)
    return {0: {"origin": lo - 1, "spacing": hi - lo + 2, "E": np.full(shape, float(consts.detector.E_FIELD)),
                "dx": np.zeros(shape), "dy": np.zeros(shape), "dz": np.zeros(shape)}}


def full_pass(ch, seg, bid, lut):
    """every path that makes a resident resource; returns the adc_list of the second chain launch"""
    n = len(seg)
    opc = np.ascontiguousarray(consts.light.TPC_TO_OP_CHANNEL[:].ravel()[:N_DET], dtype=np.int32)
    ch.seed_rng(77, N_DET * MAX_TICKS)                                   # ldsim_rng_seed
    ch.set_field_map(map_tpc0())
    ch.upload(seg, bid)
    ch.quench_drift()
    ch.light_incidence(lut)
    ch.sum_light(0, n, opc, max_truth=0, max_ticks=MAX_TICKS)            # the tile lists (light_act)
    lib.set_option("light_sum_async", 1, ch.ctx)
    ch.sum_light(0, n, opc, max_truth=0, max_ticks=MAX_TICKS)            # the same on the light stream
    lib.set_option("light_sum_async", 0, ch.ctx)
    n_ticks, _ = ch.sum_light(0, n, opc, np.arange(n, dtype="i8"), max_truth=MAX_TRUTH, max_ticks=MAX_TICKS)
    assert n_ticks == MAX_TICKS
    ch.light_response(fluctuate=True)
    lib.set_option("gform_chunks", 2, ch.ctx)
    L = lib.load()
    lib.check(L.ldsim_compact_accumulate(ch.ctx, C.c_int32(1)))          # (reset: empties the stream of compact results)
    for k in range(2):
        st = ch.run(0, n, want_fractions=True)
        assert st.n_pairs >= 2 * 4096, int(st.n_pairs)                   # (two pair ranges: the tables' stream and events exist)
        out = ch.download_async()
        ch.build_compact()
        lib.check(L.ldsim_compact_accumulate(ch.ctx, C.c_int32(0)))
        lib.check(L.ldsim_hits_accumulate(ch.ctx, C.c_int32(int(k == 0))))
    ch.wait_download()
    return out["adc_list"].copy()


def case_cycle():
    """tests 1 and 2: two passes in one context, then destroy"""
    seg, bid = configure()
    lut = synth.make_lut((14, 26, 8), 48, 20, 3)
    res = {"start": counts()}
    ch = new_chain(synth.make_response("survey"))
    adc1 = full_pass(ch, seg, bid, lut)
    res["pass1"] = counts()
    adc2 = full_pass(ch, seg, bid, lut)
    res["pass2"] = counts()
    res["same_adc"] = bool(np.array_equal(adc1, adc2)) and bool((adc1 != 0).any())
    destroy(ch)
    res["destroyed"] = counts()
    return res


def case_stage_calls():
    """test 3: the host-buffer stage calls on 12 rows, in a context that has run a pass (so that the resident scratch buffers
    of the light response, which its stage call shares, exist); the scintillation call gets the pass's own photon sum"""
    seg, bid = configure()
    lut = synth.make_lut((14, 26, 8), 48, 20, 3)
    ch = new_chain(synth.make_response("survey"))
    full_pass(ch, seg, bid, lut)
    inc, tid, tph = ch.download_light()
    g = H.gold("chain_module0.npz")
    U, M, A, NT = 12, consts.sim.MAX_TRACKS_PER_PIXEL, consts.sim.MAX_ADC_VALUES, len(consts.detector.TIME_TICKS)
    upix = np.ascontiguousarray(g["unique_pix"][:U])
    neigh, nrad = np.ascontiguousarray(g["neigh"]), np.ascontiguousarray(g["nrad"])
    pim = np.where(g["pixel_index_map"] < U, g["pixel_index_map"], -1).astype(np.int64)
    tpm = np.full((U, M), -1, dtype=np.int64)
    ps, pts, ovf = np.zeros((U, NT)), np.zeros((U, NT, M)), np.zeros(U)
    adc, tk, fr = np.zeros((U, A)), np.zeros((U, A)), np.zeros((U, A, M))
    tt = np.linspace(0, consts.detector.TIME_INTERVAL[1], NT + 1)
    thr = np.full(U, float(g["threshold_low"]))
    scint, s_id, s_ph = np.zeros_like(inc), np.full_like(tid, -1), np.zeros_like(tph)
    grid = ((inc.shape[0] + 7) // 8, (inc.shape[1] + 63) // 64), (8, 64)
    calls = [
        ("ldsim_track_pixel_map", lambda: detsim.get_track_pixel_map2[1, 32](tpm, upix, neigh, nrad, int(nrad.max()) + 1)),
        ("ldsim_sum_pixel_signals", lambda: detsim.sum_pixel_signals[1, 1](ps, g["signals"], g["track_starts"], pim, tpm, pts, ovf)),
        ("ldsim_get_adc_values", lambda: fee.get_adc_values[1, 128](ps, pts, tt, adc, tk, 0, None, fr, thr)),
        ("ldsim_digitize", lambda: fee.digitize(adc)),
        ("ldsim_scintillation_effect", lambda: light_sim.calc_scintillation_effect[grid[0], grid[1]](inc, tid, tph, scint, s_id, s_ph)),
    ]
    res = {"rows": {"pixels": U, "detectors": int(inc.shape[0])}, "calls": []}
    for name, call in calls:
        before = counts()
        call()
        res["calls"].append({"name": name, "before": before, "after": counts()})
    res["did_work"] = bool((tpm >= 0).any() and ps.any() and (adc != 0).any() and scint.any())
    destroy(ch)
    res["destroyed"] = counts()
    return res


def case_tables():
    """test 4: replacing and clearing tables"""
    seg, bid = configure()
    L = lib.load()
    ch = new_chain(None)
    res = {}
    lib.set_response(synth.make_response("survey"), ch.ctx, force=True)
    res["response_1"] = counts()
    lib.set_response(synth.make_response("dense", shape=(45, 45, 1200)), ch.ctx, force=True)
    res["response_2"] = counts()
    ch.set_pixel_thresholds(np.arange(16), np.full(16, 3000.0), float(consts.detector.DISCRIMINATION_THRESHOLD))
    res["thresholds_set"] = counts()
    ch.clear_pixel_tables()
    res["tables_cleared"] = counts()
    ch.upload(seg, bid)                  # (the store and the scratch of quench_drift exist before the map is set)
    ch.quench_drift()
    res["before_map"] = counts()
    ch.set_field_map(map_tpc0())
    ch.reset()
    ch.quench_drift()                    # (with a map set: the anode view)
    res["map_set"] = counts()
    lib.check(L.ldsim_clear_field_maps(ch.ctx))
    res["maps_cleared"] = counts()
    destroy(ch)
    res["destroyed"] = counts()
    return res


def case_two_contexts():
    """test 5: a context outlives another one's destruction"""
    seg, bid = configure()
    resp = synth.make_response("survey")

    def run(ch):
        ch.upload(seg, bid)
        ch.quench_drift()
        ch.run(0, len(seg))
        return ch.download()["adc_list"]
    a = new_chain(resp)
    run(a)
    b = new_chain(resp)
    assert a.ctx.value != b.ctx.value
    adc0 = run(b)
    res = {"both": counts()}
    destroy(a)
    res["first_destroyed"] = counts()
    adc1 = run(b)
    res["same_adc"] = bool(np.array_equal(adc0, adc1)) and bool((adc0 != 0).any())
    destroy(b)
    res["destroyed"] = counts()
    return res


CASES = {"cycle": case_cycle, "stage_calls": case_stage_calls, "tables": case_tables, "two_contexts": case_two_contexts}

if __name__ == "__main__":
    result = CASES[sys.argv[1]]()
    with open(sys.argv[2], "w") as f:
        json.dump(result, f, indent=1)
    print("ctx_lifetime_driver ok:", sys.argv[1])
