"""GPU: FEE universes (ChargeChain.fee_universes, ldsim_chain_fee_universes, simulate_pixels.py --fee_universes).

The yardstick is the code the project already has: universe k must equal, bit for bit, a fresh launch of the same segments
under ``consts`` patched to variation k (refresh_constants(), the same seed, the same batch keys) -- adc_list, adc_ticks_list,
adc_digit, the hit counts and the compact hit rows.  No tolerance: S is the same sum and the scan is the same code.  One
noise-free varied universe is also held against the oracle under the bars test_fused_chain_vs_oracle_two_batches uses.

The case is the 300-segment module0 case of test_gpu_pixel_waveforms.py (seed 31, batches (0,90) (1,47) (-1,30) (2,133), the
survey response, its four synthetic segments); the few helper lines are copied from there.  The magnitudes of KNOBS were picked
on the CPU: under each of them the oracle's get_adc_values / digitize on the oracle's sums of this case differ from the
nominal ones in a hit count or an ADC code, all three batches taken together (the GPU tests assert the same of the device's
results)."""
import contextlib
import ctypes as C
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import helpers as H
from larndsim_amd import batching, consts, detsim, lib, synth
from larndsim_amd import fee_universes as FU
from larndsim_amd.chain import ChargeChain
from larndsim_amd.layout import segments_dtype
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
SEED = 31
ECHO_TICKS = (90, 400)
LONE_SHIFT, LONE_DE = (5.0, -20.0), 30.0
LATE_SHIFT, LATE_US = (10.0, -20.0), 100.0
SIZES = [(0, 90), (1, 47), (-1, 30), (2, 133)]          # (batch id, segments)
TABLE = [(0, 0, 0, 90), (0, 1, 0, 47), (1, 0, 0, 133)]   # their identities (event, TPC group, sub-batch, n) for the keyed streams
KEYED_SEED = 20260131
DENSE = ("adc_list", "adc_ticks_list", "adc_digit")


def _segments(cfg="module0", n=300, seed=SEED):
    H.load_cfg(cfg)
    spill = bool(consts.sim.IS_SPILL_SIM)
    seg = synth.make_segments(n, seed=seed, segs_per_event=n, spill=spill)
    if spill:                            # the driver removes the spill offset
        loc = seg["event_id"] % consts.sim.MAX_EVENTS_PER_FILE
        for f in ("t0", "t0_start", "t0_end"):
            seg[f] = seg[f] - loc * consts.sim.SPILL_PERIOD
    batching.swap_coordinates(seg)
    return seg


def _add_synthetic(seg):
    """test_gpu_pixel_waveforms.py's: segments 1 and 2 echoes of segment 0 along the drift axis, segment 3 a copy moved in the
    pixel plane with LONE_DE times the energy (the launch's largest signal), segment 4 a copy LATE_US later whose signal is cut
    off by the last tick"""
    det = consts.detector
    z = float(seg["z"][0])
    for k, ticks in enumerate(ECHO_TICKS, start=1):
        dz = ticks * det.TIME_SAMPLING * det.V_DRIFT
        inside = [b for b in np.sort(np.asarray(det.TPC_BORDERS, dtype=np.float64)[:, 2, :], axis=-1) if b[0] <= z <= b[1]]
        assert len(inside) == 1, "segment 0 lies in one TPC"
        lo, hi = inside[0]
        step = dz if z + dz + 1.0 < hi else -dz
        assert lo < z + step - 1.0 and z + step + 1.0 < hi, "the echo stays inside the TPC"
        sid = seg["segment_id"][k]
        seg[k] = seg[0]
        seg["segment_id"][k] = sid
        for f in ("z", "z_start", "z_end"):
            seg[f][k] += step
    tpc = [b for b in np.sort(np.asarray(det.TPC_BORDERS, dtype=np.float64), axis=-1) if b[2][0] <= z <= b[2][1]][0]
    for k, shift in ((3, LONE_SHIFT), (4, LATE_SHIFT)):
        sid = seg["segment_id"][k]
        seg[k] = seg[0]
        seg["segment_id"][k] = sid
        for a, d in zip("xy", shift):
            for f in (a, a + "_start", a + "_end"):
                seg[f][k] += d
            i = "xyz".index(a)
            assert tpc[i][0] + 1.0 < seg[a][k] < tpc[i][1] - 1.0, "the moved segment stays inside the TPC"
    seg["dE"][3] *= LONE_DE
    for f in ("t0", "t0_start", "t0_end"):
        seg[f][4] += LATE_US
    return seg


def _oracle_sums(seg, resp):
    """(unique pixels, S f64 [U][N_t]) of one batch: the oracle's sum_pixel_signals"""
    det = consts.detector
    ref = seg.copy()
    O.quench(ref, consts.physics.BIRKS)
    O.drift(ref)
    nmax = O.max_pixels(ref)
    r = int(np.ceil(ref["tran_diff"].max() * 5 / det.PIXEL_PITCH))
    P = (2 * r + 1) * nmax + (1 + 2 * r) * r * 2
    _, neigh, nrad, _ = O.get_pixels(ref, nmax, P, r)
    upix = O.unique_pixels(neigh)
    starts, T = O.time_intervals(ref)
    sig = O.tracks_current(ref, neigh, T, resp)
    pim = O.pixel_index_map(neigh, upix)
    tpm = O.track_pixel_map(upix, neigh, nrad, int(nrad.max()) + 1, consts.sim.MAX_TRACKS_PER_PIXEL)
    ps, _, _ = O.sum_pixel_signals(sig, starts, pim, tpm, len(upix), want_tracks=False)
    return dict(upix=upix, S=ps)


@functools.lru_cache(maxsize=None)
def _module0_case():
    """the segments, their batch ids and the response: made once, read only"""
    seg = _add_synthetic(_segments())
    bid = np.concatenate([np.full(n, b) for b, n in SIZES]).astype(np.int32)
    resp = synth.make_response("survey")
    for a in (seg, bid, resp):
        a.setflags(write=False)
    return seg, bid, resp


@functools.lru_cache(maxsize=None)
def _oracle_case(batches=(0, 1, 2)):
    """the oracle's sums of the batches asked for: made once, read only"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    refs = {b: _oracle_sums(seg[bid == b], resp) for b in batches}
    for r in refs.values():
        for a in r.values():
            a.setflags(write=False)
    return refs


@contextlib.contextmanager
def _patched(v):
    """``consts.detector`` with the twelve constants of variation ``v``"""
    det = consts.detector
    names = [f.upper() for f in FU.FIELDS if f not in FU.TABLE_DEFAULTS]
    was = {n: getattr(det, n) for n in names}
    try:
        for n in names:
            setattr(det, n, v[n.lower()])
        yield
    finally:
        for n, x in was.items():
            setattr(det, n, x)


def oracle_fee(v, batches=(0, 1, 2)):
    """(adc_list, adc_ticks_list, adc_digit) per batch of the oracle's get_adc_values and digitize under the noise-free variation
    ``v`` on the oracle's sums"""
    refs = _oracle_case(batches)
    det = consts.detector
    tt = np.linspace(0, det.TIME_INTERVAL[1], len(det.TIME_TICKS) + 1)
    out = {}
    with _patched(v):
        for b, r in refs.items():
            adc, ticks, _ = O.get_adc_values(r["S"], None, tt, np.full(len(r["upix"]), float(v["discrimination_threshold"])),
                                             want_fractions=False)
            out[b] = (adc, ticks, O.digitize(adc))
    return out


def knobs():
    """{name: variation}: each front-end knob alone, moved from module0's constants (noise off).  The last one, "cap", moves four:
    threshold 0 (the discriminator fires whenever the ADC is idle: every tick is walked, as with noise) and the shortest timing,
    with which pixels fill all MAX_ADC_VALUES slots -- on the oracle's sums no positive threshold does (2 e with no reset cycle
    gives 28 of 30)."""
    H.load_cfg("module0")
    n = FU.nominal()
    return {
        "thr_half": FU.variation(n, discrimination_threshold=0.5 * n["discrimination_threshold"]),
        "thr_double": FU.variation(n, discrimination_threshold=2 * n["discrimination_threshold"]),
        "gain": FU.variation(n, gain=1.1 * n["gain"]),
        "v_pedestal": FU.variation(n, v_pedestal=n["v_pedestal"] + 40.0),
        "v_ref": FU.variation(n, v_ref=n["v_ref"] + 200.0),
        "v_cm": FU.variation(n, v_cm=n["v_cm"] + 62.0),
        "risetime_double": FU.variation(n, buffer_risetime=2 * n["buffer_risetime"]),
        "risetime_zero": FU.variation(n, buffer_risetime=0.0),
        "hold": FU.variation(n, adc_hold_delay=7),
        "busy": FU.variation(n, adc_busy_delay=40),
        "reset": FU.variation(n, reset_cycles=6),
        "cap": FU.variation(n, discrimination_threshold=0.0, adc_hold_delay=0, adc_busy_delay=0, reset_cycles=1),
    }


def _upload(ch, seg, bid, keyed=False):
    ch.upload(seg.copy(), bid)
    if keyed:
        ch.set_batch_keys(TABLE, -1)
    ch.quench_drift()


def _hit_counts(cpt, U):
    """the launch's own hit counts [U] from its compact form"""
    n = np.zeros(U, dtype=np.int32)
    n[cpt["hit_pixels"][:, 0]] = cpt["hit_pixels"][:, 3]
    return n


def _launch_result(ch, b0=0, e0=None):
    """run() and what a universe is compared with: the dense arrays, the hit counts, the compact hit rows and charges"""
    st = ch.run(b0, ch.n if e0 is None else e0, want_fractions=False)
    out, cpt = ch.download(), ch.download_compact()
    r = {k: out[k] for k in DENSE + ("unique_pix", "batch")}
    r.update(hit_count=_hit_counts(cpt, int(st.n_unique)), hit_rows=cpt["hit_rows"], hit_charge=cpt["hit_charge"])
    return r


def _fresh(ch, v, b0=0, e0=None):
    """a fresh launch of the resident segments under ``consts`` patched to ``v``; the constants are put back afterwards (the launch
    that is left is the patched one's: run() again before a pass)"""
    try:
        with _patched(v):
            ch.refresh_constants()
            return _launch_result(ch, b0, e0)
    finally:
        ch.refresh_constants()


def _assert_same(u, ref, what):
    """bit for bit: dense arrays, hit counts, compact rows field by field, charges"""
    for k in DENSE:
        assert u[k].shape == ref[k].shape and u[k].tobytes() == ref[k].tobytes(), (what, k)
    assert np.array_equal(u["hit_count"], ref["hit_count"]), what
    assert u["n_hits"] == len(ref["hit_rows"]) == int(ref["hit_count"].sum()), what
    for f in u["hit_rows"].dtype.names:
        assert u["hit_rows"][f].tobytes() == ref["hit_rows"][f].tobytes(), (what, f)
    assert u["hit_charge"].tobytes() == ref["hit_charge"].tobytes(), what


def _differs(a, b):
    return (not np.array_equal(a["hit_count"], b["hit_count"])) or (not np.array_equal(a["adc_digit"], b["adc_digit"]))


def _table_mode(resp):
    ChargeChain(resp).seed_rng(1, n_states=64)                  # (the ctx is process-wide: back to table mode)


def test_identity_noise_off_and_keyed_noise():
    """1. [nominal()] is the launch's own download() and compact hit rows: noise off, and keyed noise at the shipped charges"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    own = _launch_result(ch)
    assert FU.nominal() == ch.fee_variation_nominal() and not FU.is_noisy(FU.nominal())
    u = ch.fee_universes([FU.nominal()], dense=True)
    assert len(u) == 1 and u[0]["n_hits"] > 100
    _assert_same(u[0], own, "noise off")
    assert ch.fee_universes_ms() > 0
    H.load_cfg("module0", noise_zero=False)
    try:
        noisy = ChargeChain(resp)
        noisy.seed_keyed(KEYED_SEED)
        _upload(noisy, seg, bid, keyed=True)
        own_noisy = _launch_result(noisy)
        v = FU.nominal()
        assert FU.is_noisy(v) and v == noisy.fee_variation_nominal()
        _assert_same(noisy.fee_universes([v], dense=True)[0], own_noisy, "keyed noise")
        assert _differs(own_noisy, own)
    finally:
        H.load_cfg("module0")
        _table_mode(resp)


def test_each_knob_alone_against_a_fresh_launch():
    """2. every knob of knobs() in one call, each universe against a fresh launch under the patched constants, and each asserted
    to differ from nominal in a hit count or an ADC code; "cap" fills all MAX_ADC_VALUES slots of some pixel (4.)"""
    seg, bid, resp = _module0_case()
    K = knobs()
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    refs = {name: _fresh(ch, v) for name, v in K.items()}
    own = _launch_result(ch)
    us = ch.fee_universes([FU.nominal()] + list(K.values()), dense=True)
    _assert_same(us[0], own, "nominal")
    for (name, v), u in zip(K.items(), us[1:]):
        print(f"{name}: {u['n_hits']} hits (nominal {us[0]['n_hits']})")
        _assert_same(u, refs[name], name)
        assert _differs(u, own), name
    A = consts.sim.MAX_ADC_VALUES
    assert (us[1 + list(K).index("cap")]["hit_count"] == A).any(), "a pixel reaches MAX_ADC_VALUES hits"


def test_noise_on_and_off_over_the_other_kind_of_launch():
    """2. keyed: a noisy universe over a noise-free nominal launch, and a noise-free universe over a noisy nominal launch, each
    against the fresh launch; two noisy universes of one call share their normals (same draws, other charges)"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0", noise_zero=False)
    noisy_v = FU.nominal()
    half_v = FU.variation(noisy_v, **{f: 0.5 * noisy_v[f] for f in FU.NOISE_FIELDS})
    H.load_cfg("module0")
    quiet_v = FU.nominal()
    try:
        ch = ChargeChain(resp)
        ch.seed_keyed(KEYED_SEED)
        _upload(ch, seg, bid, keyed=True)
        ref_noisy, ref_half = _fresh(ch, noisy_v), _fresh(ch, half_v)
        own = _launch_result(ch)                                # noise-free nominal
        us = ch.fee_universes([quiet_v, noisy_v, half_v], dense=True)
        _assert_same(us[0], own, "quiet over quiet")
        _assert_same(us[1], ref_noisy, "noisy over quiet")
        _assert_same(us[2], ref_half, "half the charges over quiet")
        assert _differs(us[1], own) and _differs(us[2], own) and _differs(us[1], us[2])
        # the other way round: the nominal launch has noise
        H.load_cfg("module0", noise_zero=False)
        ch.refresh_constants()
        own_noisy = _launch_result(ch)
        _assert_same(dict(own_noisy, n_hits=len(own_noisy["hit_rows"])), ref_noisy, "the noisy launch is the fresh noisy launch")
        us = ch.fee_universes([quiet_v, noisy_v], dense=True)
        _assert_same(us[0], own, "quiet over noisy")
        _assert_same(us[1], own_noisy, "noisy over noisy")
    finally:
        H.load_cfg("module0")
        _table_mode(resp)


def test_group_boundaries_and_positions():
    """3. n = 1, 3, 4, 5 and 9 universes in one call: universe k's result is the same bits at every n and at every position"""
    seg, bid, resp = _module0_case()
    K = knobs()
    pool = [FU.nominal()] + [K[k] for k in ("thr_half", "risetime_zero", "hold", "gain", "busy", "thr_double", "reset", "v_ref")]
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    _launch_result(ch)
    alone = [dict(ch.fee_universes([v], dense=True)[0]) for v in pool]          # n = 1, nine times
    for n in (3, 4, 5, 9):
        us = ch.fee_universes(pool[:n], dense=True)
        for k in range(n):
            _assert_same(us[k], alone[k], f"n = {n}, universe {k}")
    order = [8, 3, 5, 0, 7, 1, 6, 2, 4]
    us = ch.fee_universes([pool[i] for i in order], dense=True)
    for pos, i in enumerate(order):
        _assert_same(us[pos], alone[i], f"universe {i} at position {pos}")
    # the same variation twice in one call
    us = ch.fee_universes([pool[1], pool[1], pool[2], pool[1], pool[1]], dense=True)
    for pos in (0, 1, 3, 4):
        _assert_same(us[pos], alone[1], f"repeated universe at position {pos}")


def test_record_layouts_and_sub_range_launches():
    """4. the set-up record as two lists (default) and as headers [U] (fee_one_class); one launch per batch joined equals the whole;
    pixels whose slots write no tick hold no hit in any universe"""
    seg, bid, resp = _module0_case()
    K = knobs()
    vs = [FU.nominal(), K["thr_half"], K["risetime_double"], K["cap"], K["busy"]]
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    own = _launch_result(ch)
    base = ch.fee_universes(vs, dense=True)
    truth = ch.pixel_truth(dense=True)
    dark = truth["q_abs"] == 0
    print(f"{int(dark.sum())} of {len(dark)} pixels saw no current")
    assert dark.any(), "the case holds pixels whose slots write no tick"
    for v, u in zip(vs, base):
        if v["discrimination_threshold"] > 0:                    # (threshold 0 fires on no charge at all)
            assert (u["hit_count"][dark] == 0).all() and (u["adc_list"][dark] == 0).all()
    try:
        lib.set_option("fee_one_class", 1)
        one = _launch_result(ch)
        for k in DENSE:
            assert one[k].tobytes() == own[k].tobytes(), k
        for u, b in zip(ch.fee_universes(vs, dense=True), base):
            _assert_same(u, b, "headers [U]")
    finally:
        lib.set_option("fee_one_class", 0)
    edges = np.r_[0, np.cumsum([n for _, n in SIZES])]
    parts = []
    for (b, n), lo, hi in zip(SIZES, edges[:-1], edges[1:]):
        if b >= 0:
            _launch_result(ch, int(lo), int(hi))
            parts.append(ch.fee_universes(vs, dense=True))
    for k, b in enumerate(base):
        for f in DENSE + ("hit_count", "hit_charge"):
            assert np.concatenate([p[k][f] for p in parts]).tobytes() == b[f].tobytes(), (k, f)
        joined = np.concatenate([p[k]["hit_rows"] for p in parts])
        for f in joined.dtype.names:
            assert joined[f].tobytes() == b["hit_rows"][f].tobytes(), (k, f)


def _column_segments(n=10):
    """n short parallel segments over one pixel column of TPC 0 (test_gpu_pixel_waveforms.py's)"""
    det = consts.detector
    rng = np.random.default_rng(5)
    seg = np.zeros(n, dtype=segments_dtype)
    b = np.sort(det.TPC_BORDERS[0], axis=-1)
    xc = b[0][0] + (40 + 0.5) * det.PIXEL_PITCH
    y0 = b[1][0] + (100 + 0.2) * det.PIXEL_PITCH
    z0 = 0.5 * (b[2][0] + b[2][1])
    xs = xc + rng.uniform(-0.3, 0.3, n) * det.PIXEL_PITCH
    zs = z0 + rng.uniform(-1.0, 1.0, n)
    seg["x_start"], seg["x_end"] = xs, xs + 0.01
    seg["y_start"], seg["y_end"] = y0, y0 + 2.6 * det.PIXEL_PITCH
    seg["z_start"], seg["z_end"] = zs, zs + 0.05
    for a in "xyz":
        seg[a] = 0.5 * (seg[a + "_start"] + seg[a + "_end"])
    seg["dx"] = np.sqrt(sum((seg[a + "_end"] - seg[a + "_start"]) ** 2 for a in "xyz"))
    seg["dEdx"] = 2.1
    seg["dE"] = seg["dEdx"] * seg["dx"]
    seg["segment_id"] = np.arange(n); seg["event_id"] = 0; seg["pdg_id"] = 13
    return seg


def test_more_pairs_than_slots_on_a_pixel():
    """4. MAX_TRACKS_PER_PIXEL = 4 and ten parallel segments over one pixel column: the universes sum the slots only, as the launch"""
    H.load_cfg("module0")
    consts.sim.MAX_TRACKS_PER_PIXEL = 4
    try:
        seg = _column_segments(10)
        ch = ChargeChain(synth.make_response("survey"))
        ch.upload(seg.copy(), np.zeros(len(seg), dtype=np.int32))
        ch.quench_drift()
        n = FU.nominal()
        vs = [n, FU.variation(n, discrimination_threshold=0.25 * n["discrimination_threshold"]),
              FU.variation(n, buffer_risetime=0.0, adc_hold_delay=3)]
        refs = [_fresh(ch, v) for v in vs]
        st = ch.run(want_fractions=False)
        assert st.n_overflow > 0
        us = ch.fee_universes(vs, dense=True)
        for k, (u, r) in enumerate(zip(us, refs)):
            _assert_same(u, r, f"M = 4, universe {k}")
        assert us[0]["n_hits"] > 0 and _differs(us[1], us[0]) and _differs(us[2], us[0])
    finally:
        H.load_cfg("module0")


def test_pixel_tables_scaled_like_a_fresh_launch_with_transformed_tables():
    """5. per-pixel thresholds and gains: a universe with scale 1.2, offset 50 e and gain scale 0.9 equals a fresh launch with
    the tables transformed the same way on the host; the nominal universe equals the launch with the tables as set"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    det = consts.detector
    n_ids = int(det.N_PIXELS[0] * det.N_PIXELS[1] * det.TPC_BORDERS.shape[0])
    rng = np.random.default_rng(77)
    keys = rng.choice(n_ids, size=n_ids // 2, replace=False).astype(np.int32)
    gain0 = det.GAIN * consts.units.mV / consts.units.e
    thr_default, gain_default = 1.3 * det.DISCRIMINATION_THRESHOLD, 0.9 * gain0
    thr_vals = det.DISCRIMINATION_THRESHOLD * rng.uniform(0.4, 3.0, keys.size)
    gain_vals = gain0 * rng.uniform(0.5, 1.5, keys.size)
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    plain = _launch_result(ch)
    v = FU.variation(threshold_table_scale=1.2, threshold_table_offset=50.0, gain_table_scale=0.9,
                     discrimination_threshold=123.0, gain=0.5)          # (the last two are not read with tables)
    try:
        ch.set_pixel_thresholds(keys, thr_vals * 1.2 + 50.0, thr_default * 1.2 + 50.0)
        ch.set_pixel_gains(keys, gain_vals * 0.9, gain_default * 0.9)
        ref = _launch_result(ch)
        ch.set_pixel_thresholds(keys, thr_vals, thr_default)
        ch.set_pixel_gains(keys, gain_vals, gain_default)
        own = _launch_result(ch)
        us = ch.fee_universes([FU.nominal(), v], dense=True)
        _assert_same(us[0], own, "tables as set")
        _assert_same(us[1], ref, "tables scaled")
        assert _differs(own, plain) and _differs(us[1], own)
        # a threshold table alone: the gain is the universe's constant
        ch.clear_pixel_tables()
        ch.set_pixel_thresholds(keys, thr_vals, thr_default)
        g = FU.variation(threshold_table_scale=1.2, threshold_table_offset=50.0, gain=1.1 * det.GAIN)
        with _patched(g):
            ch.refresh_constants()
            ch.set_pixel_thresholds(keys, thr_vals * 1.2 + 50.0, thr_default * 1.2 + 50.0)
            ref = _launch_result(ch)
        ch.refresh_constants()
        ch.set_pixel_thresholds(keys, thr_vals, thr_default)
        _launch_result(ch)
        _assert_same(ch.fee_universes([g], dense=True)[0], ref, "threshold table, constant gain")
    finally:
        ch.refresh_constants()
        ch.clear_pixel_tables()


def test_a_varied_universe_against_the_oracle():
    """6. one noise-free varied universe (threshold halved, rise time doubled, hold delay 7) against the oracle's get_adc_values
    and digitize under the patched constants on the oracle's sums, under the bars of test_fused_chain_vs_oracle_two_batches.
    Batch 1 (47 segments, 105 pixels): the oracle's currents of all three batches take minutes on a few cores."""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    n = FU.nominal()
    v = FU.variation(n, discrimination_threshold=0.5 * n["discrimination_threshold"], buffer_risetime=2 * n["buffer_risetime"],
                     adc_hold_delay=7)
    want = oracle_fee(v, (1,))
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    own = _launch_result(ch)
    u = ch.fee_universes([v], dense=True)[0]
    assert _differs(u, own)
    for b, (adc, ticks, digit) in want.items():
        m = own["batch"] == b
        assert np.array_equal(own["unique_pix"][m], _oracle_case((1,))[b]["upix"]) and m.sum() > 50
        assert (adc != 0).any() and not np.array_equal(digit, oracle_fee(FU.nominal(), (1,))[b][2])
        assert np.array_equal(u["adc_list"][m] != 0, adc != 0)
        np.testing.assert_allclose(u["adc_list"][m], adc, rtol=1e-5)
        assert np.array_equal(u["adc_ticks_list"][m], ticks)
        assert np.array_equal(u["adc_digit"][m], digit)


def test_the_pass_changes_nothing_of_the_launch():
    """7. download(), download_compact(), pixel_truth(), pixel_waveforms(), the statistics and (table mode, a noisy launch) the RNG
    states before and after a 9-universe call: identical bytes"""
    seg, bid, resp = _module0_case()
    K = knobs()
    H.load_cfg("module0", noise_zero=False)
    try:
        ch = ChargeChain(resp)
        states = ch.seed_rng(11, n_states=4096)
        _upload(ch, seg, bid)
        st = ch.run(want_fractions=True)
        assert st.n_unique <= 4096

        def snapshot():
            s = dict(stats=bytes(ch.stats), rng=states.copy_to_host().tobytes())
            for name, d in (("download", ch.download()), ("compact", ch.download_compact()), ("truth", ch.pixel_truth()),
                            ("truth_dense", ch.pixel_truth(dense=True)), ("waves", ch.pixel_waveforms(0.0, 3))):
                for k, a in d.items():
                    s[f"{name}.{k}"] = a.tobytes() if isinstance(a, np.ndarray) else a
            return s

        before = snapshot()
        us = ch.fee_universes([K[k] for k in ("thr_half", "thr_double", "gain", "risetime_zero", "hold", "busy", "reset", "cap",
                                              "v_cm")])
        assert len(us) == 9 and all(u["n_hits"] > 0 for u in us)
        after = snapshot()
        assert before.keys() == after.keys()
        for k in before:
            assert before[k] == after[k], k
        # the three passes in another order, twice
        ch.pixel_waveforms(0.0, 3)
        again = ch.fee_universes([K["thr_half"]])
        ch.pixel_truth()
        assert again[0]["hit_rows"].tobytes() == us[0]["hit_rows"].tobytes()
        assert snapshot() == before
    finally:
        H.load_cfg("module0")
        _table_mode(resp)


def _c_variations(vs):
    return FU.pack(vs)


def test_state_rules_and_bad_arguments():
    """8. every LDSIM_EINVAL leaves the previous result downloadable; LDSIM_ESTATE after reset, upload, quench_drift and a
    host-array stage call (the message names the call), from the downloads before a pass, and for noise without keyed mode; a
    launch without unique pixels gives zeros"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    K = knobs()
    ch = ChargeChain(resp)
    _table_mode(resp)
    _upload(ch, seg, bid)
    st = ch.run(want_fractions=False)
    L, U, A = lib.load(), int(st.n_unique), consts.sim.MAX_ADC_VALUES
    nh = (C.c_int64 * 64)()
    # the downloads before a pass of this launch
    assert L.ldsim_chain_fee_universe_download(ch.ctx, C.c_int32(0), C.c_int64(U), None, None, None, None) == -4
    assert b"ldsim_chain_fee_universes has not run for the last chain launch" in L.ldsim_last_error()
    assert L.ldsim_chain_fee_universe_hits_download(ch.ctx, C.c_int32(0), None, None) == -4
    assert L.ldsim_chain_fee_universes_ms(ch.ctx, None) == -4
    vs = [FU.nominal(), K["thr_half"]]
    base = ch.fee_universes(vs, dense=True)

    def still_there(what):
        cnt = np.zeros(U, dtype=np.int32)
        adc = np.zeros((U, A))
        lib.check(L.ldsim_chain_fee_universe_download(ch.ctx, C.c_int32(1), C.c_int64(U), lib.ptr(adc), None, None, lib.ptr(cnt)))
        assert np.array_equal(cnt, base[1]["hit_count"]) and adc.tobytes() == base[1]["adc_list"].tobytes(), what

    # k outside [0, n); too few rows
    for k in (-1, 2, 64):
        assert L.ldsim_chain_fee_universe_download(ch.ctx, C.c_int32(k), C.c_int64(U), None, None, None, None) == -1, k
        assert L.ldsim_chain_fee_universe_hits_download(ch.ctx, C.c_int32(k), None, None) == -1, k
    assert L.ldsim_chain_fee_universe_download(ch.ctx, C.c_int32(0), C.c_int64(U - 1), None, None, None, None) == -3
    # bad arguments: LDSIM_EINVAL, nothing written
    n = FU.nominal()
    arr = _c_variations(vs)
    for bad_n in (0, -1, 65):
        assert L.ldsim_chain_fee_universes(ch.ctx, arr, C.c_int32(bad_n), nh) == -1, bad_n
        assert b"[1, 64]" in L.ldsim_last_error()
        still_there(f"n = {bad_n}")
    dt = consts.detector.TIME_SAMPLING
    bad = [(dict(**{f: x}), b"not finite") for f in FU.FLOAT_FIELDS for x in (float("nan"), float("inf"))]
    bad += [(dict(v_ref=n["v_cm"]), b"v_ref == v_cm")]
    bad += [(dict(**{f: -1}), b"negative") for f in FU.INT_FIELDS + FU.NOISE_FIELDS]
    bad += [(dict(buffer_risetime=6.21 * dt), b"62 taps"), (dict(pad=1), b"pad")]
    for changes, word in bad:
        a = _c_variations([n, n])
        for f, x in changes.items():
            setattr(a[1], f, x)
        assert L.ldsim_chain_fee_universes(ch.ctx, a, C.c_int32(2), nh) == -1, changes
        assert word in L.ldsim_last_error() and b"universe 1" in L.ldsim_last_error(), (changes, L.ldsim_last_error())
        still_there(str(changes))
        if "pad" not in changes:
            with pytest.raises(ValueError, match=word.decode().replace("[", r"\[")):
                FU.validate([n, dict(n, **changes)])
    lib.check(L.ldsim_chain_fee_universes(ch.ctx, _c_variations([FU.variation(n, buffer_risetime=6.0 * dt)]), C.c_int32(1), nh))
    assert L.ldsim_chain_fee_universes(ch.ctx, None, C.c_int32(1), nh) == -1
    # noise without keyed mode: LDSIM_ESTATE naming the two calls (table mode never draws)
    noisy = FU.variation(n, uncorrelated_noise_charge=500.0)
    with pytest.raises(lib.LdsimError, match=r"ldsim error -4: .*ldsim_rng_keyed_seed.*ldsim_chain_set_batch_keys"):
        ch.fee_universes([n, noisy])
    base = ch.fee_universes(vs, dense=True)

    def refused(word):
        with pytest.raises(lib.LdsimError, match=rf"ldsim error -4: .*ldsim_chain_fee_universes.*{word}"):
            ch.fee_universes(vs)

    def rerun():
        ch.run(want_fractions=False)
        for u, b in zip(ch.fee_universes(vs, dense=True), base):
            _assert_same(u, b, "after a fresh run")

    ch.reset()
    refused("ldsim_segments_reset")
    ch.quench_drift()
    refused("ldsim_dev_quench_drift")
    rerun()
    ch.upload(seg.copy(), bid)
    refused("ldsim_segments_upload")
    ch.quench_drift()
    rerun()
    few = seg[:4].copy()
    sig = np.zeros((4, 3, 64), dtype=np.float32)
    detsim.tracks_current[1, 1](sig, np.full((4, 3), -1, dtype=np.int32), few, resp)
    refused("stage call")
    ch.upload(seg.copy(), bid)
    ch.quench_drift()
    rerun()
    # a new launch: the last pass is no longer this launch's
    ch.run(want_fractions=False)
    assert L.ldsim_chain_fee_universe_hits_download(ch.ctx, C.c_int32(0), None, None) == -4
    # nothing to simulate: every batch id negative
    ch.upload(seg.copy(), np.full(len(seg), -1, dtype=np.int32))
    ch.quench_drift()
    assert ch.run().n_unique == 0
    empty = ch.fee_universes(vs, dense=True)
    assert [u["n_hits"] for u in empty] == [0, 0]
    assert all(len(u["hit_rows"]) == 0 and u["adc_list"].shape == (0, A) and len(u["hit_count"]) == 0 for u in empty)
    assert ch.fee_universes_ms() == 0.0


def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_fee_universes_gpu", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _assert_same_bytes(x, y, what):
    """byte for byte; field by field for records (the padding bytes of an aligned record are not data)"""
    assert x.shape == y.shape and x.dtype == y.dtype, what
    for f in (x.dtype.names or [None]):
        xa, ya = (x, y) if f is None else (x[f], y[f])
        assert np.ascontiguousarray(xa).tobytes() == np.ascontiguousarray(ya).tobytes(), (what, f)


def _hits_of_raw(f):
    """(event_id, pixel_id, slot, adc, tick, charge) of a --raw_arrays file's own hits, pixel after pixel, slot 0 up"""
    adc = f["raw__adc_list"]
    u, s = np.nonzero(adc != 0)
    return (f["raw__event_id"][u], f["raw__unique_pix"][u], s, f["raw__adc_digit"][u, s].astype(np.int32),
            f["raw__adc_ticks_list"][u, s], adc[u, s])


def test_driver_writes_the_universes(tmp_path, capsys):
    """9. a 2-event file with three universes: the fee_universe_hits rows of universe 0 (nominal) are the file's own hits from
    --raw_arrays, the other universes' rows those of a second driver run under those constants; without the flag every dataset
    has the bytes it had (.npz stream: the interpreter of the GPU tests has no h5py)"""
    cli = _cli()
    H.load_cfg("module0")
    seg = synth.make_segments(80, seed=21, segs_per_event=40)          # 2 events
    seg = seg[np.random.default_rng(2).permutation(len(seg))]
    np.save(tmp_path / "in.npy", seg)
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    det = consts.detector
    entries = [dict(name="nominal"),
               dict(name="low threshold", DISCRIMINATION_THRESHOLD=0.5 * det.DISCRIMINATION_THRESHOLD),
               dict(name="slow buffer", BUFFER_RISETIME=2 * det.BUFFER_RISETIME, ADC_HOLD_DELAY=7)]
    with open(tmp_path / "uni.json", "w") as f:
        json.dump(entries, f)
    common = dict(input_filename=str(tmp_path / "in.npy"), config="module0", rand_seed=7, rng="keyed", light_simulated=False,
                  response_file=str(tmp_path / "resp.npy"), chunk_segments=40)

    def run(name, **kw):
        cli.run_simulation(output_filename=str(tmp_path / name), **common, **kw)
        with np.load(tmp_path / name) as f:
            return {k: f[k] for k in f.files}, capsys.readouterr().out

    # (the shipped configuration has noise: the nominal universe is noisy and the run keyed)
    a, log_a = run("uni.npz", fee_universes=str(tmp_path / "uni.json"), raw_arrays=True)
    assert "FEE universes:" in log_a and "no packets per universe" in log_a
    plain, log = run("plain.npz", raw_arrays=True)
    assert "FEE universes" not in log
    assert set(a) == set(plain) | {"fee_universes", "fee_universe_hits"}
    for k in plain:
        _assert_same_bytes(a[k], plain[k], k)
    rows, hits = a["fee_universes"], a["fee_universe_hits"]
    assert rows.dtype == FU.FILE_UNIVERSE and hits.dtype == FU.FILE_HIT
    assert rows["index"].tolist() == [0, 1, 2] and [n.decode() for n in rows["name"]] == [e["name"] for e in entries]
    H.load_cfg("module0", noise_zero=False)
    names, vs = FU.load(str(tmp_path / "uni.json"))
    _assert_same_bytes(rows, FU.universe_rows(names, vs), "fee_universes")
    assert set(hits["universe"].tolist()) == {0, 1, 2}

    def same_hits(k, f, what):
        mine = hits[hits["universe"] == k]
        want = _hits_of_raw(f)
        assert len(mine) == len(want[0]) > 50, (what, len(mine), len(want[0]))
        for name, w in zip(("event_id", "pixel_id", "slot", "adc", "tick", "charge"), want):
            assert np.array_equal(mine[name], w.astype(mine[name].dtype)), (what, name)
            assert mine[name].tobytes() == np.ascontiguousarray(w.astype(mine[name].dtype)).tobytes(), (what, name)

    same_hits(0, a, "nominal")
    try:
        for k in (1, 2):
            # a second driver run under those constants: the detector properties the driver loads, patched the same way
            import unittest.mock as mock
            real = consts.load_snapshot

            def patched_snapshot(*args, _v=vs[k], **kw):
                r = real(*args, **kw)
                for name in FU.FIELDS:
                    if name not in FU.TABLE_DEFAULTS:
                        setattr(consts.detector, name.upper(), _v[name])
                return r
            with mock.patch.object(consts, "load_snapshot", patched_snapshot):
                other, _ = run(f"other{k}.npz", raw_arrays=True)
            same_hits(k, other, names[k])
    finally:
        H.load_cfg("module0")
        _table_mode(synth.make_response("survey"))
    assert len(hits[hits["universe"] == 1]) != len(hits[hits["universe"] == 0])
    # the argument rules of run_simulation
    with open(tmp_path / "noisy.json", "w") as f:
        json.dump([dict(name="noisy", RESET_NOISE_CHARGE=100.0)], f)
    with pytest.raises(ValueError, match="--rng keyed"):
        cli.run_simulation(output_filename=str(tmp_path / "x.npz"), **dict(common, rng="table"),
                           fee_universes=str(tmp_path / "noisy.json"))


def test_identity_on_a_radius_3_launch():
    """[nominal()] over a launch at neighbour radius 3 (module0, TRAN_DIFF x 16) is that launch bit for bit, as in test 1: the pass
    walks the launch's slot list, in which the pixels whose every pair carries ring code -1 have no slot."""
    H.load_module0_wide(H.RADIUS3_SCALE)
    try:
        seg, resp = H.radius3_segments(), synth.make_response("survey")
        assert H.oracle_radius(seg) == 3
        ch = ChargeChain(resp)
        _upload(ch, seg, np.zeros(len(seg), dtype=np.int32))
        own = _launch_result(ch)
        tpm = ch.download()["track_pixel_map"]
        assert FU.nominal() == ch.fee_variation_nominal() and not FU.is_noisy(FU.nominal())
        u = ch.fee_universes([FU.nominal()], dense=True)
    finally:
        H.load_cfg("module0")
    no_slot = (tpm >= 0).sum(axis=1) == 0
    assert no_slot.sum() >= 10 and len(u) == 1 and u[0]["n_hits"] >= 5
    _assert_same(u[0], own, "radius 3")
    assert not u[0]["adc_list"][no_slot].any() and not u[0]["hit_count"][no_slot].any()
