"""GPU: charge universes (ChargeChain.universes, ldsim_chain_universes, simulate_pixels.py --charge_universes).

Universe k of a pass re-weights the launch's current rows by one number per segment, w_k = n_k / n_res, and digitises the sum
again.  What is exact is tested exactly: the nominal variation (weights 1.0, the launch's own result), charge=None (the FEE
universes), the weights (n_k against a fresh quench_drift under the patched constants), S_k against the numpy twin fed with the
rows of a stage-call tracks_current, a universe alone against the same universe among others.  Against a fresh launch under the
patched constants a universe is held under the bars of test_fused_chain_vs_oracle_two_batches (hit masks, adc_list at 1e-5,
ticks, ADC codes), on the pixels whose hit count and hit ticks agree; the pixels left out (a row is f32: the fresh launch rounds
q' * shape, the universe w * f32(q * shape), and a threshold crossing can move by a tick) may be at most 2 % of the pixels with
hits, the three batches together.

The case is the 300-segment module0 case of test_gpu_fee_universes.py (seed 31, batches (0,90) (1,47) (-1,30) (2,133), the survey
response, its synthetic segments); the few helper lines are copied from there."""
import contextlib
import ctypes as C
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import helpers as H
from larndsim_amd import batching, consts, detsim, lib, pixels_from_track, synth
from larndsim_amd import charge_universes as CU
from larndsim_amd import fee_universes as FU
from larndsim_amd.chain import ChargeChain
from larndsim_amd.layout import segments_dtype

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
MAX_LEFT_OUT = 0.02


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
    """test_gpu_fee_universes.py's: segments 1 and 2 echoes of segment 0 along the drift axis, segment 3 a copy moved in the
    pixel plane with LONE_DE times the energy, segment 4 a copy LATE_US later whose signal is cut off by the last tick"""
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


@functools.lru_cache(maxsize=None)
def _module0_case():
    """the segments, their batch ids and the response: made once, read only"""
    seg = _add_synthetic(_segments())
    bid = np.concatenate([np.full(n, b) for b, n in SIZES]).astype(np.int32)
    resp = synth.make_response("survey")
    for a in (seg, bid, resp):
        a.setflags(write=False)
    return seg, bid, resp


_CONSTS = {"electron_lifetime": ("detector", "ELECTRON_LIFETIME"), "w_ion": ("physics", "W_ION"),
           "box_alpha": ("physics", "BOX_ALPHA"), "box_beta": ("physics", "BOX_BETA"), "birks_ab": ("physics", "BIRKS_Ab"),
           "birks_kb": ("physics", "BIRKS_kb")}


@contextlib.contextmanager
def _patched(charge=None, fee=None):
    """``consts`` with the six constants of the charge variation and the twelve of the FEE variation"""
    places = []
    if charge is not None:
        places += [(getattr(consts, ns), name, charge[f]) for f, (ns, name) in _CONSTS.items()]
    if fee is not None:
        places += [(consts.detector, f.upper(), fee[f]) for f in FU.FIELDS if f not in FU.TABLE_DEFAULTS]
    was = [(o, n, getattr(o, n)) for o, n, _ in places]
    try:
        for o, n, x in places:
            setattr(o, n, x)
        yield
    finally:
        for o, n, x in was:
            setattr(o, n, x)


def knobs():
    """{name: charge variation}: each knob of the issue alone, moved from module0's constants under Birks"""
    H.load_cfg("module0")
    n = CU.nominal(CU.BIRKS)
    return {
        "lifetime_half": CU.variation(n, electron_lifetime=0.5 * n["electron_lifetime"]),
        "lifetime_tenth": CU.variation(n, electron_lifetime=0.1 * n["electron_lifetime"]),
        "birks_ab": CU.variation(n, birks_ab=0.9 * n["birks_ab"]),
        "birks_kb": CU.variation(n, birks_kb=1.2 * n["birks_kb"]),
        "box": CU.variation(n, recomb_mode=CU.BOX),
        "box_alpha": CU.variation(n, recomb_mode=CU.BOX, box_alpha=0.9 * n["box_alpha"]),
        "w_ion_half": CU.variation(n, w_ion=0.5 * n["w_ion"]),
    }


def _upload(ch, seg, bid, keyed=False, mode=None):
    ch.upload(seg.copy(), bid)
    if keyed:
        ch.set_batch_keys(TABLE, -1)
    ch.quench_drift(mode)


def _hit_counts(cpt, U):
    n = np.zeros(U, dtype=np.int32)
    n[cpt["hit_pixels"][:, 0]] = cpt["hit_pixels"][:, 3]
    return n


def _launch_result(ch, b0=0, e0=None):
    """run() and what a universe is compared with: the dense arrays, the hit counts, the compact hit rows and charges"""
    st = ch.run(b0, ch.n if e0 is None else e0, want_fractions=False)
    out, cpt = ch.download(), ch.download_compact()
    r = {k: out[k] for k in DENSE + ("unique_pix", "batch", "track_pixel_map")}
    r.update(hit_count=_hit_counts(cpt, int(st.n_unique)), hit_rows=cpt["hit_rows"], hit_charge=cpt["hit_charge"])
    return r


def _fresh(ch, seg, bid, charge, fee=None, b0=0, e0=None):
    """a fresh upload, quench_drift and launch under ``consts`` patched to the variations: (the launch's result, the n_electrons
    column the quench_drift stored).  An upload, not reset(): download_segments writes the drifted fields into the staged
    records that reset() unpacks.  The constants are put back afterwards; the store and the launch that are left are the patched
    ones': ``_nominal_again`` before a pass."""
    try:
        with _patched(charge, fee):
            ch.refresh_constants()
            ch.upload(seg.copy(), bid)
            ch.quench_drift(charge["recomb_mode"])
            n_e = ch.download_segments(seg.copy())["n_electrons"].astype(np.float64)
            return _launch_result(ch, b0, e0), n_e
    finally:
        ch.refresh_constants()


def _nominal_again(ch, seg, bid, b0=0, e0=None):
    ch.upload(seg.copy(), bid)
    ch.quench_drift()
    return _launch_result(ch, b0, e0)


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


def _assert_close_to_fresh(u, ref, what, min_pixels=100):
    """the bars of test_fused_chain_vs_oracle_two_batches on the pixels whose hit count and hit ticks agree; the others at most
    MAX_LEFT_OUT of the pixels with hits"""
    assert u["adc_list"].shape == ref["adc_list"].shape, what
    has = (u["hit_count"] > 0) | (ref["hit_count"] > 0)
    same = (u["hit_count"] == ref["hit_count"]) & (u["adc_ticks_list"] == ref["adc_ticks_list"]).all(axis=1)
    left_out = int((has & ~same).sum())
    share = left_out / max(int(has.sum()), 1)
    print(f"{what}: {left_out} of {int(has.sum())} pixels with hits left out ({100 * share:.2f} %), {int(ref['hit_count'].sum())} hits")
    assert has.sum() > min_pixels and share <= MAX_LEFT_OUT, (what, left_out, int(has.sum()))
    a, b = u["adc_list"][same], ref["adc_list"][same]
    assert np.array_equal(a != 0, b != 0), what
    np.testing.assert_allclose(a, b, rtol=1e-5, err_msg=what)
    assert np.array_equal(u["adc_digit"][same], ref["adc_digit"][same]), what
    return share


def _table_mode(resp):
    ChargeChain(resp).seed_rng(1, n_states=64)                  # (the ctx is process-wide: back to table mode)


@functools.lru_cache(maxsize=None)
def _device_case():
    """Made once, read only: the fresh launch and n_electrons column of every knob, the nominal launch, the pass over
    [nominal] + knobs, the resident n_electrons, S_k of every universe"""
    seg, bid, resp = _module0_case()
    K = knobs()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    fresh = {name: _fresh(ch, seg, bid, v) for name, v in K.items()}
    own = _nominal_again(ch, seg, bid)
    n_res = ch.download_segments(seg.copy())["n_electrons"].astype(np.float64)
    nominal = CU.nominal(CU.BIRKS)
    assert nominal == ch.charge_variation_nominal()
    us = ch.universes(charge=[nominal] + list(K.values()), dense=True)
    weights_ms = ch.universes_weights_ms()
    S = [ch.universe_waveforms(k) for k in range(len(us))]
    return dict(K=K, fresh=fresh, own=own, n_res=n_res, us=us, S=S, weights_ms=weights_ms)


def test_nominal_is_the_launch_noise_off_and_keyed_noise():
    """1. universes(charge=[nominal]): every weight exactly 1.0, nothing unweightable, the result the launch's own download() and
    compact rows bit for bit -- noise off, and keyed noise at the shipped charges"""
    seg, bid, resp = _module0_case()
    D = _device_case()
    u = D["us"][0]
    assert (u["weights"] == 1.0).all() and len(u["weights"]) == len(seg) and u["n_unweightable"] == 0
    assert u["n_hits"] > 100 and D["weights_ms"] > 0
    _assert_same(u, D["own"], "noise off")
    H.load_cfg("module0", noise_zero=False)
    try:
        noisy = ChargeChain(resp)
        noisy.seed_keyed(KEYED_SEED)
        _upload(noisy, seg, bid, keyed=True)
        own_noisy = _launch_result(noisy)
        v = FU.nominal()
        assert FU.is_noisy(v)
        for fee in (None, [v]):                                  # (fee = None is the context's nominal front end: noisy here)
            un = noisy.universes(fee=fee, charge=[CU.nominal(CU.BIRKS)], dense=True)[0]
            assert (un["weights"] == 1.0).all()
            _assert_same(un, own_noisy, "keyed noise")
        assert _differs(own_noisy, D["own"])
    finally:
        H.load_cfg("module0")
        _table_mode(resp)


def test_charge_none_is_the_fee_universes():
    """2. charge=None: bit for bit fee_universes for the same FEE list, through the Python call and through the C entry point"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    n = FU.nominal()
    vs = [n, FU.variation(n, discrimination_threshold=0.5 * n["discrimination_threshold"]),
          FU.variation(n, buffer_risetime=0.0, adc_hold_delay=7)]
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    _launch_result(ch)
    base = ch.fee_universes(vs, dense=True)
    for u, b in zip(ch.universes(fee=vs, dense=True), base):
        assert "weights" not in u
        _assert_same(u, b, "charge=None")
    L, nh = lib.load(), (C.c_int64 * 3)()
    lib.check(L.ldsim_chain_universes(ch.ctx, FU.pack(vs), None, C.c_int32(3), nh))
    assert list(nh) == [b["n_hits"] for b in base]
    for u, b in zip(ch._universe_results(3, nh, True), base):
        _assert_same(u, b, "ldsim_chain_universes(fee, NULL)")
    # no weights after such a pass; S is the plain sum
    assert L.ldsim_chain_universe_weights_download(ch.ctx, C.c_int32(0), None, C.c_int64(len(seg)), None) == -4
    assert b"no charge variations" in L.ldsim_last_error()
    assert L.ldsim_chain_universes(ch.ctx, None, None, C.c_int32(3), nh) == -1
    # nominal charge under a varied front end is that FEE universe
    for u, b in zip(ch.universes(fee=vs, charge=[CU.nominal(CU.BIRKS)] * 3, dense=True), base):
        _assert_same(u, b, "nominal charge, varied FEE")


def _check_weights(ch, seg, bid, K, what):
    """every knob alone: n_k = weights * n_res, rounded to the column's type, against the n_electrons of a fresh quench_drift
    under the patched constants -- exact where n_res > 0"""
    fresh = {}
    for name, v in K.items():
        try:
            with _patched(v):
                ch.refresh_constants()
                ch.upload(seg.copy(), bid)
                ch.quench_drift(v["recomb_mode"])
                fresh[name] = ch.download_segments(seg.copy())["n_electrons"].astype(np.float64)
        finally:
            ch.refresh_constants()
    _nominal_again(ch, seg, bid)
    n_res = ch.download_segments(seg.copy())["n_electrons"].astype(np.float64)
    live = (n_res > 0) & (np.asarray(bid) >= 0)
    assert live.sum() > 200
    kind = seg.dtype["n_electrons"].kind
    for name, v in K.items():
        u = ch.universes(charge=[v])[0]                         # alone
        n_k = u["weights"] * n_res
        n_k = np.rint(n_k) if kind in "iu" else n_k.astype(seg.dtype["n_electrons"]).astype(np.float64)
        assert np.array_equal(n_k[live], fresh[name][live]), (what, name)
        assert not np.array_equal(fresh[name][live], n_res[live]), (what, name)
        w = u["weights"][live]
        print(f"{what} {name}: weights {w.min():.6f} ... {w.max():.6f}, unweightable {u['n_unweightable']}")
        assert (u["weights"][np.asarray(bid) < 0] == 1.0).all()


def test_weights_replay_a_fresh_quench_drift():
    """3. without a field map"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    _check_weights(ch, seg, bid, knobs(), "uniform field")
    D = _device_case()
    for (name, _), u in zip(D["K"].items(), D["us"][1:]):      # the same from the eight-universe call
        live = (D["n_res"] > 0) & (np.asarray(bid) >= 0)
        assert np.array_equal(np.rint(u["weights"] * D["n_res"])[live], D["fresh"][name][1][live]), name


def test_weights_replay_a_fresh_quench_drift_with_a_field_map():
    """3. with a 2x2x2 map per TPC whose E varies (and a drift offset, so the drift coordinate is the anode view's)"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    rs = np.random.default_rng(9)
    maps = {}
    for t in range(len(consts.detector.TPC_BORDERS)):
        b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[t]
        lo, hi = b.min(axis=1), b.max(axis=1)
        maps[t] = {"origin": lo - 1, "spacing": hi - lo + 2, "E": consts.detector.E_FIELD * rs.uniform(0.7, 1.3, (2, 2, 2)),
                   "dz": rs.uniform(-0.5, 0.5, (2, 2, 2))}
    ch = ChargeChain(resp)
    try:
        ch.set_field_map(maps)
        _upload(ch, seg, bid)
        _check_weights(ch, seg, bid, knobs(), "field map")
        # against the same segments without the map: the map changes the resident charge, so the replay read it
        mapped = ch.download_segments(seg.copy())["n_electrons"]
        ch.clear_field_map()
        _upload(ch, seg, bid)
        assert not np.array_equal(mapped, ch.download_segments(seg.copy())["n_electrons"])
    finally:
        ch.clear_field_map()


def _stage_rows(drifted, upix, tpm, resp):
    """per pixel of one batch its slots (segment in the batch, start tick, 0, T, row) from the stage calls on the drifted records:
    get_pixels, time_intervals, tracks_current (rows written in full: the window is the row)"""
    det = consts.detector
    r = np.ascontiguousarray(drifted)
    n = len(r)
    mp = np.array([0])
    pixels_from_track.max_pixels[1, 128](r, mp)
    rad = int(np.ceil(r["tran_diff"].max() * 5 / det.PIXEL_PITCH))
    P = (2 * rad + 1) * int(mp[0]) + (1 + 2 * rad) * rad * 2
    active = np.full((n, int(mp[0])), -1, dtype=np.int32)
    neigh = np.full((n, P), -1, dtype=np.int32)
    nrad = np.full((n, P), -1, dtype=np.int32)
    pixels_from_track.get_pixels[1, 128](r, active, neigh, nrad, np.zeros(n), rad)
    starts, tmax = np.empty(n), np.array([0])
    detsim.time_intervals[1, 128](starts, tmax, r)
    T = int(tmax[0])
    sig = np.zeros((n, P, T), dtype=np.float32)
    detsim.tracks_current[(1, 1, 1), (1, 1, 64)](sig, neigh, r, resp)
    pixels = []
    for u, pix in enumerate(upix):
        slots = []
        for j in tpm[u]:
            if j < 0:
                continue
            p = np.flatnonzero(neigh[j] == pix)
            assert len(p) == 1
            slots.append((int(j), int(np.rint(starts[j] / det.TIME_SAMPLING)), 0, T, sig[j, p[0]]))
        pixels.append(slots)
    return pixels


def test_weighted_sums_against_the_twin():
    """4. S_k of the dense download against charge_universes.weighted_sums fed with the per-slot rows of a stage-call
    tracks_current, the weights those of the pass: bit for bit, on pixels with one slot and on pixels with several"""
    seg, bid, resp = _module0_case()
    D = _device_case()
    H.load_cfg("module0")
    own = D["own"]
    NT = len(consts.detector.TIME_TICKS)
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    drifted = ch.download_segments(seg.copy())
    first = {b: int(np.flatnonzero(np.asarray(bid) == b)[0]) for b in (0, 1, 2)}
    n_one = n_many = 0
    for b in (1, 2):
        m = own["batch"] == b
        rows = np.flatnonzero(m)
        pixels = _stage_rows(drifted[np.asarray(bid) == b], own["unique_pix"][m], own["track_pixel_map"][m], resp)
        n_slots = np.array([len(s) for s in pixels])
        n_one += int((n_slots == 1).sum())
        n_many += int((n_slots > 1).sum())
        for k in (0, 2, 5, 7):                                  # nominal, lifetime / 10, box, W_ion / 2
            w = D["us"][k]["weights"][first[b]:first[b] + int((np.asarray(bid) == b).sum())]
            want = CU.weighted_sums(pixels, w, NT)
            got = D["S"][k][rows]
            assert np.abs(want).max() > 0
            assert got.tobytes() == want.tobytes(), (b, k, float(np.abs(got - want).max()))
    assert n_one > 20 and n_many > 20


def test_each_knob_against_a_fresh_launch():
    """5. every knob against a fresh launch under the patched constants: the bars and the 2 % cap; each knob changes a hit count
    or an ADC code"""
    D = _device_case()
    for (name, v), u in zip(D["K"].items(), D["us"][1:]):
        assert _differs(u, D["own"]), name
        _assert_close_to_fresh(u, D["fresh"][name][0], name)


def test_groups_and_positions():
    """6. n = 1, 3, 4, 5 and 9 universes; two charge variations, each repeated with different FEE variations and interleaved:
    every universe equals the same universe run alone, bit for bit"""
    seg, bid, resp = _module0_case()
    K = knobs()
    H.load_cfg("module0")
    n = FU.nominal()
    fees = [n, FU.variation(n, discrimination_threshold=0.5 * n["discrimination_threshold"]),
            FU.variation(n, buffer_risetime=0.0), FU.variation(n, adc_hold_delay=7), FU.variation(n, gain=1.1 * n["gain"])]
    a, b, c = K["lifetime_tenth"], K["box"], CU.nominal(CU.BIRKS)
    pool = [(a, fees[0]), (b, fees[1]), (a, fees[2]), (b, fees[0]), (c, fees[3]), (a, fees[4]), (b, fees[2]), (a, fees[1]),
            (K["w_ion_half"], fees[0])]
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    _launch_result(ch)
    alone = [dict(ch.universes(fee=[f], charge=[q], dense=True)[0]) for q, f in pool]
    for cnt in (3, 4, 5, 9):
        us = ch.universes(fee=[f for _, f in pool[:cnt]], charge=[q for q, _ in pool[:cnt]], dense=True)
        for k in range(cnt):
            _assert_same(us[k], alone[k], f"n = {cnt}, universe {k}")
            assert us[k]["weights"].tobytes() == alone[k]["weights"].tobytes()
    order = [8, 3, 5, 0, 7, 1, 6, 2, 4]
    us = ch.universes(fee=[pool[i][1] for i in order], charge=[pool[i][0] for i in order], dense=True)
    for pos, i in enumerate(order):
        _assert_same(us[pos], alone[i], f"universe {i} at position {pos}")
    # six universes of one charge variation: one group, more universes than waves
    six = ch.universes(fee=[fees[k % 5] for k in range(6)], charge=[a] * 6, dense=True)
    for k, i in {0: 0, 1: 7, 2: 2, 4: 5, 5: 0}.items():
        _assert_same(six[k], alone[i], f"one group, universe {k}")
    assert _differs(alone[0], alone[3]) and _differs(alone[0], alone[2])


def _column_segments(n=10):
    """n short parallel segments over one pixel column of TPC 0 (test_gpu_fee_universes.py's)"""
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


def test_more_pairs_than_slots_and_a_segment_without_charge():
    """7. MAX_TRACKS_PER_PIXEL = 4 and ten parallel segments over one pixel column (overflowing pixels): the universe sums the
    slots only, as the fresh launch; one segment's dE so small that the resident n_electrons is 0 while W_ion / 4 gives it
    electrons: weight 0, counted in n_unweightable"""
    H.load_cfg("module0")
    consts.sim.MAX_TRACKS_PER_PIXEL = 4
    try:
        seg = _column_segments(10)
        seg["dE"][6] = 0.9 * consts.physics.W_ION / 0.7        # recombination ~0.7: under one electron, more than two at W_ion / 4
        bid = np.zeros(len(seg), dtype=np.int32)
        ch = ChargeChain(synth.make_response("survey"))
        ch.upload(seg.copy(), bid)
        ch.quench_drift()
        nom = CU.nominal(CU.BIRKS)
        vs = [nom, CU.variation(nom, electron_lifetime=0.1 * nom["electron_lifetime"]), CU.variation(nom, w_ion=0.25 * nom["w_ion"])]
        refs = [_fresh(ch, seg, bid, v) for v in vs]
        _nominal_again(ch, seg, bid)
        assert ch.stats.n_overflow > 0
        n_res = ch.download_segments(seg.copy())["n_electrons"]
        assert n_res[6] == 0 and (np.delete(n_res, 6) > 0).all() and refs[2][1][6] > 0
        us = ch.universes(charge=vs, dense=True)
        assert [u["n_unweightable"] for u in us] == [0, 0, 1] and all(u["weights"][6] == 0 for u in us)
        _assert_same(us[0], refs[0][0], "M = 4, nominal")
        for k in (1, 2):
            live = n_res > 0
            assert np.array_equal(np.rint(us[k]["weights"] * n_res)[live], refs[k][1][live])
            _assert_close_to_fresh(us[k], refs[k][0], f"M = 4, universe {k}", min_pixels=5)
            assert _differs(us[k], us[0])
    finally:
        H.load_cfg("module0")


def test_record_layouts_and_sub_range_launches():
    """7. the set-up record as two lists (default) and as headers [U] (fee_one_class); one launch per batch joined equals the whole"""
    seg, bid, resp = _module0_case()
    K = knobs()
    H.load_cfg("module0")
    n = FU.nominal()
    charge = [CU.nominal(CU.BIRKS), K["lifetime_tenth"], K["box"], K["lifetime_tenth"], K["w_ion_half"]]
    fee = [n, n, FU.variation(n, buffer_risetime=0.0), FU.variation(n, adc_busy_delay=40), n]
    ch = ChargeChain(resp)
    _upload(ch, seg, bid)
    own = _launch_result(ch)
    base = ch.universes(fee=fee, charge=charge, dense=True)
    try:
        lib.set_option("fee_one_class", 1)
        one = _launch_result(ch)
        for k in DENSE:
            assert one[k].tobytes() == own[k].tobytes(), k
        for u, b in zip(ch.universes(fee=fee, charge=charge, dense=True), base):
            _assert_same(u, b, "headers [U]")
    finally:
        lib.set_option("fee_one_class", 0)
    edges = np.r_[0, np.cumsum([n for _, n in SIZES])]
    parts = []
    for (b, cnt), lo, hi in zip(SIZES, edges[:-1], edges[1:]):
        if b >= 0:
            _launch_result(ch, int(lo), int(hi))
            parts.append(ch.universes(fee=fee, charge=charge, dense=True))
            for k, u in enumerate(parts[-1]):
                assert u["weights"].tobytes() == base[k]["weights"][lo:hi].tobytes(), (b, k)
    for k, b in enumerate(base):
        for f in DENSE + ("hit_count", "hit_charge"):
            assert np.concatenate([p[k][f] for p in parts]).tobytes() == b[f].tobytes(), (k, f)
        joined = np.concatenate([p[k]["hit_rows"] for p in parts])
        for f in joined.dtype.names:
            assert joined[f].tobytes() == b["hit_rows"][f].tobytes(), (k, f)


def test_state_rules_and_bad_arguments():
    """8. no recorded mode (segments uploaded already quenched; after reset), charge statistics on: LDSIM_ESTATE with a message;
    every LDSIM_EINVAL names the universe and the field and leaves the earlier result downloadable"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    K = knobs()
    nom = CU.nominal(CU.BIRKS)
    ch = ChargeChain(resp)
    _table_mode(resp)
    _upload(ch, seg, bid)
    st = ch.run(want_fractions=False)
    L, U, A = lib.load(), int(st.n_unique), consts.sim.MAX_ADC_VALUES
    nh = (C.c_int64 * 64)()
    n_seg = C.c_int64(len(seg))
    assert L.ldsim_chain_universe_weights_download(ch.ctx, C.c_int32(0), None, n_seg, None) == -4
    assert L.ldsim_chain_universe_waveforms_dense(ch.ctx, C.c_int32(0), C.c_int64(0), C.c_int64(1), None) == -4
    vs = [nom, K["lifetime_tenth"]]
    base = ch.universes(charge=vs, dense=True)

    def still_there(what):
        cnt = np.zeros(U, dtype=np.int32)
        adc = np.zeros((U, A))
        lib.check(L.ldsim_chain_fee_universe_download(ch.ctx, C.c_int32(1), C.c_int64(U), lib.ptr(adc), None, None, lib.ptr(cnt)))
        assert np.array_equal(cnt, base[1]["hit_count"]) and adc.tobytes() == base[1]["adc_list"].tobytes(), what
        w, nu = ch.universe_weights(1)
        assert w.tobytes() == base[1]["weights"].tobytes() and nu == base[1]["n_unweightable"], what

    for bad_n in (0, -1, 65):
        assert L.ldsim_chain_universes(ch.ctx, None, CU.pack(vs), C.c_int32(bad_n), nh) == -1, bad_n
        assert b"[1, 64]" in L.ldsim_last_error()
        still_there(f"n = {bad_n}")
    bad = [(dict(**{f: x}), b"not finite") for f in CU.FLOAT_FIELDS for x in (float("nan"), float("inf"))]
    bad += [(dict(electron_lifetime=0.0), b"electron_lifetime"), (dict(electron_lifetime=-1.0), b"electron_lifetime"),
            (dict(w_ion=0.0), b"w_ion"), (dict(w_ion=-2.0), b"w_ion"), (dict(recomb_mode=0), b"recomb_mode"),
            (dict(recomb_mode=3), b"recomb_mode"), (dict(pad=1), b"pad")]
    for changes, word in bad:
        a = CU.pack([nom, nom])
        for f, x in changes.items():
            setattr(a[1], f, x)
        assert L.ldsim_chain_universes(ch.ctx, None, a, C.c_int32(2), nh) == -1, changes
        assert word in L.ldsim_last_error() and b"universe 1" in L.ldsim_last_error(), (changes, L.ldsim_last_error())
        for f in changes:
            if f != "pad":
                assert f.encode() in L.ldsim_last_error(), (changes, L.ldsim_last_error())
        still_there(str(changes))
        if "pad" not in changes:
            with pytest.raises(ValueError, match="universe 1"):
                CU.validate([nom, dict(nom, **changes)])
    # a bad FEE variation beside good charge variations
    f = FU.pack([FU.nominal(), FU.nominal()])
    f[1].v_ref = f[1].v_cm
    assert L.ldsim_chain_universes(ch.ctx, f, CU.pack(vs), C.c_int32(2), nh) == -1 and b"v_ref == v_cm" in L.ldsim_last_error()
    still_there("bad FEE variation")
    # the downloads' own arguments
    for k in (-1, 2):
        assert L.ldsim_chain_universe_weights_download(ch.ctx, C.c_int32(k), None, n_seg, None) == -1
        assert L.ldsim_chain_universe_waveforms_dense(ch.ctx, C.c_int32(k), C.c_int64(0), C.c_int64(1), None) == -1
    assert L.ldsim_chain_universe_weights_download(ch.ctx, C.c_int32(0), None, C.c_int64(len(seg) - 1), None) == -1
    for rows in ((-1, 1), (2, 1), (0, U + 1)):
        assert L.ldsim_chain_universe_waveforms_dense(ch.ctx, C.c_int32(0), C.c_int64(rows[0]), C.c_int64(rows[1]), None) == -1
    assert ch.universe_waveforms(1, (3, 3)).shape == (0, len(consts.detector.TIME_TICKS))
    with pytest.raises(ValueError, match="2 FEE variations for 1 charge"):
        ch.universes(fee=[FU.nominal()] * 2, charge=[nom])
    # noise without keyed mode
    with pytest.raises(lib.LdsimError, match=r"ldsim error -4: .*ldsim_rng_keyed_seed"):
        ch.universes(fee=[FU.variation(uncorrelated_noise_charge=500.0)], charge=[nom])
    base = ch.universes(charge=vs, dense=True)
    # the state rules of the FEE pass, the message naming this call
    ch.reset()
    with pytest.raises(lib.LdsimError, match=r"ldsim error -4: .*ldsim_chain_universes.*ldsim_segments_reset"):
        ch.universes(charge=vs)
    with pytest.raises(lib.LdsimError, match=r"ldsim error -4: .*no recorded recombination mode"):
        ch.charge_variation_nominal()
    # no recorded mode: the launch ran on segments uploaded already quenched and drifted
    ch.quench_drift()
    drifted = ch.download_segments(seg.copy())
    ch.upload(drifted, bid)
    ch.run(want_fractions=False)
    with pytest.raises(lib.LdsimError, match=r"ldsim error -4: ldsim_chain_universes: no recorded recombination mode"):
        ch.universes(charge=vs)
    assert len(ch.fee_universes([FU.nominal()])) == 1           # (the FEE pass does not need it)
    # the box model recorded: its nominal variation has weights 1
    _upload(ch, seg, bid, mode=CU.BOX)
    own_box = _launch_result(ch)
    assert ch.charge_variation_nominal() == CU.nominal(CU.BOX)
    ub = ch.universes(charge=[CU.nominal(CU.BOX), nom], dense=True)
    assert (ub[0]["weights"] == 1.0).all() and not (ub[1]["weights"] == 1.0).all()
    _assert_same(ub[0], own_box, "box launch, nominal")
    # charge statistics on
    try:
        ch.seed_keyed(KEYED_SEED)
        ch.set_charge_statistics(True)
        _upload(ch, seg, bid, keyed=True)
        ch.run(want_fractions=False)
        with pytest.raises(lib.LdsimError, match=r"ldsim error -4: ldsim_chain_universes: charge statistics are on"):
            ch.universes(charge=vs)
    finally:
        ch.set_charge_statistics(False)
        _table_mode(resp)
    # after all that a fresh upload and launch give the first result again
    _upload(ch, seg, bid)
    ch.run(want_fractions=False)
    for u, b in zip(ch.universes(charge=vs, dense=True), base):
        _assert_same(u, b, "after a fresh run")
    # nothing to simulate: every batch id negative
    ch.upload(seg.copy(), np.full(len(seg), -1, dtype=np.int32))
    ch.quench_drift()
    assert ch.run().n_unique == 0
    empty = ch.universes(charge=vs, dense=True)
    assert [u["n_hits"] for u in empty] == [0, 0] and all((u["weights"] == 1.0).all() for u in empty)


def test_the_pass_changes_nothing_of_the_launch():
    """8. download(), download_compact(), pixel_truth(), pixel_waveforms(), the statistics and (table mode, a noisy launch) the RNG
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
            s = dict(stats=bytes(ch.stats), rng=states.copy_to_host().tobytes(),
                     segments=ch.download_segments(seg.copy()).tobytes())
            for name, d in (("download", ch.download()), ("compact", ch.download_compact()), ("truth", ch.pixel_truth()),
                            ("truth_dense", ch.pixel_truth(dense=True)), ("waves", ch.pixel_waveforms(0.0, 3))):
                for k, a in d.items():
                    s[f"{name}.{k}"] = a.tobytes() if isinstance(a, np.ndarray) else a
            return s

        before = snapshot()
        H.load_cfg("module0")                                    # (noise-free universes over the noisy launch)
        quiet = FU.nominal()
        H.load_cfg("module0", noise_zero=False)
        charge = list(K.values()) + [CU.nominal(CU.BIRKS), K["box"]]
        us = ch.universes(fee=[quiet] * 9, charge=charge)
        assert len(us) == 9 and all(u["n_hits"] > 0 for u in us)
        ch.universe_waveforms(3, (0, 10))
        after = snapshot()
        assert before.keys() == after.keys()
        for k in before:
            assert before[k] == after[k], k
    finally:
        H.load_cfg("module0")
        _table_mode(resp)


def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_charge_universes_gpu", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _hits_of_raw(f):
    """per-pixel arrays of a --raw_arrays file keyed by (event, pixel)"""
    return {(int(e), int(p)): (f["raw__adc_list"][i], f["raw__adc_ticks_list"][i], f["raw__adc_digit"][i])
            for i, (e, p) in enumerate(zip(f["raw__event_id"], f["raw__unique_pix"]))}


def test_driver_writes_the_universes(tmp_path, capsys):
    """9. a 2-event file with three universes (one combined with a FEE key): charge_universes holds the values, the
    charge_universe_hits rows of universe 0 (nominal) are the file's own hits from --raw_arrays bit for bit, the other universes'
    rows those of second driver runs under the varied configuration within the bars of test 5; without the flag every dataset
    has the bytes it had"""
    cli = _cli()
    H.load_cfg("module0")
    seg = synth.make_segments(80, seed=21, segs_per_event=40)          # 2 events
    seg = seg[np.random.default_rng(2).permutation(len(seg))]
    np.save(tmp_path / "in.npy", seg)
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    life, w_ion, thr = (0.1 * consts.detector.ELECTRON_LIFETIME, 0.5 * consts.physics.W_ION,
                        0.5 * consts.detector.DISCRIMINATION_THRESHOLD)
    entries = [dict(name="nominal"), dict(name="short lifetime", ELECTRON_LIFETIME=life),
               dict(name="w_ion and threshold", W_ION=w_ion, DISCRIMINATION_THRESHOLD=thr)]
    with open(tmp_path / "uni.json", "w") as f:
        json.dump(entries, f)
    # noise off in every run (the second runs' noise would be drawn at other charges; keyed streams all the same)
    real = consts.load_snapshot

    nominal = CU.nominal(CU.BIRKS)

    def snapshot_with(charge=None, fee=None):
        def patched_snapshot(*args, **kw):
            r = real(*args, **kw)
            d = consts.detector
            d.RESET_NOISE_CHARGE = d.UNCORRELATED_NOISE_CHARGE = d.DISCRIMINATOR_NOISE = 0
            for fld, (ns, name) in _CONSTS.items():                 # (a snapshot does not reload consts.physics: always set)
                setattr(getattr(consts, ns), name, (charge or nominal)[fld])
            if fee is not None:
                d.DISCRIMINATION_THRESHOLD = fee["discrimination_threshold"]
            return r
        return patched_snapshot

    common = dict(input_filename=str(tmp_path / "in.npy"), config="module0", rand_seed=7, rng="keyed", light_simulated=False,
                  response_file=str(tmp_path / "resp.npy"), chunk_segments=40)
    import unittest.mock as mock

    def run(name, charge=None, fee=None, **kw):
        with mock.patch.object(consts, "load_snapshot", snapshot_with(charge, fee)):
            cli.run_simulation(output_filename=str(tmp_path / name), **common, **kw)
        with np.load(tmp_path / name) as f:
            return {k: f[k] for k in f.files}, capsys.readouterr().out

    try:
        a, log_a = run("uni.npz", charge_universes=str(tmp_path / "uni.json"), raw_arrays=True)
        assert "Charge universes:" in log_a
        plain, log = run("plain.npz", raw_arrays=True)
        assert "Charge universes" not in log
        assert set(a) == set(plain) | {"charge_universes", "charge_universe_hits"}
        for k in plain:
            x, y = a[k], plain[k]
            assert x.shape == y.shape and x.dtype == y.dtype, k
            for fld in (x.dtype.names or [None]):
                xa, ya = (x, y) if fld is None else (x[fld], y[fld])
                assert np.ascontiguousarray(xa).tobytes() == np.ascontiguousarray(ya).tobytes(), (k, fld)
        rows, hits = a["charge_universes"], a["charge_universe_hits"]
        assert rows.dtype == CU.FILE_UNIVERSE and hits.dtype == CU.FILE_HIT
        assert rows["index"].tolist() == [0, 1, 2] and [n.decode() for n in rows["name"]] == [e["name"] for e in entries]
        with mock.patch.object(consts, "load_snapshot", snapshot_with()):
            H.load_cfg("module0")
            names, cs, fs = CU.load(str(tmp_path / "uni.json"))
        assert rows["electron_lifetime"][1] == life and rows["w_ion"][2] == w_ion
        assert rows["discrimination_threshold"][2] == thr and (rows["recomb_mode"] == 2).all()
        expect = CU.universe_rows(names, cs, fs)
        for fld in rows.dtype.names:
            assert rows[fld].tobytes() == expect[fld].tobytes(), fld
        assert set(hits["universe"].tolist()) == {0, 1, 2}
        A = consts.sim.MAX_ADC_VALUES

        def per_pixel(k):
            """universe k's rows as per-pixel arrays keyed by (event, pixel)"""
            out = {}
            for r in hits[hits["universe"] == k]:
                adc, ticks, digit = out.setdefault((int(r["event_id"]), int(r["pixel_id"])), (np.zeros(A), np.zeros(A), np.zeros(A)))
                adc[r["slot"]], ticks[r["slot"]], digit[r["slot"]] = r["charge"], r["tick"], r["adc"]
            return out

        for k, (f, what) in enumerate(((a, "nominal"), (run("other1.npz", cs[1], fs[1], raw_arrays=True)[0], names[1]),
                                       (run("other2.npz", cs[2], fs[2], raw_arrays=True)[0], names[2]))):
            mine, want = per_pixel(k), {key: v for key, v in _hits_of_raw(f).items() if (v[0] != 0).any()}
            keys = sorted(set(mine) | set(want))
            zero = (np.zeros(A), np.zeros(A), np.zeros(A))
            same = [key for key in keys if np.array_equal(mine.get(key, zero)[1], want.get(key, zero)[1])
                    and np.array_equal(mine.get(key, zero)[0] != 0, want.get(key, zero)[0] != 0)]
            share = 1 - len(same) / len(keys)
            print(f"driver, {what}: {len(keys) - len(same)} of {len(keys)} pixels with hits left out ({100 * share:.2f} %)")
            assert len(keys) > 50 and share <= (0 if k == 0 else MAX_LEFT_OUT), what
            for key in same:
                hit = want[key][0] != 0                         # (a slot without hit holds the pedestal's code in the file's array)
                if k == 0:
                    assert all(x[hit].tobytes() == y[hit].tobytes() for x, y in zip(mine[key], want[key])), (what, key)
                else:
                    np.testing.assert_allclose(mine[key][0], want[key][0], rtol=1e-5)
                    assert np.array_equal(mine[key][2][hit], want[key][2][hit]), (what, key)
        assert len(hits[hits["universe"] == 1]) != len(hits[hits["universe"] == 0])
        # beside --fee_universes: two passes, four datasets
        with open(tmp_path / "fee.json", "w") as f:
            json.dump([dict(name="low threshold", DISCRIMINATION_THRESHOLD=thr)], f)
        both, _ = run("both.npz", charge_universes=str(tmp_path / "uni.json"), fee_universes=str(tmp_path / "fee.json"),
                      raw_arrays=True)
        assert set(both) == set(a) | {"fee_universes", "fee_universe_hits"}
        assert both["charge_universe_hits"].tobytes() == hits.tobytes() and both["charge_universes"].tobytes() == rows.tobytes()
        # the FEE pass beside it gives what the combined universe gives without its charge change ... and with it, other hits
        fee_hits = both["fee_universe_hits"]
        assert len(fee_hits) > 50 and len(fee_hits) != len(hits[hits["universe"] == 2])
        # the compact path (no --raw_arrays) writes the same rows, launch after launch
        compact, _ = run("compact.npz", charge_universes=str(tmp_path / "uni.json"))
        order = lambda h: np.sort(h, order=["universe", "event_id", "pixel_id", "slot"])          # noqa: E731
        assert order(compact["charge_universe_hits"]).tobytes() == order(hits).tobytes()
    finally:
        H.load_cfg("module0")
        for fld, (ns, name) in _CONSTS.items():
            setattr(getattr(consts, ns), name, nominal[fld])
        _table_mode(synth.make_response("survey"))


def test_nominal_is_the_launch_at_radius_3():
    """universes(charge=[nominal]) over a launch at neighbour radius 3 (module0, TRAN_DIFF x 16) is that launch bit for bit, every
    weight exactly 1.0, as in test 1: the pass walks the launch's slot list, in which the pixels whose every pair carries ring
    code -1 have no slot."""
    H.load_module0_wide(H.RADIUS3_SCALE)
    try:
        seg, resp = H.radius3_segments(), synth.make_response("survey")
        assert H.oracle_radius(seg) == 3
        ch = ChargeChain(resp)
        _upload(ch, seg, np.zeros(len(seg), dtype=np.int32))
        own = _launch_result(ch)
        nominal = CU.nominal(CU.BIRKS)
        assert nominal == ch.charge_variation_nominal()
        u = ch.universes(charge=[nominal], dense=True)[0]
    finally:
        H.load_cfg("module0")
    no_slot = (own["track_pixel_map"] >= 0).sum(axis=1) == 0
    assert no_slot.sum() >= 10 and u["n_hits"] >= 5
    assert (u["weights"] == 1.0).all() and len(u["weights"]) == len(seg) and u["n_unweightable"] == 0
    _assert_same(u, own, "radius 3")
    assert not u["adc_list"][no_slot].any() and not u["hit_count"][no_slot].any()
