"""GPU: pixel current waveforms (ChargeChain.pixel_waveforms, ldsim_chain_pixel_waveforms, simulate_pixels.py --pixel_waveforms).

The reference for S[t] is the project's own: the oracle's sum_pixel_signals, compared tick by tick under the project's bar
(helpers.assert_wave_close: 1e-5 |ref_t| + 1e-7 peak) -- no new number.  The compact form has no tolerance: it is the numpy
statement of the definition (larndsim_amd/pixel_waveforms.py) applied to the device's own dense S, bit for bit."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

import helpers as H
from larndsim_amd import batching, consts, detsim, lib, synth
from larndsim_amd import pixel_truth as PT
from larndsim_amd import pixel_waveforms as PW
from larndsim_amd.chain import ChargeChain
from larndsim_amd.layout import segments_dtype
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
# The module0 case: synth.make_segments(300, seed=SEED) in three unequal batches and a run with batch id < 0 (seed 31, the case of
# test_gpu_pixel_truth.py), with four of batch 0's segments made synthetic by _add_synthetic, for what no seed gives:
# - The segments of one synthetic event that reach a pixel arrive within about 20 ticks of each other at every seed tried (1..8
#   and 31), so no pixel has two spans.  Segments 1 and 2 become copies of segment 0 moved along the drift axis by ECHO_TICKS: the
#   near one gives the pixels of that segment a second run of active ticks that pads of 63 and 64 join to the first, the far one a
#   run no pad reaches.
# - The dense form holds (float)S while a tick is active by its unrounded f64 S, so a threshold taken from a dense sample says
#   nothing about that sample's own tick unless its S is exactly an f32: a sum of one slot.  Segment 3 becomes a copy of segment 0
#   moved in the pixel plane to pixels no other segment of the batch reaches, with LONE_DE times the energy: its peak is the
#   launch's largest |S| (79 007 against 22 251 in the oracle's sums) and a one-slot sum, so "threshold = the largest |S|" tests
#   the strict comparison on an exact tie.
# - No signal of the case comes within 64 ticks of an end of the time axis.  Segment 4 becomes a copy of segment 0 moved in the
#   pixel plane and LATE_US later: its signal (ticks 1892 .. 2000 in the oracle's sums) is cut off by the last tick, N_t - 1,
#   so its spans are clipped there.
# With them the oracle's S through PW.compact_of on the CPU holds every condition test_compact_form_is_the_definition asserts at
# seed 31: spans crossing a multiple of 64 ticks, merges caused by padding, a span clipped at N_t - 1, pixels with several spans
# and pixels with none.
SEED = 31
ECHO_TICKS = (90, 400)
LONE_SHIFT, LONE_DE = (5.0, -20.0), 30.0      # cm in the pixel plane (x, y here); factor on dE
LATE_SHIFT, LATE_US = (10.0, -20.0), 100.0    # cm in the pixel plane; microseconds on t0
SIZES = [(0, 90), (1, 47), (-1, 30), (2, 133)]          # (batch id, segments)
TABLE = [(0, 0, 0, 90), (0, 1, 0, 47), (1, 0, 0, 133)]   # their identities (event, TPC group, sub-batch, n) for the keyed streams
PADS = (0, 1, 7, 63, 64)


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
    """segments 1 and 2 become copies of segment 0 moved along the drift axis (z here) by ECHO_TICKS ticks of drift, towards the
    side of its TPC that has the room; segment 3 a copy moved by LONE_SHIFT in the pixel plane with LONE_DE times the energy
    (dEdx, which sets the recombination, stays); segment 4 a copy moved by LATE_SHIFT and LATE_US later.  They keep their own
    segment ids."""
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
    """(unique pixels, track_pixel_map, S f64 [U][N_t]) of one batch: the oracle's sum_pixel_signals"""
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
    ps, _, ovf = O.sum_pixel_signals(sig, starts, pim, tpm, len(upix), want_tracks=False)
    return dict(upix=upix, tpm=tpm, S=ps, ovf=ovf)


@functools.lru_cache(maxsize=None)
def _module0_case():
    """the segments, their batch ids, the response and the oracle's sums per batch: made once, read only"""
    seg = _add_synthetic(_segments())
    bid = np.concatenate([np.full(n, b) for b, n in SIZES]).astype(np.int32)
    resp = synth.make_response("survey")
    refs = {b: _oracle_sums(seg[bid == b], resp) for b, _ in SIZES if b >= 0}
    for a in [seg, bid, resp] + [v for r in refs.values() for v in r.values()]:
        a.setflags(write=False)
    return seg, bid, resp, refs


def _launch(ch, seg, bid, b0=0, e0=None, keyed=None):
    ch.upload(seg.copy(), bid)
    if keyed is not None:
        ch.set_batch_keys(TABLE, -1)
    ch.quench_drift()
    st = ch.run(b0, len(seg) if e0 is None else e0, want_fractions=False)
    return st, ch.download()


def _meta(out):
    n_hits, _ = PT.hits_of(out["adc_list"])
    return dict(row=np.arange(len(out["unique_pix"])), pixel_id=out["unique_pix"], batch=out["batch"], n_hits=n_hits)


def _assert_dense_matches_oracle(out, S, refs, batches, what):
    worst = 0.0
    for b in batches:
        o, m = refs[b], out["batch"] == b
        assert np.array_equal(out["unique_pix"][m], o["upix"]), what
        assert S[m].shape == o["S"].shape, (what, S[m].shape, o["S"].shape)
        ref = o["S"]
        tol = 1e-5 * np.abs(ref) + 1e-7 * np.abs(ref).max(axis=-1, keepdims=True)
        lit = tol > 0
        worst = max(worst, float(np.max(np.abs(S[m].astype(np.float64) - ref)[lit] / tol[lit])))
        print(f"{what} batch {b}: {int(m.sum())} pixels, worst error / tolerance so far {worst:.3g}")
        H.assert_wave_close(S[m], ref, what=f"{what} batch {b}")
        assert (S[m][np.abs(ref).max(axis=-1) == 0] == 0).all(), what       # a pixel the oracle leaves dark is exactly 0
    return worst


def _same_compact(got, want, what=""):
    """span rows, sample_begin and sample bits"""
    assert got["n_ticks"] == want["n_ticks"], what
    assert len(got["spans"]) == len(want["spans"]) and len(got["samples"]) == len(want["samples"]), \
        (what, len(got["spans"]), len(want["spans"]), len(got["samples"]), len(want["samples"]))
    for f in PW.SPAN_ROW.names:
        assert np.array_equal(got["spans"][f], want["spans"][f]), (what, f)
    assert np.array_equal(got["samples"].view(np.uint32), want["samples"].view(np.uint32)), what


def test_dense_against_the_oracle_whole_and_sub_range():
    """1. ~300 synthetic segments, three unequal batches and a run with batch id < 0, launched whole and as a sub-range with
    seg_begin > 0: dense S of every row against the oracle's sum_pixel_signals, tick by tick"""
    seg, bid, resp, refs = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    st, out = _launch(ch, seg, bid)
    S = ch.pixel_waveforms(dense=True)
    assert S.dtype == np.float32 and S.shape == (st.n_unique, len(consts.detector.TIME_TICKS))
    assert sorted(set(out["batch"].tolist())) == [0, 1, 2] and st.n_unique == sum(len(r["upix"]) for r in refs.values())
    _assert_dense_matches_oracle(out, S, refs, (0, 1, 2), "whole")
    # a row range is those rows of the whole
    U = int(st.n_unique)
    for b, e in ((0, 1), (U // 3, U // 3 + 5), (U - 3, U), (7, 7)):
        assert np.array_equal(ch.pixel_waveforms(dense=True, rows=(b, e)), S[b:e])
    assert np.array_equal(ch.pixel_waveforms(dense=True, rows=range(2, 9)), S[2:9])
    b0 = SIZES[0][1]
    st2, out2 = _launch(ch, seg, bid, b0=b0)
    S2 = ch.pixel_waveforms(dense=True)
    assert sorted(set(out2["batch"].tolist())) == [1, 2]
    _assert_dense_matches_oracle(out2, S2, refs, (1, 2), "sub-range")
    assert np.array_equal(S2, S[out["batch"] >= 1])


def test_dense_two_response_samples_per_tick():
    """1. TIME_SAMPLING / RESPONSE_SAMPLING = 2 (the ndlar snapshot), 80 segments in one batch"""
    seg = _segments("ndlar", n=80, seed=8)
    det = consts.detector
    assert int(round(det.TIME_SAMPLING / det.RESPONSE_SAMPLING)) == 2
    try:
        resp = H.response_for("golden")
        ref = _oracle_sums(seg, resp)
        ch = ChargeChain(resp)
        ch.upload(seg.copy(), np.zeros(len(seg), dtype=np.int32))
        ch.quench_drift()
        st = ch.run()
        out, S = ch.download(), ch.pixel_waveforms(dense=True)
        assert st.n_unique == len(ref["upix"]) > 50
        _assert_dense_matches_oracle(out, S, {0: ref}, (0,), "ndlar")
        _same_compact(ch.pixel_waveforms(0.0, 7), PW.compact_of(S, _meta(out), 0.0, 7), "ndlar")
    finally:
        H.load_cfg("module0")


def _column_segments(n=10):
    """n short parallel segments over one pixel column of TPC 0"""
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


def test_dense_more_pairs_than_slots_on_a_pixel():
    """1. MAX_TRACKS_PER_PIXEL = 4 and ten parallel segments over one pixel column: S is the sum over the slots only, as the FEE's"""
    H.load_cfg("module0")
    consts.sim.MAX_TRACKS_PER_PIXEL = 4
    try:
        seg = _column_segments(10)
        resp = synth.make_response("survey")
        ref = _oracle_sums(seg, resp)
        ch = ChargeChain(resp)
        ch.upload(seg.copy(), np.zeros(len(seg), dtype=np.int32))
        ch.quench_drift()
        st = ch.run()
        out, S = ch.download(), ch.pixel_waveforms(dense=True)
        assert st.n_overflow > 0 and ref["ovf"].any() and (ref["tpm"] >= 0).all(axis=1).any()
        assert np.array_equal(out["track_pixel_map"], ref["tpm"])
        _assert_dense_matches_oracle(out, S, {0: ref}, (0,), "M = 4")
        _same_compact(ch.pixel_waveforms(0.0, 1), PW.compact_of(S, _meta(out), 0.0, 1), "M = 4")
    finally:
        H.load_cfg("module0")


def _fresh_launch():
    """the module0 case launched on a new ChargeChain (the ctx is process-wide: other tests upload other segments)"""
    seg, bid, resp, refs = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    st, out = _launch(ch, seg, bid)
    return ch, st, out


@functools.lru_cache(maxsize=None)
def _device_case():
    """the rows of the module0 launch, the device's dense S and the thresholds taken from it: made once, read only"""
    ch, st, out = _fresh_launch()
    S = ch.pixel_waveforms(dense=True)
    a = np.abs(S[S != 0]).astype(np.float64)
    thr = (0.0, float(np.median(a)), float(np.quantile(a, 0.99)), float(a.max()), 2 * float(a.max()))
    S.setflags(write=False)
    return out, S, thr


def test_compact_form_is_the_definition():
    """2. span rows, sample_begin and sample bits against PW.compact_of of the device's own dense S: thresholds 0, the median
    and the 0.99 quantile of the non-zero |S|, and twice the largest |S| (no tick active: sizes 0, 0); pads 0, 1, 7, 63, 64;
    hits_only off and on.  The end asserts, from the twin's output, what the cases together contained.  The fifth threshold,
    the largest |S| itself, is test_no_tick_is_active_at_the_largest_sample."""
    out, S, thrs = _device_case()
    ch, st, again = _fresh_launch()
    assert np.array_equal(again["unique_pix"], out["unique_pix"]) and np.array_equal(ch.pixel_waveforms(dense=True), S)
    meta, (U, NT) = _meta(out), S.shape
    assert (meta["n_hits"] > 0).any() and (meta["n_hits"] == 0).any()
    seen = dict(crosses_64=False, pad_merges=False, clipped=False, several=False, none=False)
    for i, thr in enumerate(thrs):
        if i == 3:
            continue
        bare = np.bincount(PW.compact_of(S, meta, thr, 0)["spans"]["row"], minlength=U)      # runs of active ticks per pixel
        for pad in PADS:
            for hits_only in (False, True):
                want = PW.compact_of(S, meta, thr, pad, hits_only)
                got = ch.pixel_waveforms(thr, pad, hits_only)
                print(f"threshold {thr!r} pad {pad} hits_only {hits_only}: device {len(got['spans'])} spans, "
                      f"{len(got['samples'])} samples; definition {len(want['spans'])}, {len(want['samples'])}")
                _same_compact(got, want, f"threshold {thr!r} pad {pad} hits_only {hits_only}")
                if i >= 3:
                    assert len(got["spans"]) == 0 and len(got["samples"]) == 0 and got["n_ticks"] == NT
                sp = want["spans"]
                last = sp["t_begin"].astype(np.int64) + sp["n_samples"] - 1
                per_pixel = np.bincount(sp["row"], minlength=U)
                seen["crosses_64"] |= bool((sp["t_begin"] // 64 != last // 64).any())
                seen["clipped"] |= bool(((sp["t_begin"] == 0) | (last == NT - 1)).any())
                seen["several"] |= bool((per_pixel > 1).any())
                seen["none"] |= bool((per_pixel == 0).any()) and len(sp) > 0
                if not hits_only:                                    # a pixel whose runs the padding joined
                    seen["pad_merges"] |= bool(((per_pixel < bare) & (per_pixel > 0)).any())
    print("the cases contained:", seen)
    for k in ("crosses_64", "pad_merges", "clipped", "several", "none"):
        assert seen[k], k
    assert (S[:, -1] != 0).any()                                     # (the late segment's signal reaches the last tick)


def test_no_tick_is_active_at_the_largest_sample():
    """2. the threshold "the largest |S|" of the device's dense S: the comparison is strict, so no tick is active and the sizes
    are 0, 0 at every pad, as the twin finds.  The dense form holds (float)S and the comparison is made on the unrounded S, so the
    case says something only where the two are the same number: the test asserts that the pixel holding the largest sample has
    one filled slot (the lone segment of _add_synthetic), whose S is its f32 current row exactly.  (Where the largest sample
    is a sum of several slots that rounding moved down, the unrounded |S| exceeds the rounded threshold and that tick is active
    by the definition: test_largest_sample_threshold_keeps_only_ties states what holds then.)"""
    out, S, thrs = _device_case()
    ch, st, _ = _fresh_launch()
    meta, NT = _meta(out), S.shape[1]
    assert thrs[3] == float(np.abs(S).max())
    rows = np.unique(np.nonzero(np.abs(S) == np.float32(thrs[3]))[0])
    assert ((out["track_pixel_map"][rows] >= 0).sum(axis=1) == 1).all(), "the largest sample is a one-slot sum: exact in f32"
    for pad in PADS:
        for hits_only in (False, True):
            want = PW.compact_of(S, meta, thrs[3], pad, hits_only)
            got = ch.pixel_waveforms(thrs[3], pad, hits_only)
            print(f"threshold {thrs[3]!r} pad {pad} hits_only {hits_only}: device {len(got['spans'])} spans, "
                  f"{len(got['samples'])} samples; definition {len(want['spans'])}, {len(want['samples'])}")
            assert len(want["spans"]) == 0
            _same_compact(got, want, f"largest |S| {thrs[3]!r} pad {pad} hits_only {hits_only}")
            assert len(got["spans"]) == 0 and len(got["samples"]) == 0 and got["n_ticks"] == NT


def test_largest_sample_threshold_keeps_only_ties():
    """2. what the definition guarantees at the threshold "the largest |S|" of the rounded samples: rounding is monotonic, so a
    tick whose unrounded |S| exceeds it holds exactly that sample -- at pad 0 every kept sample equals the threshold in
    magnitude, and the compact form is the definition's for those active ticks"""
    out, S, thrs = _device_case()
    ch, st, _ = _fresh_launch()
    got = ch.pixel_waveforms(thrs[3], 0)
    assert (np.abs(got["samples"]).astype(np.float64) == thrs[3]).all()
    assert (got["spans"]["n_samples"] == 1).all() or len(got["spans"]) == 0          # (pad 0: the active ticks themselves)
    active = PW.expand(got["spans"], got["samples"], *S.shape) != 0
    assert np.array_equal(S[active], got["samples"])
    meta = _meta(out)
    for pad in PADS:
        _same_compact(ch.pixel_waveforms(thrs[3], pad), _twin_for_active(S, active, meta, pad), f"ties, pad {pad}")


def _twin_for_active(S, active, meta, pad):
    """the compact form the definition gives for dense rows S and a given set of active ticks"""
    marks = PW.compact_of(active.astype(np.float32), meta, 0.0, pad)                 # spans of the kept ticks
    kept = PW.expand(marks["spans"], np.ones(len(marks["samples"]), np.float32), *S.shape) != 0
    return dict(spans=marks["spans"], samples=S[kept].astype(np.float32), n_ticks=S.shape[1])


def test_consistent_with_pixel_truth():
    """3. threshold 0, pad 0: dt * sum of a pixel's samples is q_induced within q_abs * 2^-23 (each sample is S rounded to f32,
    half an ulp = 2^-24 |S| at most; the rest covers the order of the f64 sums); every pixel with a hit has a span; pixel truth
    before, after and between waveform passes leaves both results bit-identical"""
    out, S, thrs = _device_case()
    ch, st, _ = _fresh_launch()
    U, dt = int(st.n_unique), consts.detector.TIME_SAMPLING
    t0 = ch.pixel_truth(dense=True)
    w0 = ch.pixel_waveforms()
    t1 = ch.pixel_truth(dense=True)
    c1 = ch.pixel_truth(0.0)
    w1 = ch.pixel_waveforms(thrs[1], 7)
    t2 = ch.pixel_truth(dense=True)
    w2 = ch.pixel_waveforms()
    c2 = ch.pixel_truth(0.0)
    w3 = ch.pixel_waveforms(thrs[1], 7)
    for k in t0:
        assert np.array_equal(t0[k], t1[k]) and np.array_equal(t0[k], t2[k]), k
    for k in ("pixels", "tracks"):
        assert np.array_equal(c1[k], c2[k]), k
    _same_compact(w0, w2, "threshold 0 again")
    _same_compact(w1, w3, "median threshold again")
    sp = w0["spans"]
    per_span = np.add.reduceat(w0["samples"].astype(np.float64), sp["sample_begin"]) if len(sp) else np.zeros(0)
    q = dt * np.bincount(sp["row"], weights=per_span, minlength=U)
    err, bound = np.abs(q - t0["q_induced"]), t0["q_abs"] * 2.0 ** -23
    print("dt * sum(samples) - q_induced, worst error / bound:", float(np.max(err[bound > 0] / bound[bound > 0])))
    assert (err <= bound).all()
    n_hits, _ = PT.hits_of(out["adc_list"])
    assert (n_hits > 0).any() and (np.bincount(sp["row"], minlength=U)[n_hits > 0] >= 1).all()


def test_same_bits_from_both_layouts_any_chunking_and_under_noise():
    """4. the set-up record as two lists (default) and as headers [U] (fee_one_class); one launch against one launch per batch;
    keyed FEE noise on against off"""
    seg, bid, resp, refs = _module0_case()
    out, S, thrs = _device_case()
    ch, st, _ = _fresh_launch()
    sel = (thrs[1], 7)
    base = ch.pixel_waveforms(*sel)
    base_hits = ch.pixel_waveforms(*sel, hits_only=True)
    assert 0 < len(base_hits["spans"]) < len(base["spans"])
    try:
        lib.set_option("fee_one_class", 1)
        ch.run(want_fractions=False)
        assert np.array_equal(ch.pixel_waveforms(dense=True), S)
        _same_compact(ch.pixel_waveforms(*sel), base, "headers [U]")
        _same_compact(ch.pixel_waveforms(*sel, hits_only=True), base_hits, "headers [U], hits only")
    finally:
        lib.set_option("fee_one_class", 0)
    # one launch per batch: the rows count from each launch's 0, the samples from each launch's first
    edges = np.r_[0, np.cumsum([n for _, n in SIZES])]
    parts = []
    for (b, n), lo, hi in zip(SIZES, edges[:-1], edges[1:]):
        if b >= 0:
            ch.run(int(lo), int(hi), want_fractions=False)
            parts.append(ch.pixel_waveforms(*sel))
    joined = np.concatenate([p["spans"] for p in parts])
    for k in ("pixel_id", "batch", "t_begin", "n_samples"):
        assert np.array_equal(joined[k], base["spans"][k]), k
    assert np.array_equal(np.concatenate([p["samples"] for p in parts]).view(np.uint32), base["samples"].view(np.uint32))
    # FEE noise moves the hits, never S
    H.load_cfg("module0", noise_zero=False)
    assert consts.detector.RESET_NOISE_CHARGE > 0 and consts.detector.UNCORRELATED_NOISE_CHARGE > 0
    try:
        noisy = ChargeChain(resp)
        noisy.seed_keyed(20260131)
        _launch(noisy, seg, bid, keyed=True)
        assert np.array_equal(noisy.pixel_waveforms(dense=True), S)
        _same_compact(noisy.pixel_waveforms(*sel), base, "keyed FEE noise")
    finally:
        H.load_cfg("module0")
        ChargeChain(resp).seed_rng(1, n_states=64)                  # (the ctx is process-wide: back to table mode)


def test_state_rules_and_bad_arguments():
    """5. LDSIM_ESTATE after reset, upload, quench_drift and a host-array tracks_current, and from the download before a pass;
    LDSIM_EINVAL for the bad arguments; a launch without unique pixels gives zeros"""
    seg, bid, resp, refs = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    st, out = _launch(ch, seg, bid)
    L, U = lib.load(), int(st.n_unique)
    sizes = (C.c_int64 * 3)()
    # the download before a pass of this launch
    rc = L.ldsim_chain_pixel_waveforms_download(ch.ctx, None, None)
    assert rc == -4 and b"ldsim_chain_pixel_waveforms has not run for the last chain launch" in L.ldsim_last_error()
    assert L.ldsim_chain_pixel_waveforms_ms(ch.ctx, None, None) == -4
    ch.pixel_waveforms(1e300)                                        # no tick active: the fill kernel is not launched
    count_ms, fill_ms = ch.pixel_waveforms_ms()
    assert count_ms > 0 and fill_ms == 0
    base = ch.pixel_waveforms(0.0, 3)
    assert L.ldsim_chain_pixel_waveforms_download(ch.ctx, None, None) == 0
    count_ms, fill_ms = ch.pixel_waveforms_ms()
    assert count_ms > 0 and fill_ms > 0
    NT = base["n_ticks"]
    assert NT == len(consts.detector.TIME_TICKS) and len(base["spans"]) > 0
    # bad arguments: LDSIM_EINVAL, nothing counted
    for thr, pad in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.0, -1), (0.0, 65)):
        rc = L.ldsim_chain_pixel_waveforms(ch.ctx, C.c_double(thr), C.c_int32(pad), C.c_int32(0), sizes)
        assert rc == -1 and tuple(sizes) == (0, 0, 0), (thr, pad, rc)
    row = np.zeros((2, NT), dtype=np.float32)
    for b, e in ((-1, 1), (2, 1), (U - 1, U + 1), (U + 1, U + 1)):
        assert L.ldsim_chain_pixel_waveforms_dense(ch.ctx, C.c_int64(b), C.c_int64(e), lib.ptr(row)) == -1, (b, e)
    assert L.ldsim_chain_pixel_waveforms_dense(ch.ctx, C.c_int64(0), C.c_int64(1), None) == -1
    assert L.ldsim_chain_pixel_waveforms_dense(ch.ctx, C.c_int64(U), C.c_int64(U), None) == 0       # (an empty range writes nothing)
    _same_compact(ch.pixel_waveforms(0.0, 3), base, "after the refused calls")

    def refused(word):
        for kw in (dict(), dict(dense=True), dict(dense=True, rows=(0, 1))):
            with pytest.raises(lib.LdsimError, match=rf"ldsim error -4: .*ldsim_chain_pixel_waveforms.*{word}"):
                ch.pixel_waveforms(**kw)

    def rerun():
        ch.run(want_fractions=False)
        _same_compact(ch.pixel_waveforms(0.0, 3), base, "after a fresh run")

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
    assert L.ldsim_chain_pixel_waveforms_download(ch.ctx, None, None) == -4
    # nothing to simulate: every batch id negative
    ch.upload(seg.copy(), np.full(len(seg), -1, dtype=np.int32))
    ch.quench_drift()
    assert ch.run().n_unique == 0
    lib.check(L.ldsim_chain_pixel_waveforms(ch.ctx, C.c_double(0.0), C.c_int32(64), C.c_int32(1), sizes))
    assert tuple(sizes) == (0, 0, NT)
    empty = ch.pixel_waveforms()
    assert len(empty["spans"]) == 0 and len(empty["samples"]) == 0 and empty["n_ticks"] == NT
    assert ch.pixel_waveforms(dense=True).shape == (0, NT)
    assert ch.pixel_waveforms_ms() == (0.0, 0.0)


def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_pixel_waveforms_gpu", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _assert_same_bytes(x, y, what):
    """byte for byte; field by field for records (the padding bytes of an aligned record are not data)"""
    assert x.shape == y.shape and x.dtype == y.dtype, what
    for f in (x.dtype.names or [None]):
        xa, ya = (x, y) if f is None else (x[f], y[f])
        assert np.ascontiguousarray(xa).tobytes() == np.ascontiguousarray(ya).tobytes(), (what, f)


def test_driver_writes_both_datasets(tmp_path, capsys):
    """6. --pixel_waveforms: both datasets, equal to a ChargeChain run by hand on the same batches (the same rows up to the
    file-wide sample_begin) at --chunk_segments 40 and 100000; the rest of the file and the printed header are what they are
    without the flag (.npz stream: the interpreter of the GPU tests has no h5py)"""
    cli = _cli()
    H.load_cfg("module0")
    seg = synth.make_segments(200, seed=21, segs_per_event=40)          # 5 events
    seg = seg[np.random.default_rng(2).permutation(len(seg))]
    np.save(tmp_path / "in.npy", seg)
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    common = dict(input_filename=str(tmp_path / "in.npy"), config="module0", rand_seed=7, rng="keyed", light_simulated=False,
                  response_file=str(tmp_path / "resp.npy"))
    sel = dict(pixel_waveforms_threshold=0.5, pixel_waveforms_pad=5)

    def run(name, **kw):
        cli.run_simulation(output_filename=str(tmp_path / name), **common, **kw)
        with np.load(tmp_path / name) as f:
            return {k: f[k] for k in f.files}, capsys.readouterr().out

    a, log_a = run("w40.npz", pixel_waveforms=True, chunk_segments=40, **sel)
    assert "Pixel current waveforms: on (--pixel_waveforms, --pixel_waveforms_threshold 0.5, --pixel_waveforms_pad 5)" in log_a
    b, _ = run("w1e5.npz", pixel_waveforms=True, chunk_segments=100000, **sel)
    plain, log = run("plain.npz", chunk_segments=40)
    assert "Pixel current waveforms" not in log
    hits, _ = run("hits.npz", pixel_waveforms=True, pixel_waveforms_hits_only=True, chunk_segments=40, **sel)
    assert set(a) == set(b) == set(hits) == set(plain) | {"pixel_waveforms", "pixel_waveform_samples"}
    for k in a:
        _assert_same_bytes(a[k], b[k], k)
    for k in plain:
        _assert_same_bytes(a[k], plain[k], k)
    sp, sam = a["pixel_waveforms"], a["pixel_waveform_samples"]
    assert sp.dtype == PW.FILE_SPAN and sam.dtype == np.float32 and len(sp) > 100
    assert np.array_equal(sp["sample_begin"], np.cumsum(sp["n_samples"], dtype=np.int64) - sp["n_samples"])     # tiles the samples
    assert int(sp["n_samples"].sum()) == len(sam)
    assert 0 < len(hits["pixel_waveforms"]) < len(sp)
    # by hand: the driver's batches through a ChargeChain, every batch in one launch
    consts.load_snapshot("module0")
    tracks, _ = cli.load_input(str(tmp_path / "in.npy"))
    tracks = cli.prepare_tracks(tracks)
    tracks = tracks[batching.select_active_volume(tracks, consts.detector.TPC_BORDERS)]
    bid, order, table = batching.assign_batches(tracks, tpc_borders=consts.detector.TPC_BORDERS)
    tracks, bid = np.ascontiguousarray(tracks[order]), bid[order]
    try:
        lib.set_option("numba_f32", cli.numba_f32_mode("auto", tracks.dtype))
        ch = ChargeChain(synth.make_response("survey"))
        ch.clear_pixel_tables()
        ch.seed_keyed(7)
        ch.upload(tracks, bid)
        ch.set_batch_keys(table, -1)
        ch.quench_drift()
        ch.run(0, int((bid >= 0).sum()), want_fractions=True)
        hand = ch.pixel_waveforms(0.5, 5)
        hand_hits = ch.pixel_waveforms(0.5, 5, hits_only=True)
    finally:
        lib.set_option("numba_f32", 0)
        ChargeChain(synth.make_response("survey")).seed_rng(1, n_states=64)
        H.load_cfg("module0")
    for got, want in ((a, hand), (hits, hand_hits)):
        rows, samples = PW.file_rows(want, [t[0] for t in table])
        _assert_same_bytes(got["pixel_waveforms"], rows, "pixel_waveforms")
        _assert_same_bytes(got["pixel_waveform_samples"], samples, "pixel_waveform_samples")
    # empty, the datasets exist all the same
    none, _ = run("none.npz", pixel_waveforms=True, pixel_waveforms_threshold=1e30, chunk_segments=40)
    assert none["pixel_waveforms"].dtype == PW.FILE_SPAN and len(none["pixel_waveforms"]) == 0
    assert none["pixel_waveform_samples"].dtype == np.float32 and len(none["pixel_waveform_samples"]) == 0


def test_dense_radius_3_launch_with_pixels_without_a_slot():
    """A launch at neighbour radius 3 (module0, TRAN_DIFF x 16): the pixels whose every pair carries ring code -1 are rows of the
    launch with no slot (pixels_from_track.py:251-252, detsim.py:582); their waveform is exactly 0, every other row is the
    oracle's sum_pixel_signals as in test 1."""
    H.load_module0_wide(H.RADIUS3_SCALE)
    try:
        seg, resp = H.radius3_segments(), synth.make_response("survey")
        assert H.oracle_radius(seg) == 3
        ref = _oracle_sums(seg, resp)
        ch = ChargeChain(resp)
        st, out = _launch(ch, seg, np.zeros(len(seg), dtype=np.int32))
        S = ch.pixel_waveforms(dense=True)
        compact = ch.pixel_waveforms()
    finally:
        H.load_cfg("module0")
    no_slot = (ref["tpm"] >= 0).sum(axis=1) == 0
    assert no_slot.sum() >= 10 and not ref["S"][no_slot].any() and st.n_unique == len(ref["upix"])
    assert np.array_equal(out["track_pixel_map"], ref["tpm"])
    _assert_dense_matches_oracle(out, S, {0: ref}, (0,), "radius 3")
    assert not S[no_slot].any() and S[~no_slot].any()
    assert not np.isin(compact["spans"]["row"], np.flatnonzero(no_slot)).any()      # no span on a pixel without a slot
