"""GPU: the front of a chain launch -- the segment pass, get_pixels writing its own empty slots, the keyed selection, the pair-list
sort over two bit ranges, the head scan and the read-backs -- through ChargeChain on sets of at most 64 segments.

Every launch is compared with the CPU oracle per batch: unique_pix, batch, track_pixel_map (its slot order is the order of the
sorted pair list among equal pixels), adc_ticks_list and adc_digit exactly, adc_list as test_fused_chain_vs_oracle_two_batches
does.  The oracle's currents cost 40 ms per (segment, pixel) pair, so the segments are short (one or two pixels each) and the
oracle of a set is computed once (lru_cache) and read only; the 64-segment set takes the oracle about half a minute."""
import functools

import numpy as np
import pytest

import helpers as H
from larndsim_amd import consts, lib, synth
from larndsim_amd.chain import ChargeChain
from larndsim_amd.layout import segments_dtype

pytestmark = pytest.mark.gpu

# TRAN_DIFF factors that give short segments at mid-drift the neighbour radius 0 .. 4 (5 tran_diff / PIXEL_PITCH is 0.45 .. 0.48
# there for module0 and 2x2_no_modvar); every test asserts the radius the oracle derives
SCALE_OF_RADIUS = {0: 0, 1: 1, 2: 6, 3: 28, 4: 50}
OUT_KEYS = ("unique_pix", "batch", "track_pixel_map", "adc_list", "adc_ticks_list", "adc_digit", "current_fractions")


def _load(cfg, radius):
    H.load_cfg(cfg)
    consts.detector.TRAN_DIFF = consts.detector.TRAN_DIFF * SCALE_OF_RADIUS[radius]


def _short_segments(pixels, seed, outside=()):
    """one segment of a few hundred microns per entry (tpc, px, py) of `pixels`, inside that pixel or reaching into a neighbour,
    at mid-drift; the segments whose index is in `outside` are moved out of every TPC"""
    det = consts.detector
    n = len(pixels)
    rng = np.random.default_rng(seed)
    seg = np.zeros(n, dtype=segments_dtype)
    half = 0.35 * det.PIXEL_PITCH
    for i, (tpc, px, py) in enumerate(pixels):
        b = np.sort(det.TPC_BORDERS[tpc], axis=-1)
        seg["x_start"][i] = b[0][0] + (px + 0.5) * det.PIXEL_PITCH + rng.uniform(-half, half)
        seg["y_start"][i] = b[1][0] + (py + 0.5) * det.PIXEL_PITCH + rng.uniform(-half, half)
        seg["z_start"][i] = b[2][0] + rng.uniform(0.45, 0.55) * (b[2][1] - b[2][0])
    seg["x_end"] = seg["x_start"] + rng.uniform(0.01, 0.05, n) * rng.choice([-1, 1], n)
    seg["y_end"] = seg["y_start"] + rng.uniform(-0.05, 0.05, n)
    seg["z_end"] = seg["z_start"] + rng.uniform(-0.07, 0.07, n)
    for i in outside:
        for f in ("x_start", "x_end"):
            seg[f][i] += 1.0e4
    for a in "xyz":
        seg[a] = 0.5 * (seg[a + "_start"] + seg[a + "_end"])
    seg["dx"] = np.sqrt(sum((seg[a + "_end"] - seg[a + "_start"]) ** 2 for a in "xyz"))
    seg["dEdx"] = 30.0      # (dense enough that these short segments make hits)
    seg["dE"] = seg["dEdx"] * seg["dx"]
    seg["segment_id"] = np.arange(n)
    seg["event_id"] = 0
    seg["pdg_id"] = 13
    return seg


def _launch(seg, bid, resp, fresh=False):
    """one launch over all of `seg`; fresh: on a context made for it"""
    if fresh:
        lib.destroy_context()
    ch = ChargeChain(resp)
    ch.upload(seg.copy(), np.asarray(bid, dtype=np.int32))
    ch.quench_drift()
    st = ch.run(0, len(seg), want_fractions=True)
    out = ch.download()
    return st, {k: np.array(out[k], copy=True) for k in OUT_KEYS}


def _oracle_per_batch(seg, bid, resp):
    return {int(b): H.oracle_chain(seg[bid == b], resp) for b in np.unique(bid[bid >= 0])}


def _assert_launch(st, out, os_, what=""):
    """a launch against the oracle's chain on each of its batches"""
    assert sorted(set(out["batch"].tolist())) == sorted(b for b, o in os_.items() if len(o["unique_pix"])), what
    assert st.n_unique == sum(len(o["unique_pix"]) for o in os_.values()), what
    assert st.n_pairs == sum(int((o["neigh"] >= 0).sum()) for o in os_.values()), what
    assert (np.diff(out["batch"]) >= 0).all(), what
    for b, o in os_.items():
        m = out["batch"] == b
        assert np.array_equal(out["unique_pix"][m], o["unique_pix"]), (what, b)
        assert np.array_equal(out["track_pixel_map"][m], o["tpm"]), (what, b)
        assert np.array_equal(out["adc_list"][m] != 0, o["adc"] != 0), (what, b)
        np.testing.assert_allclose(out["adc_list"][m], o["adc"], rtol=1e-5, err_msg=f"{what} batch {b}")
        assert np.array_equal(out["adc_ticks_list"][m], o["ticks"]), (what, b)
        assert np.array_equal(out["adc_digit"][m], o["digit"]), (what, b)


def _assert_same(a, b, what):
    for k in OUT_KEYS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


# ---- the sets ------------------------------------------------------------------------------------------------------------------------------
BIG_IDS = [-1] * 4 + [0] * 14 + [1] * 14 + [3] * 14 + [4] * 14 + [-1] * 4      # 5 batches (bb = 3), no segment in batch 2


@functools.lru_cache(maxsize=None)
def _big_case():
    """64 segments at radius 2 in the batches 0, 1, 3, 4 (none in 2) with not-simulated segments (-1) at both ends of the range;
    of the 14 segments of a batch 6 lie outside every TPC and 3 lie over one pixel"""
    _load("module0", 2)
    try:
        rng = np.random.default_rng(41)
        bid = np.array(BIG_IDS, dtype=np.int32)
        pixels, outside = [], []
        for i, b in enumerate(bid):
            k = i - 4 - 14 * [0, 1, -1, 2, 3][b] if b >= 0 else -1      # index within its batch
            tpc = int(b) % 2 if b >= 0 else 0
            if b >= 0 and k in (1, 4, 5, 8, 11, 13):
                outside.append(i)
            if b >= 0 and k in (2, 6, 9):
                pixels.append((tpc, 50, 60 + int(b)))                   # the same pixel three times: equal keys
            else:
                pixels.append((tpc, int(rng.integers(48, 53)), int(rng.integers(58, 66))))
        seg = _short_segments(pixels, 7, outside)
        resp = synth.make_response("survey")
        os_ = _oracle_per_batch(seg, bid, resp)
    finally:
        H.load_cfg("module0")
    for v in (seg, bid, resp):
        v.setflags(write=False)
    return seg, bid, resp, os_


@functools.lru_cache(maxsize=None)
def _small_case():
    """8 segments in one batch under TRAN_DIFF = 0: radius 0, P = max_pixels"""
    _load("module0", 0)
    try:
        seg = _short_segments([(0, 20 + 3 * i, 30) for i in range(8)], 3)
        bid = np.zeros(8, dtype=np.int32)
        resp = synth.make_response("survey")
        os_ = _oracle_per_batch(seg, bid, resp)
    finally:
        H.load_cfg("module0")
    return seg, bid, resp, os_


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------
def test_stale_buffers_big_small_big_equal_fresh_contexts():
    """64 segments at radius 2, then 8 at radius 0 (smaller n, max_pixels and P) on the same context, then the first again: each
    launch equals the same launch on a context of its own, array for array, and the oracle.  A slot of the pixel arrays, the
    keys or the per-batch block that kept a value of the launch before would change a row."""
    seg, bid, resp, os_ = _big_case()
    seg0, bid0, resp0, os0 = _small_case()
    assert all(o["radius"] == 2 for o in os_.values()) and os0[0]["radius"] == 0
    assert os0[0]["P"] < min(o["P"] for o in os_.values())
    got = []
    try:
        lib.destroy_context()
        for radius, (s, b, r) in ((2, (seg, bid, resp)), (0, (seg0, bid0, resp0)), (2, (seg, bid, resp))):
            _load("module0", radius)
            got.append(_launch(s, b, r))
        fresh = []
        for radius, (s, b, r) in ((2, (seg, bid, resp)), (0, (seg0, bid0, resp0))):
            _load("module0", radius)
            fresh.append(_launch(s, b, r, fresh=True))
    finally:
        H.load_cfg("module0")
        lib.destroy_context()
    assert got[1][0].max_neigh < got[0][0].max_neigh and got[1][0].max_active <= got[0][0].max_active
    _assert_same(got[0][1], fresh[0][1], "first launch against a fresh context")
    _assert_same(got[1][1], fresh[1][1], "small launch after the big one against a fresh context")
    _assert_same(got[2][1], fresh[0][1], "big launch after the small one against a fresh context")
    _assert_launch(got[0][0], got[0][1], os_, "big")
    _assert_launch(got[1][0], got[1][1], os0, "small")
    _assert_launch(got[2][0], got[2][1], os_, "big again")


def test_five_batches_with_a_gap_negative_ends_empty_rows_and_equal_keys():
    """The 64-segment set: batch ids 0, 1, 3, 4 (bb = 3; no segment carries 2), -1 at both ends, segments without any pixel mixed
    in, three segments of every batch over one pixel -- their slots in track_pixel_map come in the oracle's order."""
    seg, bid, resp, os_ = _big_case()
    assert sorted(os_) == [0, 1, 3, 4]
    for b, o in os_.items():
        empty = (o["neigh"] >= 0).sum(axis=1) == 0
        assert empty.sum() == 6                                           # rows without a pixel
        shared = (o["tpm"] >= 0).sum(axis=1).max()
        assert shared >= 3                                                # a pixel with several pairs of one batch
    _load("module0", 2)
    try:
        st, out = _launch(seg, bid, resp)
    finally:
        H.load_cfg("module0")
    assert st.n_batches == 5 and 2 not in out["batch"] and (out["batch"] >= 0).all()
    _assert_launch(st, out, os_, "five batches")


@pytest.mark.parametrize("n_batches", [1, 2, 3])
def test_batch_counts_one_two_three(n_batches):
    """bb = 0, 1, 2: six segments in 1, 2 and 3 batches at radius 1, the batches over the same pixels"""
    _load("module0", 1)
    seg = _short_segments([(i % 2, 30 + (i // 2) % 2, 40) for i in range(6)], 5)
    bid = np.repeat(np.arange(n_batches), 6 // n_batches).astype(np.int32)
    resp = synth.make_response("survey")
    os_ = _oracle_per_batch(seg, bid, resp)
    assert all(o["radius"] == 1 for o in os_.values())
    st, out = _launch(seg, bid, resp)
    assert st.n_batches == n_batches
    _assert_launch(st, out, os_, f"{n_batches} batches")


def test_every_segment_outside_returns_empty():
    """no active pixel at all: no valid pair, empty results, and the context serves the next launch"""
    _load("module0", 1)
    seg = _short_segments([(0, 10 + i, 10) for i in range(8)], 9, outside=range(8))
    resp = synth.make_response("survey")
    st, out = _launch(seg, np.zeros(8, dtype=np.int32), resp)
    assert st.n_pairs == 0 and st.n_unique == 0
    assert len(out["unique_pix"]) == 0 and len(out["batch"]) == 0 and out["adc_list"].shape[0] == 0
    seg2 = _short_segments([(0, 10 + i, 10) for i in range(4)], 9)
    bid2 = np.zeros(4, dtype=np.int32)
    st, out = _launch(seg2, bid2, resp)
    _assert_launch(st, out, _oracle_per_batch(seg2, bid2, resp), "after the empty launch")


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("cfg", ["module0", "2x2_no_modvar"])
def test_last_pixel_of_the_last_tpc(cfg, radius):
    """A segment over the last pixel of the last TPC: the largest pixel id the constants allow is in a key, with every ring
    code the radius reaches (0-8 at radius 4) in the low four bits.  (One segment: the oracle's currents for the 81 pixels of
    radius 4 take it ten seconds.)"""
    _load(cfg, radius)
    try:
        det = consts.detector
        last = (det.TPC_BORDERS.shape[0] - 1, det.N_PIXELS[0] - 1, det.N_PIXELS[1] - 1)
        seg = _short_segments([last], 13)
        seg["x_end"] = seg["x_start"] - 0.02      # towards the pixels before it: the walk never leaves the plane
        seg["y_end"] = seg["y_start"] - 0.02
        for a in "xy":
            seg[a] = 0.5 * (seg[a + "_start"] + seg[a + "_end"])
        bid = np.array([0], dtype=np.int32)
        resp = H.response_for("survey")
        os_ = _oracle_per_batch(seg, bid, resp)
        pixel_max = det.N_PIXELS[0] * det.N_PIXELS[1] * det.TPC_BORDERS.shape[0] - 1
        for o in os_.values():
            assert o["radius"] == radius and o["unique_pix"].max() == pixel_max
            codes = set(np.unique(o["nrad"][o["neigh"] >= 0]).tolist())
            assert codes >= {1: {0, 1, 2}, 2: {0, 1, 2, 3, 4, 6}, 3: set(range(8)), 4: set(range(9))}[radius]
        st, out = _launch(seg, bid, resp)
    finally:
        H.load_cfg("module0")
    assert out["unique_pix"].max() == pixel_max
    _assert_launch(st, out, os_, f"{cfg} radius {radius}")
