"""GPU: pixel neighbourhoods of radius 2 to 4 -- ring codes 2-8, the -1 of |dx| + |dy| > 4 (pixels_from_track.py:246-269), unique
pixels whose every pair is unmapped (detsim.py:582-607), per-batch radii in one launch.

The stage kernels run on the reference's own outputs (tests/golden/pixels_wide_*.npz, oracle/gen_golden.py gen_pixels_wide);
the fused chain runs against the CPU oracle, which tests/test_oracle_golden.py pins to the same fixtures.  module0 with
TRAN_DIFF multiplied gives the chain its radius; every test asserts the radius the oracle derives.  Bars: integers exact, the
stage sums to rtol 1e-12 and 1e-12 of the largest sum (test_stage_api_chain_golden), the chain as in
test_fused_chain_vs_oracle_two_batches."""
import functools

import numpy as np
import pytest

import helpers as H
from larndsim_amd import batching, consts, detsim, pixels_from_track, synth
from larndsim_amd.chain import ChargeChain, expand_compact
from larndsim_amd.layout import segments_dtype
from oracle import oracle as O

pytestmark = pytest.mark.gpu


# ---- stage kernels against the reference's fixtures --------------------------------------------------------------------------
@pytest.mark.parametrize("radius", H.WIDE_RADII)
@pytest.mark.parametrize("cfg", H.WIDE_CFGS)
def test_stage_kernels_wide_golden(cfg, radius):
    """max_pixels, get_pixels, get_track_pixel_map2 and sum_pixel_signals through the reference-named wrappers on the fixture of
    one radius: clipped neighbourhoods, -1 gaps, a segment outside every TPC, every ring code the radius reaches, pixels
    without a slot, and the slots kept when the cap is too small."""
    H.load_cfg(cfg)
    g, signals, starts = H.wide_case(cfg, radius)
    r = H.quench_drift(O, g["segments_in"])      # oracle upstream: isolates the stages under test
    n = r.shape[0]
    mp = np.array([0])
    pixels_from_track.max_pixels[1, 128](r, mp)
    assert mp[0] == int(g["max_pixels"])
    active = np.full((n, mp[0]), -1, dtype=np.int32)
    neigh = np.full(g["neigh"].shape, -1, dtype=np.int32)
    nrad = np.full(g["neigh"].shape, -1, dtype=np.int32)
    nlist = np.zeros(n)
    pixels_from_track.get_pixels[1, 128](r, active, neigh, nrad, nlist, radius)
    assert np.array_equal(active, g["active"])
    assert np.array_equal(neigh, g["neigh"])
    assert np.array_equal(nrad, g["nrad"])
    assert np.array_equal(nlist, g["n_pixels_list"])
    upix = g["unique_pix"]
    U, NT = len(upix), len(consts.detector.TIME_TICKS)
    pim = g["pixel_index_map"].astype(np.int64)
    for tag, M in (("", consts.sim.MAX_TRACKS_PER_PIXEL), ("_low", int(g["max_tracks_low"]))):
        tpm = np.full((U, M), -1, dtype=np.int64)
        detsim.get_track_pixel_map2[1, 32](tpm, upix, neigh, nrad, int(nrad.max()) + 1)
        assert np.array_equal(tpm, g["track_pixel_map" + tag])
        ps = np.zeros((U, NT)); pts = np.zeros((U, NT, M)); ovf = np.zeros(U)
        detsim.sum_pixel_signals[1, 1](ps, signals, starts, pim, tpm, pts, ovf)
        top = H.sparse_field(g, "pixels_signals" + tag)[2].max()
        H.assert_sparse_close(ps, g, "pixels_signals" + tag, rtol=1e-12, atol=1e-12 * top)
        H.assert_sparse_close(pts, g, "pixels_tracks_signals" + tag, rtol=1e-12, atol=1e-12 * top)
        assert np.array_equal(ovf, g["overflow" + tag])


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_segment_counts_off_the_wave_and_workgroup(n, tail):
    """max_pixels, get_pixels (radius 3) and time_intervals on the first n segments of the fixture (repeated to reach n), n no
    multiple of the wave (64) or of the workgroup (128, 256): the wave reductions in front of their atomics, against the oracle
    on the same rows.  `tail`: the longest walk (segment 5) and the latest track sit on the last row alone, so that a reduction
    which drops the tail of a partial wave loses the maximum."""
    H.load_cfg("module0")
    g, _, _ = H.wide_case("module0", 3)
    base = H.quench_drift(O, g["segments_in"])
    rest = np.delete(base, 5) if tail else base
    r = np.concatenate([rest] * (-(-n // len(rest))))[:n].copy()
    if tail:
        r[-1] = base[5]
        r["t_end"][-1] = base["t_end"].max() + 7.0
    nmax = O.max_pixels(r)
    starts_ref, tmax_ref = O.time_intervals(r)
    if tail and n > 1:
        assert nmax > O.max_pixels(r[:-1]) and tmax_ref > O.time_intervals(r[:-1])[1]
    mp = np.array([0])
    pixels_from_track.max_pixels[1, 128](r, mp)
    assert mp[0] == nmax
    radius = 3
    P = (2 * radius + 1) * nmax + (1 + 2 * radius) * radius * 2
    ref = O.get_pixels(r, nmax, P, radius)
    active = np.full((n, nmax), -1, dtype=np.int32)
    neigh = np.full((n, P), -1, dtype=np.int32)
    nrad = np.full((n, P), -1, dtype=np.int32)
    nlist = np.zeros(n)
    pixels_from_track.get_pixels[1, 128](r, active, neigh, nrad, nlist, radius)
    for got, want in zip((active, neigh, nrad, nlist), ref):
        assert np.array_equal(got, want)
    starts = np.empty(n); tmax = np.array([0])
    detsim.time_intervals[1, 128](starts, tmax, r)
    assert np.array_equal(starts, starts_ref)
    assert tmax[0] == tmax_ref


# ---- the fused chain against the oracle -----------------------------------------------------------------------------------------
RADIUS2_SCALE = 6        # TRAN_DIFF x 6: radius 2 for the same segments


def _describe(o):
    tpm = o["tpm"]
    codes = sorted(set(np.unique(o["nrad"][o["neigh"] >= 0]).tolist()))
    return (f"radius {o['radius']}, P {o['P']}, {int((o['neigh'] >= 0).sum())} pairs, {len(tpm)} unique pixels, "
            f"{int(((tpm >= 0).sum(axis=1) == 0).sum())} without a slot, ring codes {codes}, {int((o['adc'] != 0).sum())} hits")


def _assert_rows(out, m, o, what):
    """the bars of test_fused_chain_vs_oracle_two_batches on the rows `m` of a download"""
    assert np.array_equal(out["unique_pix"][m], o["unique_pix"]), what
    assert np.array_equal(out["track_pixel_map"][m], o["tpm"]), what
    assert np.array_equal(out["adc_list"][m] != 0, o["adc"] != 0), what
    np.testing.assert_allclose(out["adc_list"][m], o["adc"], rtol=1e-5, err_msg=what)
    assert np.array_equal(out["adc_ticks_list"][m], o["ticks"]), what
    assert np.array_equal(out["adc_digit"][m], o["digit"]), what
    hit = o["adc"] != 0
    np.testing.assert_allclose(out["current_fractions"][m][hit], o["frac"][hit], rtol=1e-5, atol=1e-9, err_msg=what)


def _assert_far_slot_on_a_hit(o):
    """some hit pixel's map row holds a slot of ring code 2 or more that carries a non-zero fraction of a hit"""
    hit = o["adc"] != 0
    frac_on_hits = np.where(hit[:, :, None], np.abs(o["frac"]), 0.0).max(axis=1)      # [U][M]
    assert ((o["slot_code"] >= 2) & (frac_on_hits > 0)).any()


@functools.lru_cache(maxsize=None)
def _one_batch_case(scale):
    """the shared segments under TRAN_DIFF x scale and the oracle's chain on them: made once, read only"""
    H.load_module0_wide(scale)
    try:
        seg = H.radius3_segments()
        resp = synth.make_response("survey")
        o = H.oracle_chain(seg, resp)
    finally:
        H.load_cfg("module0")
    print(f"TRAN_DIFF x {scale}: " + _describe(o))
    return seg, resp, o


@pytest.mark.parametrize("scale,radius", [(RADIUS2_SCALE, 2), (H.RADIUS3_SCALE, 3)])
def test_fused_chain_radius_2_and_3_vs_oracle(scale, radius):
    """One batch at radius 2 (ring codes 0-4 and 6) and at radius 3 (0-7 and -1): pairs with code -1 stay in the pair list and
    make their pixel a row of every output, but take no slot; a pixel with nothing else has no track, no charge, no hit."""
    seg, resp, o = _one_batch_case(scale)
    assert o["radius"] == radius
    no_slot = (o["tpm"] >= 0).sum(axis=1) == 0
    codes = set(np.unique(o["nrad"][o["neigh"] >= 0]).tolist())
    _assert_far_slot_on_a_hit(o)
    if radius == 3:
        assert no_slot.sum() >= 10 and (o["adc"] != 0).sum() >= 5 and -1 in codes and max(codes) >= 5
        assert not o["adc"][no_slot].any()
    else:
        assert not no_slot.any() and -1 not in codes and max(codes) >= 3
    H.load_module0_wide(scale)
    try:
        ch = ChargeChain(resp)
        ch.upload(seg.copy(), np.zeros(len(seg), dtype=np.int32))
        ch.quench_drift()
        st = ch.run(0, len(seg), want_fractions=True)
        out = ch.download()
    finally:
        H.load_cfg("module0")
    assert st.max_neigh == o["P"] and st.n_unique == len(o["unique_pix"]) and st.n_pairs == int((o["neigh"] >= 0).sum())
    _assert_rows(out, slice(None), o, f"radius {radius}")
    assert (out["track_pixel_map"][no_slot] == -1).all() and not out["adc_list"][no_slot].any()
    assert not out["current_fractions"][no_slot].any()
    # the reference raises the overflow flag of a pixel for a pair it leaves unmapped, whatever the reason (detsim.py:526-527)
    assert st.n_overflow == int(o["overflow"].sum()) and (o["overflow"][no_slot] == 1).all()


def _near_and_far_batches():
    """6 + 6 segments moved along the drift axis: batch 0 within a centimetre of its anode, batch 1 in the last centimetre of
    the drift length (x, y and the directions stay)."""
    seg = synth.make_segments(12, seed=21, segs_per_event=6)
    batching.swap_coordinates(seg)
    B = np.asarray(consts.detector.TPC_BORDERS)
    bid = (seg["event_id"] - seg["event_id"][0]).astype(np.int32)
    for i in range(len(seg)):
        p = 0 if seg["z"][i] < 0 else 1
        anode, cathode = B[p, 2, 0], B[p, 2, 1]
        length, sign = abs(cathode - anode), np.sign(cathode - anode)
        d0 = 0.2 if bid[i] == 0 else length - 0.9
        for f in ("z_start", "z_end", "z"):
            seg[f][i] = anode + sign * (d0 + 0.6 * abs(seg[f][i] - anode) / length)
    return seg, bid


def test_two_batches_of_one_launch_with_radius_1_and_3():
    """Two batches of one launch, radius 1 and radius 3: they share the launch's P (that of the larger radius) but each keeps its
    own neighbourhoods -- every output per batch is the oracle's on that batch alone, with its own radius and P.  The far batch
    launched alone over its sub-range gives the same rows."""
    H.load_module0_wide(H.RADIUS3_SCALE)
    try:
        seg, bid = _near_and_far_batches()
        resp = synth.make_response("survey")
        os_ = [H.oracle_chain(seg[bid == b], resp) for b in (0, 1)]
        for b, o in enumerate(os_):
            print(f"batch {b}: " + _describe(o))
        assert [o["radius"] for o in os_] == [1, 3]
        assert os_[0]["P"] < os_[1]["P"]
        assert ((os_[1]["tpm"] >= 0).sum(axis=1) == 0).sum() >= 10 and all((o["adc"] != 0).sum() >= 5 for o in os_)
        ch = ChargeChain(resp)
        ch.upload(seg.copy(), bid)
        ch.quench_drift()
        st = ch.run(0, len(seg), want_fractions=True)
        out = ch.download()
        n0 = int((bid == 0).sum())
        st2 = ch.run(n0, len(seg), want_fractions=True)
        out2 = ch.download()
    finally:
        H.load_cfg("module0")
    assert st.n_batches == 2 and st.n_unique == sum(len(o["unique_pix"]) for o in os_)
    for b, o in enumerate(os_):
        _assert_rows(out, out["batch"] == b, o, f"batch {b}")
    assert st.n_overflow == sum(int(o["overflow"].sum()) for o in os_)
    # the far batch alone: P is now its own; the rows are the same
    assert st2.n_batches == 1 and st2.max_neigh == os_[1]["P"] and (out2["batch"] == 1).all()
    _assert_rows(out2, slice(None), os_[1], "far batch alone")
    m = out["batch"] == 1
    for k in ("unique_pix", "track_pixel_map", "adc_list", "adc_ticks_list", "adc_digit"):
        assert np.array_equal(out[k][m], out2[k]), k
    hit = out2["adc_list"] != 0
    assert np.array_equal(out["current_fractions"][m][hit], out2["current_fractions"][hit])


def _cluster_segments(n):
    """the cluster of test_more_than_max_tracks_per_pixel_vs_oracle over one pixel, the segments half as long (the oracle's
    currents for it then take well under a minute)"""
    det = consts.detector
    rng = np.random.default_rng(12)
    seg = np.zeros(n, dtype=segments_dtype)
    b = np.sort(det.TPC_BORDERS[0], axis=-1)
    px, py = 40, 100
    xc = b[0][0] + (px + 0.5) * det.PIXEL_PITCH
    yc = b[1][0] + (py + 0.5) * det.PIXEL_PITCH
    z0 = 0.5 * (b[2][0] + b[2][1])
    half = 0.35 * det.PIXEL_PITCH
    xs = xc + rng.uniform(-half, half, n); xe = xs + rng.uniform(0.01, 0.05, n) * rng.choice([-1, 1], n)
    ys = yc + rng.uniform(-half, half, n); ye = ys + rng.uniform(-0.05, 0.05, n)
    zs = z0 + rng.uniform(-1.0, 1.0, n); ze = zs + rng.uniform(-0.07, 0.07, n)
    seg["x_start"], seg["x_end"], seg["y_start"], seg["y_end"], seg["z_start"], seg["z_end"] = xs, xe, ys, ye, zs, ze
    for a in "xyz":
        seg[a] = 0.5 * (seg[a + "_start"] + seg[a + "_end"])
    seg["dx"] = np.sqrt((xe - xs) ** 2 + (ye - ys) ** 2 + (ze - zs) ** 2)
    seg["dEdx"] = 2.1
    seg["dE"] = seg["dEdx"] * seg["dx"]
    seg["segment_id"] = np.arange(n); seg["event_id"] = 0; seg["pdg_id"] = 13
    return seg


def test_more_pairs_than_slots_at_radius_2_vs_oracle():
    """52 short segments over one pixel at radius 2: pixels two pitches away collect 52 pairs of ring code 3 and more, keep the
    first MAX_TRACKS_PER_PIXEL = 50 in (ring code, segment) order and leave the rest out of the sum (detsim.py:510-524, 582-607)."""
    n = 52
    H.load_module0_wide(RADIUS2_SCALE)
    try:
        seg = _cluster_segments(n)
        resp = synth.make_response("survey")
        o = H.oracle_chain(seg, resp)
        print(_describe(o))
        ch = ChargeChain(resp)
        ch.upload(seg.copy(), np.zeros(n, dtype=np.int32))
        ch.quench_drift()
        st = ch.run(0, n, want_fractions=True)
        out = ch.download()
    finally:
        H.load_cfg("module0")
    assert o["radius"] == 2
    full = (o["tpm"] >= 0).sum(axis=1) == consts.sim.MAX_TRACKS_PER_PIXEL
    assert full.any() and o["overflow"].sum() > 0
    assert (o["slot_code"][full] >= 3).any(axis=1).any()      # a full pixel whose kept slots reach ring code 3 or more
    assert st.n_overflow > 0 and st.n_overflow == int(o["overflow"].sum())
    _assert_rows(out, slice(None), o, "radius 2, more pairs than slots")


def test_compact_download_of_the_radius_3_launch():
    """chain.expand_compact on the radius-3 launch gives the dense rows of its hit pixels (as
    test_compact_download_expands_to_the_dense_rows); no pixel without a slot is among them."""
    seg, resp, o = _one_batch_case(H.RADIUS3_SCALE)
    assert o["radius"] == 3
    H.load_module0_wide(H.RADIUS3_SCALE)
    try:
        ch = ChargeChain(resp)
        ch.upload(seg.copy(), np.zeros(len(seg), dtype=np.int32))
        ch.quench_drift()
        ch.run(0, len(seg), want_fractions=True)
        dense = ch.download()
        c = ch.download_compact()
        e = expand_compact(c)
    finally:
        H.load_cfg("module0")
    rows = e["row"]
    has_hit = dense["adc_list"][:, 0] != 0
    assert np.array_equal(np.flatnonzero(has_hit), rows) and np.array_equal(rows, np.flatnonzero((o["adc"] != 0).any(axis=1)))
    assert len(c["hit_rows"]) == int((dense["adc_list"] != 0).sum()) == ch.compact_hits()[1] == int((o["adc"] != 0).sum())
    for k in ("unique_pix", "batch", "adc_list", "adc_ticks_list", "adc_digit", "track_pixel_map"):
        assert np.array_equal(e[k], dense[k][rows]), k
    written = dense["adc_list"][rows] != 0
    assert np.array_equal(e["current_fractions"][written], dense["current_fractions"][rows][written])
    assert not e["current_fractions"][~written].any()
    no_slot = (o["tpm"] >= 0).sum(axis=1) == 0
    assert no_slot.sum() >= 10 and not no_slot[rows].any()
    assert np.array_equal(e["track_pixel_map"], o["tpm"][rows])
