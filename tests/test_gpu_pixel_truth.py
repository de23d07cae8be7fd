"""GPU: pixel charge truth (ChargeChain.pixel_truth, ldsim_chain_pixel_truth, simulate_pixels.py --pixel_truth).

The reference for the waveforms is the project's own: the oracle's per-(track, pixel) currents and per-pixel sums, reduced in
numpy by the restatement of the definition (larndsim_amd/pixel_truth.py).  The tolerance is the project's per-tick bar
(helpers.assert_wave_close: 1e-5 |ref_t| + 1e-7 peak), summed over the ticks and times dt -- no new number."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import helpers as H
from larndsim_amd import batching, consts, detsim, lib, synth
from larndsim_amd import pixel_truth as PT
from larndsim_amd.chain import ChargeChain
from larndsim_amd.layout import segments_dtype
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
SIZES = [(0, 90), (1, 47), (-1, 30), (2, 133)]          # (batch id, segments): three unequal batches and a skipped run
TABLE = [(0, 0, 0, 90), (0, 1, 0, 47), (1, 0, 0, 133)]   # their identities (event, TPC group, sub-batch, n) for the keyed streams


def _segments(cfg="module0", n=300, seed=31):
    H.load_cfg(cfg)
    spill = bool(consts.sim.IS_SPILL_SIM)
    seg = synth.make_segments(n, seed=seed, segs_per_event=n, spill=spill)
    if spill:                            # the driver removes the spill offset (cli/simulate_pixels.py:574-582)
        loc = seg["event_id"] % consts.sim.MAX_EVENTS_PER_FILE
        for f in ("t0", "t0_start", "t0_end"):
            seg[f] = seg[f] - loc * consts.sim.SPILL_PERIOD
    batching.swap_coordinates(seg)
    return seg


def _reference(seg, resp):
    """The five values of every unique pixel of one batch from the oracle's currents, with the summed per-tick tolerances"""
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
    M = consts.sim.MAX_TRACKS_PER_PIXEL
    tpm = O.track_pixel_map(upix, neigh, nrad, int(nrad.max()) + 1, M)
    ps, _, ovf = O.sum_pixel_signals(sig, starts, pim, tpm, len(upix), want_tracks=False)
    dt, NT, U = det.TIME_SAMPLING, ps.shape[1], len(upix)
    tick0 = np.rint(starts / dt).astype(np.int64)                  # detsim.py:506
    out = dict(upix=upix, tpm=tpm, ovf=ovf, q_track=np.zeros((U, M)), tol_track=np.zeros((U, M)), q_induced=np.zeros(U),
               q_abs=np.zeros(U), abs_sum=np.zeros(U), n_samples=np.zeros(U, dtype=np.int64))
    for u in range(U):
        ks = tpm[u][tpm[u] >= 0]
        rows = np.stack([sig[t, np.flatnonzero(pim[t] == u)[0]] for t in ks]) if len(ks) else np.zeros((0, T), np.float32)
        v = PT.restate(rows, tick0[ks], [(0, T)] * len(ks), dt, NT)
        out["q_track"][u, :len(ks)] = v["q_track"]
        out["q_induced"][u], out["q_abs"][u] = v["q_induced"], v["q_abs"]
        for k, t in enumerate(ks):
            lo, hi = max(int(tick0[t]), 0), min(int(tick0[t]) + T, NT)
            part = np.abs(rows[k, lo - int(tick0[t]):max(hi, lo) - int(tick0[t])].astype(np.float64))
            out["tol_track"][u, k] = dt * (1e-5 * part.sum() + 1e-7 * np.abs(rows[k]).max() * len(part))
            out["abs_sum"][u] += part.sum()
            out["n_samples"][u] += len(part)
    # the restated sums are the oracle's own pixel sums (its atomics add the same terms in another order)
    assert np.allclose(out["q_induced"], dt * ps.sum(axis=1), rtol=0, atol=1e-9 * dt * max(np.abs(ps).sum(axis=1).max(), 1e-300))
    out["tol_pix"] = dt * (1e-5 * np.abs(ps).sum(axis=1) + 1e-7 * np.abs(ps).max(axis=1) * NT)
    return out


@functools.lru_cache(maxsize=None)
def _module0_case():
    """300 segments in three unequal batches and a skipped run, the response, the per-batch references: made once, read only"""
    seg = _segments()
    bid = np.concatenate([np.full(n, b) for b, n in SIZES]).astype(np.int32)
    resp = synth.make_response("survey")
    refs = {b: _reference(seg[bid == b], resp) for b, _ in SIZES if b >= 0}
    for a in [seg, bid, resp] + [v for r in refs.values() for v in r.values()]:
        a.setflags(write=False)
    return seg, bid, resp, refs


def _launch(ch, seg, bid, b0=0, e0=None, keyed=None, min_abs=0.0):
    ch.upload(seg.copy(), bid)
    if keyed is not None:
        ch.set_batch_keys(TABLE, -1)
    ch.quench_drift()
    st = ch.run(b0, len(seg) if e0 is None else e0, want_fractions=False)
    out = ch.download()
    dense = ch.pixel_truth(dense=True)
    compact = ch.pixel_truth(min_abs)
    return st, out, dense, compact


def _assert_matches_reference(out, dense, refs, batches, what):
    for b in batches:
        o, m = refs[b], out["batch"] == b
        assert np.array_equal(out["unique_pix"][m], o["upix"]), what
        assert np.array_equal(out["track_pixel_map"][m], o["tpm"]), what
        for name, tol in (("q_induced", "tol_pix"), ("q_abs", "tol_pix")):
            err = np.abs(dense[name][m] - o[name])
            print(f"{what} batch {b} {name}: worst error / tolerance {np.max(err[o[tol] > 0] / o[tol][o[tol] > 0]):.3g}")
            assert (err <= o[tol]).all(), (what, b, name, float(np.max(err / o[tol])))
        err = np.abs(dense["q_track"][m] - o["q_track"])
        filled = o["tpm"] >= 0
        lit = filled & (o["tol_track"] > 0)
        print(f"{what} batch {b} q_track: worst error / tolerance {np.max(err[lit] / o['tol_track'][lit]):.3g}")
        assert (err[filled] <= o["tol_track"][filled]).all(), (what, b)
        assert (dense["q_track"][m][~filled] == 0).all(), what      # empty slots hold exactly 0


def _assert_compact_is_the_dense_selection(out, dense, compact, min_abs):
    """the compact form against numpy on the dense arrays and the downloaded results"""
    px, tr = compact["pixels"], compact["tracks"]
    n_hits, q_hits = PT.hits_of(out["adc_list"])
    keep = (n_hits > 0) | (dense["q_abs"] >= min_abs)
    rows = np.flatnonzero(keep)
    assert np.array_equal(px["row"], rows)                          # (the kept rows, in row order)
    assert np.array_equal(px["pixel_id"], out["unique_pix"][rows]) and np.array_equal(px["batch"], out["batch"][rows])
    assert np.array_equal(px["n_hits"], n_hits[rows]) and np.array_equal(px["q_hits"], q_hits[rows])
    assert np.array_equal(px["q_induced"], dense["q_induced"][rows]) and np.array_equal(px["q_abs"], dense["q_abs"][rows])
    filled = out["track_pixel_map"][rows] >= 0
    assert np.array_equal(px["n_tracks"], filled.sum(axis=1))
    assert (filled == (np.arange(filled.shape[1])[None, :] < px["n_tracks"][:, None])).all()      # filled from slot 0 on
    assert len(tr) == int(filled.sum())
    assert np.array_equal(tr["segment"], out["track_pixel_map"][rows][filled])      # pixel after pixel, slot 0 up
    assert np.array_equal(tr["q"], dense["q_track"][rows][filled])
    return rows


def test_against_the_oracle_whole_and_sub_range():
    """1. ~300 synthetic segments, three unequal batches and a run with batch id < 0, launched whole and as a sub-range"""
    seg, bid, resp, refs = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    st, out, dense, compact = _launch(ch, seg, bid)
    assert sorted(set(out["batch"].tolist())) == [0, 1, 2] and st.n_unique == sum(len(r["upix"]) for r in refs.values())
    _assert_matches_reference(out, dense, refs, (0, 1, 2), "whole")
    rows = _assert_compact_is_the_dense_selection(out, dense, compact, 0.0)
    assert len(rows) == st.n_unique                                  # min_abs_charge 0 keeps every unique pixel
    # the samples the pass sums: the written windows, at most the whole rows the reference sums
    assert 0 < ch.pixel_truth_row_samples() <= sum(int(r["n_samples"].sum()) for r in refs.values())
    assert (compact["pixels"]["n_hits"] > 0).any() and (compact["pixels"]["n_hits"] == 0).any()
    # the sub-range: batches 1 and 2 only (seg_begin > 0); their rows are the whole launch's
    b0 = SIZES[0][1]
    st2, out2, dense2, compact2 = _launch(ch, seg, bid, b0=b0)
    assert sorted(set(out2["batch"].tolist())) == [1, 2]
    _assert_matches_reference(out2, dense2, refs, (1, 2), "sub-range")
    _assert_compact_is_the_dense_selection(out2, dense2, compact2, 0.0)
    m = out["batch"] >= 1
    for k in dense:
        assert np.array_equal(dense[k][m], dense2[k]), k


def test_both_header_layouts_and_noise_give_the_same_bits():
    """2. the set-up record as two lists (default), as headers [U] (fee_one_class), and under keyed FEE noise (one class, keyed
    instance): q_induced, q_abs and q_track bit for bit; noise only moves n_hits and q_hits"""
    seg, bid, resp, refs = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    st, out, dense, compact = _launch(ch, seg, bid)
    try:
        lib.set_option("fee_one_class", 1)
        st1, out1, dense1, compact1 = _launch(ch, seg, bid)
    finally:
        lib.set_option("fee_one_class", 0)
    for k in dense:
        assert np.array_equal(dense[k], dense1[k]), k
    for k in ("pixels", "tracks"):
        assert np.array_equal(compact[k], compact1[k]), k
    H.load_cfg("module0", noise_zero=False)
    assert consts.detector.RESET_NOISE_CHARGE > 0 and consts.detector.UNCORRELATED_NOISE_CHARGE > 0
    try:
        noisy = ChargeChain(resp)
        noisy.seed_keyed(20260131)
        stn, outn, densen, compactn = _launch(noisy, seg, bid, keyed=True)
        for k in dense:
            assert np.array_equal(dense[k], densen[k]), k
        _assert_compact_is_the_dense_selection(outn, densen, compactn, 0.0)
        assert not np.array_equal(compactn["pixels"]["q_hits"], compact["pixels"]["q_hits"])
        for k in ("row", "pixel_id", "batch", "n_tracks", "q_induced", "q_abs"):
            assert np.array_equal(compactn["pixels"][k], compact["pixels"][k]), k
        assert np.array_equal(compactn["tracks"], compact["tracks"])
    finally:
        H.load_cfg("module0")
        ChargeChain(resp).seed_rng(1, n_states=64)                  # (the ctx is process-wide: back to table mode)


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


def test_more_pairs_than_slots_on_a_pixel():
    """3. MAX_TRACKS_PER_PIXEL = 4 and ten parallel segments over one pixel column: q_track has the M slots the FEE sum has,
    q_induced is their sum to f64 rounding, and the launch counts the overflow"""
    H.load_cfg("module0")
    consts.sim.MAX_TRACKS_PER_PIXEL = M = 4
    try:
        seg = _column_segments(10)
        resp = synth.make_response("survey")
        ref = _reference(seg, resp)
        ch = ChargeChain(resp)
        ch.upload(seg.copy(), np.zeros(len(seg), dtype=np.int32))
        ch.quench_drift()
        st = ch.run()
        out, dense, compact = ch.download(), ch.pixel_truth(dense=True), ch.pixel_truth()
        assert st.n_overflow > 0 and ref["ovf"].any()
        assert dense["q_track"].shape == (st.n_unique, M)
        full = (ref["tpm"] >= 0).all(axis=1)
        assert full.any() and np.array_equal(out["track_pixel_map"], ref["tpm"])
        _assert_matches_reference(out, dense, {0: ref}, (0,), "M = 4")
        _assert_compact_is_the_dense_selection(out, dense, compact, 0.0)
        assert (compact["pixels"]["n_tracks"][full] == M).all()
        dt = consts.detector.TIME_SAMPLING
        bound = ref["n_samples"] * 2.0 ** -52 * dt * ref["abs_sum"]
        err = np.abs(dense["q_induced"] - dense["q_track"].sum(axis=1))
        print("q_induced - sum of its slots, worst error / bound:", float(np.max(err[bound > 0] / bound[bound > 0])))
        assert (err <= bound).all()
    finally:
        H.load_cfg("module0")


def test_two_response_samples_per_tick():
    """4. TIME_SAMPLING / RESPONSE_SAMPLING = 2 (the ndlar snapshot), about 100 segments (80) in one batch"""
    seg = _segments("ndlar", n=80, seed=8)
    det = consts.detector
    assert int(round(det.TIME_SAMPLING / det.RESPONSE_SAMPLING)) == 2
    try:
        resp = H.response_for("golden")
        ref = _reference(seg, resp)
        ch = ChargeChain(resp)
        ch.upload(seg.copy(), np.zeros(len(seg), dtype=np.int32))
        ch.quench_drift()
        st = ch.run()
        out, dense, compact = ch.download(), ch.pixel_truth(dense=True), ch.pixel_truth()
        assert st.n_unique == len(ref["upix"]) > 50
        _assert_matches_reference(out, dense, {0: ref}, (0,), "ndlar")
        _assert_compact_is_the_dense_selection(out, dense, compact, 0.0)
    finally:
        H.load_cfg("module0")


def test_selection_on_the_device():
    """5. min_abs_charge 0 keeps all rows; a threshold between two observed q_abs values keeps what numpy keeps, plus every
    pixel with hits; above every q_abs with no hits: sizes (0, 0) and rc 0"""
    import ctypes as C
    seg, bid, resp, refs = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    st, out, dense, compact = _launch(ch, seg, bid)
    assert len(compact["pixels"]) == st.n_unique
    n_hits, _ = PT.hits_of(out["adc_list"])
    quiet = np.sort(dense["q_abs"][n_hits == 0])
    assert len(quiet) > 10 and quiet[len(quiet) // 2] > quiet[len(quiet) // 2 - 1]
    thr = 0.5 * (quiet[len(quiet) // 2 - 1] + quiet[len(quiet) // 2])      # between two observed values
    sizes = (C.c_int64 * 2)()
    lib.check(lib.load().ldsim_chain_pixel_truth(ch.ctx, C.c_double(thr), sizes))
    part = ch.pixel_truth(thr)
    rows = _assert_compact_is_the_dense_selection(out, dense, part, thr)
    assert (sizes[0], sizes[1]) == (len(rows), int((out["track_pixel_map"][rows] >= 0).sum()))
    assert (n_hits > 0).sum() < len(rows) < st.n_unique                # some hit-less pixels kept, some dropped
    assert set(np.flatnonzero(n_hits > 0)) <= set(rows.tolist())
    begin, count = PT.tracks_of(part["pixels"], part["tracks"])         # contiguous per pixel
    assert np.array_equal(begin + count, np.r_[begin[1:], len(part["tracks"])])
    # no hits at all: a discrimination threshold no pixel reaches
    consts.detector.DISCRIMINATION_THRESHOLD = 1e12
    try:
        deaf = ChargeChain(resp)
        st0, out0, dense0, all0 = _launch(deaf, seg, bid)
        assert (out0["adc_list"] == 0).all() and len(all0["pixels"]) == st0.n_unique
        for k in dense:
            assert np.array_equal(dense0[k], dense[k]), k               # (the threshold does not enter the truth)
        lib.check(lib.load().ldsim_chain_pixel_truth(deaf.ctx, C.c_double(2 * dense0["q_abs"].max()), sizes))
        assert (sizes[0], sizes[1]) == (0, 0)
        none = deaf.pixel_truth(2 * dense0["q_abs"].max())
        assert len(none["pixels"]) == 0 and len(none["tracks"]) == 0
    finally:
        H.load_cfg("module0")


def test_validity_of_the_resident_launch():
    """6. reset, upload, quench_drift and a host-array tracks_current call each make pixel_truth refuse on the host
    (LDSIM_ESTATE, naming the call); a fresh run makes it work again with the same values; U == 0 gives empty arrays"""
    seg, bid, resp, refs = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    st, out, base, compact = _launch(ch, seg, bid)

    def refused(word):
        for kw in (dict(), dict(dense=True)):
            with pytest.raises(lib.LdsimError, match=rf"ldsim error -4: .*{word}"):
                ch.pixel_truth(**kw)

    def rerun():
        ch.run()
        again = ch.pixel_truth(dense=True)
        for k in base:
            assert np.array_equal(again[k], base[k]), k
        assert np.array_equal(ch.pixel_truth()["pixels"], compact["pixels"])

    ch.reset()
    refused("ldsim_segments_reset")
    with pytest.raises(lib.LdsimError, match="ldsim error -4: .*ldsim_segments_reset"):
        ch.pixel_truth_row_samples()
    ch.quench_drift()
    refused("ldsim_dev_quench_drift")
    rerun()
    ch.upload(seg.copy(), bid)
    refused("ldsim_segments_upload")
    ch.quench_drift()
    rerun()
    # a host-array stage call takes the launch's buffers (and the segment store) over
    few = seg[:4].copy()
    sig = np.zeros((4, 3, 64), dtype=np.float32)
    detsim.tracks_current[1, 1](sig, np.full((4, 3), -1, dtype=np.int32), few, resp)
    refused("stage call")
    ch.upload(seg.copy(), bid)
    ch.quench_drift()
    rerun()
    # a launch that failed leaves nothing to read either
    with pytest.raises(lib.LdsimError, match="outside the resident store"):
        ch.run(0, len(seg) + 1)
    rerun()
    # nothing to simulate: every batch id negative
    ch.upload(seg.copy(), np.full(len(seg), -1, dtype=np.int32))
    ch.quench_drift()
    st0 = ch.run()
    assert st0.n_unique == 0
    empty, dense0 = ch.pixel_truth(), ch.pixel_truth(dense=True)
    assert len(empty["pixels"]) == 0 and len(empty["tracks"]) == 0
    assert dense0["q_induced"].shape == (0,) and dense0["q_track"].shape == (0, consts.sim.MAX_TRACKS_PER_PIXEL)
    # before any launch of a context's life the call refuses as well: checked through a download without a pass
    ch.upload(seg.copy(), bid)
    ch.quench_drift()
    ch.run()
    import ctypes as C
    rc = lib.load().ldsim_chain_pixel_truth_dense_download(ch.ctx, C.c_int64(int(ch.stats.n_unique)), None, None, None)
    assert rc == -4 and b"has not run for the last chain launch" in lib.load().ldsim_last_error()


def _uniform_maps(shape=(3, 4, 5), **const):
    maps = {}
    for t in range(len(consts.detector.TPC_BORDERS)):
        b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[t]
        lo, hi = b.min(axis=1), b.max(axis=1)
        m = {"origin": lo - 1, "spacing": (hi - lo + 2) / (np.array(shape) - 1)}
        m.update({k: np.full(shape, float(v)) for k, v in const.items()})
        maps[t] = m
    return maps


def test_with_the_opt_in_physics():
    """7. a uniform field map leaves every bit; with keyed charge statistics the charge a segment puts on its collecting pixels
    changes, and is the same whether the batches run in one launch or one launch each"""
    seg, bid, resp, refs = _module0_case()
    H.load_cfg("module0")
    ch = ChargeChain(resp)
    st, out, dense, compact = _launch(ch, seg, bid)
    try:
        ch.set_field_map(_uniform_maps(E=consts.detector.E_FIELD, dx=0, dy=0, dz=0))
        stm, outm, densem, compactm = _launch(ch, seg, bid)
    finally:
        ch.clear_field_map()
    for k in dense:
        assert np.array_equal(dense[k], densem[k]), k
    for k in ("pixels", "tracks"):
        assert np.array_equal(compact[k], compactm[k]), k

    def charge_per_segment(c):
        """sum of q over the track entries of every (batch, segment)"""
        begin, count = PT.tracks_of(c["pixels"], c["tracks"])
        b = np.repeat(c["pixels"]["batch"].astype(np.int64), count)
        key = b * 1000 + c["tracks"]["segment"]
        order = np.argsort(key, kind="stable")
        uk, first = np.unique(key[order], return_index=True)
        return uk, np.add.reduceat(c["tracks"]["q"][order], first)

    try:
        ch.seed_keyed(77)
        ch.set_charge_statistics(True)
        ch.upload(seg.copy(), bid)
        ch.set_batch_keys(TABLE, -1)
        ch.quench_drift()
        ch.run()
        whole = ch.pixel_truth()
        edges = np.r_[0, np.cumsum([n for _, n in SIZES])]
        parts = []
        for (b, n), lo, hi in zip(SIZES, edges[:-1], edges[1:]):
            if b >= 0:
                ch.run(int(lo), int(hi))
                parts.append(ch.pixel_truth())
    finally:
        ch.set_charge_statistics(False)
        ch.seed_rng(1, n_states=64)
    k0, q0 = charge_per_segment(compact)
    k1, q1 = charge_per_segment(whole)
    assert np.array_equal(k0, k1) and not np.array_equal(q0, q1)
    assert np.abs(q1.sum() / q0.sum() - 1) < 0.05                     # (counted charge fluctuates about the mean-value charge)
    joined = np.concatenate([p["pixels"] for p in parts])
    for k in ("pixel_id", "batch", "n_hits", "n_tracks", "q_hits", "q_induced", "q_abs"):      # (row counts from each launch's 0)
        assert np.array_equal(joined[k], whole["pixels"][k]), k
    assert np.array_equal(np.concatenate([p["tracks"] for p in parts]), whole["tracks"])


def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_pixel_truth_gpu", CLI)
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
    """8. --pixel_truth: both datasets, equal to a ChargeChain run by hand on the same batches, track_begin / track_count tiling
    pixel_truth_tracks, the same at --chunk_segments 40 and 100000, and nothing else of the file moved (.npz stream: the
    interpreter of the GPU tests has no h5py)"""
    cli = _cli()
    H.load_cfg("module0")
    seg = synth.make_segments(200, seed=21, segs_per_event=40)          # 5 events
    seg = seg[np.random.default_rng(2).permutation(len(seg))]
    np.save(tmp_path / "in.npy", seg)
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    common = dict(input_filename=str(tmp_path / "in.npy"), config="module0", rand_seed=7, rng="keyed", light_simulated=False,
                  response_file=str(tmp_path / "resp.npy"))

    def run(name, **kw):
        cli.run_simulation(output_filename=str(tmp_path / name), **common, **kw)
        with np.load(tmp_path / name) as f:
            return {k: f[k] for k in f.files}, capsys.readouterr().out

    a, log = run("t40.npz", pixel_truth=True, chunk_segments=40)
    assert "Pixel charge truth: on (--pixel_truth, --pixel_truth_min_charge 0 e)" in log
    b, _ = run("t1e5.npz", pixel_truth=True, chunk_segments=100000)
    plain, log = run("plain.npz", chunk_segments=40)
    assert "Pixel charge truth" not in log
    cut, _ = run("cut.npz", pixel_truth=True, pixel_truth_min_charge=500.0, chunk_segments=40)
    assert set(a) == set(b) == set(plain) | {"pixel_truth", "pixel_truth_tracks"}
    for k in a:
        _assert_same_bytes(a[k], b[k], k)
    for k in plain:
        _assert_same_bytes(a[k], plain[k], k)
    px, tr = a["pixel_truth"], a["pixel_truth_tracks"]
    assert px.dtype == PT.FILE_PIXEL and tr.dtype == PT.FILE_TRACK and len(px) > 100 and (px["n_hits"] > 0).any()
    assert np.array_equal(px["track_begin"], np.cumsum(px["track_count"]) - px["track_count"])       # tiles the entries
    assert int(px["track_count"].sum()) == len(tr)
    keep = (px["n_hits"] > 0) | (px["q_abs"] >= 500.0)
    assert 0 < keep.sum() < len(px)
    for k in ("event_id", "pixel_id", "n_hits", "q_hits", "q_induced", "q_abs", "track_count"):
        assert np.array_equal(cut["pixel_truth"][k], px[k][keep]), k
    assert np.array_equal(cut["pixel_truth_tracks"], tr[np.repeat(keep, px["track_count"])])
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
        hand = ch.pixel_truth()
    finally:
        lib.set_option("numba_f32", 0)
        ChargeChain(synth.make_response("survey")).seed_rng(1, n_states=64)
        H.load_cfg("module0")
    hp, ht = hand["pixels"], hand["tracks"]
    assert np.array_equal(px["event_id"], np.array([t[0] for t in table])[hp["batch"]])
    for k in ("pixel_id", "n_hits", "q_hits", "q_induced", "q_abs"):
        assert np.array_equal(px[k], hp[k]), k
    assert np.array_equal(px["track_count"], hp["n_tracks"]) and np.array_equal(tr["q"], ht["q"])
    first = np.searchsorted(bid[:int((bid >= 0).sum())], np.arange(len(table)), side="left")
    seg_idx = np.repeat(first[hp["batch"]], hp["n_tracks"]) + ht["segment"]
    assert np.array_equal(tr["segment_id"], tracks["segment_id"][seg_idx].astype(np.int64))
    # ... and through the file's own segments: every entry names a segment of its pixel's event
    fseg = a["segments"]
    by_id = np.argsort(fseg["segment_id"], kind="stable")
    pos = by_id[np.searchsorted(fseg["segment_id"][by_id], tr["segment_id"])]
    assert np.array_equal(fseg["segment_id"][pos], tr["segment_id"])
    assert np.array_equal(fseg["event_id"][pos], np.repeat(px["event_id"], px["track_count"]))


def test_radius_3_launch_with_pixels_without_a_slot():
    """A launch at neighbour radius 3 (module0, TRAN_DIFF x 16): pairs farther than |dx| + |dy| = 4 from their segment carry ring
    code -1, make their pixel a row of the results and take no slot (pixels_from_track.py:251-252, detsim.py:582).  Such a pixel
    has no track and exactly no charge; every other row against the oracle as in test 1."""
    H.load_module0_wide(H.RADIUS3_SCALE)
    try:
        seg, resp = H.radius3_segments(), synth.make_response("survey")
        assert H.oracle_radius(seg) == 3
        ref = _reference(seg, resp)
        ch = ChargeChain(resp)
        st, out, dense, compact = _launch(ch, seg, np.zeros(len(seg), dtype=np.int32))
    finally:
        H.load_cfg("module0")
    no_slot = (ref["tpm"] >= 0).sum(axis=1) == 0
    assert no_slot.sum() >= 10 and (ref["ovf"][no_slot] == 1).all() and st.n_unique == len(ref["upix"])
    _assert_matches_reference(out, dense, {0: ref}, (0,), "radius 3")
    assert (out["track_pixel_map"][no_slot] == -1).all() and not out["adc_list"][no_slot].any()
    assert (dense["q_induced"][no_slot] == 0).all() and (dense["q_abs"][no_slot] == 0).all()
    assert (dense["q_track"][no_slot] == 0).all()
    rows = _assert_compact_is_the_dense_selection(out, dense, compact, 0.0)
    assert len(rows) == st.n_unique and (compact["pixels"]["n_tracks"][no_slot] == 0).all()
