"""
GPU: the self-trigger / ADC scan (adc_scan in csrc/kernels_fee.hip) against the reference's own get_adc_values.

Dense form: tests/golden/fee_scan_<variant>.npz (oracle/gen_golden.py gen_fee) holds hand-made waveforms, the constants of five
variants and what the reference's fee.get_adc_values / fee.digitize made of them -- failed triggers, hits past the end of the
waveform, the MAX_ADC_VALUES cap, true_q <= 0, no buffer rise time, interval / busy delay / reset longer than a 64-tick chunk,
thresholds <= 0 and, in `noisy`, the order in which the scan consumes its normals.  The generator proves which branch each row
reached; tests/test_oracle_golden.py pins the oracle to the same files.

Chain form: pixel_adc_body (windowed LDS image, start at the first written tick, stop after the last, one-wave and 256-thread
instantiations) against that oracle on a few hand-placed module0 segments.
"""
import numpy as np
import pytest

import helpers as H
from larndsim_amd import consts, fee, lib, rng as lrng
from larndsim_amd.chain import ChargeChain
from larndsim_amd.layout import segments_dtype
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FEE_SPAN = 512          # csrc/kernels_fee.hip


@pytest.mark.parametrize("variant", H.FEE_SCAN_VARIANTS)
def test_dense_scan_vs_reference(variant):
    """fee.get_adc_values / fee.digitize on the fixture's inputs: hit pattern, tick stamps and codes exact, charges to 1e-9
    (noisy: 1e-6 / 1e-2, the f32 normals' last bit), fractions at hit slots to 1e-9 / 1e-12, the generator's expect_* counts;
    noisy: the state table ends where the reference's stream ended."""
    try:
        g, tt = H.load_fee_scan_case(variant)
        noisy = variant == "noisy"
        U = len(g["thresholds"])
        A, M = consts.sim.MAX_ADC_VALUES, g["pixels_signals_tracks"].shape[2]
        assert g["adc_list"].shape == (U, A)
        adc = np.zeros((U, A)); ticks = np.zeros((U, A)); fr = np.zeros((U, A, M))
        states = lrng.create_xoroshiro128p_states(U, int(g["rng_seed"])) if noisy else None
        fee.get_adc_values[1, 128](g["pixels_signals"], g["pixels_signals_tracks"], tt, adc, ticks, 0, states, fr, g["thresholds"])
        digit = fee.digitize(adc)
        for u, name in enumerate(g["rows"]):
            print(variant, name, "hits", int((adc[u] != 0).sum()), "slots", int((ticks[u] != 0).sum()), "first stamp", ticks[u, 0],
                  "max |adc - ref|", float(np.abs(adc[u] - g["adc_list"][u]).max()))
        H.assert_fee_scan_matches(g, adc, ticks, fr, digit, noisy)
        if noisy:
            assert np.array_equal(states.copy_to_host().view(np.uint64).reshape(-1, 2), g["rng_states_after"]), \
                "draw counts differ from the reference's"
    finally:
        H.load_cfg("module0")


# ---- chain form ------------------------------------------------------------------------------------------------------------
def _segment(ix, iy, z0, length, dedx, t0=0.0, tilt=0.5):
    """one segment over pixel (ix, iy) of TPC 0, starting z0 cm from the anode, direction (tilt, tilt, sqrt(1 - 2 tilt^2))"""
    d = consts.detector
    B = np.asarray(d.TPC_BORDERS)
    s = np.zeros(1, dtype=segments_dtype)
    x, y, z = B[0, 0, 0] + (ix + 0.5) * d.PIXEL_PITCH, B[0, 1, 0] + (iy + 0.5) * d.PIXEL_PITCH, B[0, 2, 0] + z0
    dxy, dz = length * tilt, length * np.sqrt(1 - 2 * tilt * tilt)
    s["x_start"], s["y_start"], s["z_start"] = x, y, z
    s["x_end"], s["y_end"], s["z_end"] = x + dxy, y + dxy, z + dz
    for a in "xyz":
        s[a] = 0.5 * (s[a + "_start"].astype(np.float64) + s[a + "_end"])
    s["dx"], s["dEdx"], s["dE"] = length, dedx, dedx * length
    s["t0"] = s["t0_start"] = s["t0_end"] = t0
    return s


def _hand_segments():
    """[0, 1]   one pixel, 5 cm and 20 cm from the anode: drift times 94 us apart, more than FEE_SPAN ticks, a hit from each
       [2, 3]   29 cm from the anode with t0 such that the charge arrives in the last 2 us of the time axis: the integration runs
                past the end and the stamp exceeds time_ticks[-1]
       [4]      3 cm at 30 MeV/cm, 17 degrees off the drift axis: back-to-back hits on its pixels for 18 us (MAX_ADC_VALUES
                lowered to 3 cuts them)"""
    d = consts.detector
    drift29 = 29.0 / d.V_DRIFT
    seg = np.concatenate([_segment(20, 30, 5.0, 0.25, 6.0), _segment(20, 30, 20.0, 0.25, 6.0)] +
                         [_segment(40 + 10 * i, 60, 29.0, 0.25, 6.0, t0=t - drift29) for i, t in enumerate((200.2, 200.8))] +
                         [_segment(80, 90, 10.0, 3.0, 30.0, tilt=0.2)])
    seg["segment_id"] = np.arange(len(seg))
    return seg


_CACHE = {}


def _oracle_waveforms(seg, resp):
    """reference dataflow on the oracle up to the per-pixel waveforms (constants of the scan play no part): computed once"""
    if "w" not in _CACHE:
        ref = seg.copy()
        O.quench(ref, consts.physics.BIRKS)
        O.drift(ref)
        nmax = O.max_pixels(ref)
        r = int(np.ceil(ref["tran_diff"].max() * 5 / consts.detector.PIXEL_PITCH))
        _, neigh, nrad, _ = O.get_pixels(ref, nmax, (2 * r + 1) * nmax + (1 + 2 * r) * r * 2, r)
        upix = O.unique_pixels(neigh)
        starts, T = O.time_intervals(ref)
        sig = O.tracks_current(ref, neigh, T, resp)
        tpm = O.track_pixel_map(upix, neigh, nrad, int(nrad.max()) + 1, consts.sim.MAX_TRACKS_PER_PIXEL)
        ps, pts, _ = O.sum_pixel_signals(sig, starts, O.pixel_index_map(neigh, upix), tpm, len(upix))
        _CACHE["w"] = dict(upix=upix, tpm=tpm, ps=ps, pts=pts, t=ref["t"].astype(np.float64))
    return _CACHE["w"]


def _oracle_scan(w, thr):
    tt = np.linspace(0, consts.detector.TIME_INTERVAL[1], w["ps"].shape[1] + 1)
    adc, ticks, frac = O.get_adc_values(w["ps"], w["pts"], tt, thr)
    return dict(adc=adc, ticks=ticks, frac=frac, digit=O.digitize(adc), tt=tt)


def _assert_chain_equals(out, w, o, what):
    assert np.array_equal(out["unique_pix"], w["upix"]), what
    assert np.array_equal(out["track_pixel_map"], w["tpm"]), what
    assert np.array_equal(out["adc_list"] != 0, o["adc"] != 0), what
    assert np.array_equal(out["adc_ticks_list"], o["ticks"]), what
    assert np.array_equal(out["adc_digit"], o["digit"]), what
    H.assert_wave_close(out["adc_list"], o["adc"], what=what)          # 1e-5 |ref| + 1e-7 of the pixel's largest charge
    hit = o["adc"] != 0
    np.testing.assert_allclose(out["current_fractions"][hit], o["frac"][hit], rtol=1e-5, atol=1e-9, err_msg=what)


def _chain_run(seg, resp, one_class=False, table=None):
    ch = ChargeChain(resp)
    try:
        ch.upload(seg, np.zeros(len(seg), dtype=np.int32))
        ch.quench_drift()
        if one_class:
            lib.set_option("fee_one_class", 1, ch.ctx)
        if table is not None:
            ch.set_pixel_thresholds(*table)
        ch.run(0, len(seg), want_fractions=True)
        return ch.download(fractions=True)
    finally:
        lib.set_option("fee_one_class", 0, ch.ctx)
        lib.check(lib.load().ldsim_clear_pixel_tables(ch.ctx))


def test_chain_scan_vs_oracle_hand_placed():
    """ChargeChain against the oracle (pinned to the reference by the fee_scan fixtures) where pixel_adc_body differs from the
    dense kernel: a pixel whose two windows lie further apart than the one-wave form's LDS image, hits stamped past the end of
    the time axis, the MAX_ADC_VALUES cap and a per-pixel threshold <= 0 under the windowed image."""
    try:
        H.load_cfg("module0")
        d = consts.detector
        seg = _hand_segments()
        resp = H.response_for("survey")
        w = _oracle_waveforms(seg, resp)
        upix, tpm = w["upix"], w["tpm"]
        thr0 = np.full(len(upix), d.DISCRIMINATION_THRESHOLD * 1.0)
        o = _oracle_scan(w, thr0)
        # -- the cases are there, by the oracle's own output
        wide = [u for u in np.flatnonzero((tpm >= 0).sum(axis=1) > 1)
                if np.ptp(w["t"][tpm[u][tpm[u] >= 0]]) / d.TIME_SAMPLING > FEE_SPAN and (o["adc"][u] != 0).sum() >= 2]
        assert wide, "no pixel with two hits from windows further apart than FEE_SPAN ticks"
        for u in wide:
            stamps = o["ticks"][u][o["adc"][u] != 0]
            assert np.ptp(stamps) / d.TIME_SAMPLING > FEE_SPAN, "the hits are not one from each segment"
        assert (o["ticks"] > o["tt"][-1]).any(), "no hit stamped past time_ticks[-1]"
        # -- default constants: both instantiations against the oracle, and against each other bit by bit
        out = _chain_run(seg, resp)
        _assert_chain_equals(out, w, o, "two classes")
        one = _chain_run(seg, resp, one_class=True)
        for k in out:
            assert np.array_equal(out[k], one[k]), ("fee_one_class changed " + k)
        # -- a threshold table: one hit pixel at a threshold <= 0, one raised.  The pixel at -100 triggers from tick 0 on, long
        # before its window, and has spent its MAX_ADC_VALUES slots on empty hits when its charge arrives (a pixel whose charge
        # arrives earlier would integrate the response's leading tail, f32 denormals, where `adc != 0` is no stable property;
        # the fee_scan rows h_negq / j_thr_zero integrate real charge under such thresholds)
        hit_rows = np.flatnonzero((o["adc"] != 0).any(axis=1))
        late = hit_rows[np.argmax(o["ticks"][hit_rows, 0])]
        other = hit_rows[np.argmax(np.abs(o["adc"][hit_rows]).sum(axis=1))]
        assert late != other
        n_ids = int(d.N_PIXELS[0] * d.N_PIXELS[1] * np.asarray(d.TPC_BORDERS).shape[0])
        keys = np.array([upix[late], upix[other]], dtype=np.int32)
        vals = np.array([-100.0, 2.0 * d.DISCRIMINATION_THRESHOLD])
        thr_of_pixel = np.full(n_ids, 1.1 * d.DISCRIMINATION_THRESHOLD)
        thr_of_pixel[keys] = vals
        ot = _oracle_scan(w, np.ascontiguousarray(thr_of_pixel[upix]))
        assert (ot["ticks"][late] != 0).sum() == consts.sim.MAX_ADC_VALUES and not (ot["adc"][late] != 0).any()
        assert ot["ticks"][late, 0] < 0 and not np.array_equal(ot["ticks"][other], o["ticks"][other])
        outt = _chain_run(seg, resp, table=(keys, vals, 1.1 * d.DISCRIMINATION_THRESHOLD))
        _assert_chain_equals(outt, w, ot, "threshold table")
        # -- MAX_ADC_VALUES = 3
        consts.sim.MAX_ADC_VALUES = 3
        oc = _oracle_scan(w, thr0)
        assert ((oc["adc"] != 0).sum(axis=1) == 3).any() and ((o["adc"] != 0).sum(axis=1) > 3).any()
        outc = _chain_run(seg, resp)
        assert outc["adc_list"].shape[1] == 3
        _assert_chain_equals(outc, w, oc, "MAX_ADC_VALUES = 3")
    finally:
        H.load_cfg("module0")
