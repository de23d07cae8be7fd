"""
CPU: pin the oracle (oracle/ldsim_oracle.c) against golden vectors produced by the reference's own
source (oracle/gen_golden.py).  Integer outputs bit-exact; f64 outputs to 1e-13 relative (same libm
functions, same operation order).
"""
import os

import numpy as np
import pytest

import helpers as H
from larndsim_amd import consts
from oracle import oracle as O

CFGS = ["module0", "2x2_no_modvar", "ndlar"]


@pytest.mark.parametrize("cfg", CFGS)
def test_quench_drift(cfg):
    H.load_cfg(cfg)
    g = H.gold(f"qd_{cfg}.npz")
    seg = g["segments_in"]
    for mode, name in ((2, "birks"), (1, "box")):
        r = H.to_ref(seg)
        O.quench(r, mode)
        assert np.array_equal(r["n_electrons"], g[f"{name}_n_electrons"])
        np.testing.assert_allclose(H.f4(r["n_photons"]), g[f"{name}_n_photons"], rtol=0, atol=0)
        if name == "birks":
            H.round_f4(r, ["n_photons"])
            O.drift(r)
            assert np.array_equal(r["pixel_plane"], g["drift_pixel_plane"])
            assert np.array_equal(r["n_electrons"], g["drift_n_electrons"])
            for f in ("long_diff", "tran_diff", "t", "t_start", "t_end"):
                np.testing.assert_allclose(r[f], g["drift_" + f], rtol=1e-15, atol=0, err_msg=f)
    assert (g["drift_pixel_plane"] == consts.detector.DEFAULT_PLANE_INDEX).any() or cfg != "module0"


@pytest.mark.parametrize("cfg", CFGS)
def test_pixels_time_intervals(cfg):
    H.load_cfg(cfg)
    g = H.gold(f"pixels_{cfg}.npz")
    r = H.quench_drift(O, g["segments_in"])
    assert O.max_pixels(r) == int(g["max_pixels"])
    radius = int(g["max_radius"])
    active, neigh, nrad, nlist = O.get_pixels(r, int(g["max_pixels"]), g["neigh"].shape[1], radius)
    assert np.array_equal(active, g["active"])
    assert np.array_equal(neigh, g["neigh"])
    assert np.array_equal(nrad, g["nrad"])
    assert np.array_equal(nlist, g["n_pixels_list"])
    starts, tmax = O.time_intervals(r)
    assert np.array_equal(starts, g["track_starts"])
    assert tmax == int(g["max_length"])
    assert (g["active"] == -1).any()        # the -1 gap quirk is exercised


SAMPLED_SETS = [(c, "") for c in CFGS] + [(c, "corners_") for c in ("module0", "ndlar")
                                          if os.path.exists(os.path.join(os.path.dirname(__file__), "golden", f"sampled_corners_{c}.npz"))]


@pytest.mark.parametrize("cfg,tag", SAMPLED_SETS)
def test_tracks_current_sampled(cfg, tag):
    """Induced current at sampled ticks for diverse (segment, pixel) pairs incl. the pID == -1 quirk slots.  The `corners_`
    sets hold the degenerate geometries: segments hugging a TPC face, 0.5-50 um long, along / perpendicular to the drift axis,
    heavily ionising long ones (oracle/gen_golden.py:corner_segments)."""
    H.load_cfg(cfg)
    g = H.gold(f"sampled_{tag}{cfg}.npz")
    r = H.quench_drift(O, g["segments_in"])
    neigh = g["neigh"]
    T = int(g["max_length"])
    resp = H.response_for(g["response_kind"])
    sig = O.tracks_current(r, neigh, T, resp)
    got = sig[:, :, g["ticks"]]
    ref = g["signals"]
    assert (ref != 0).sum() > (100 if tag else 500)        # the corner sets hold a dozen ticks per pair
    # same operation order as the reference -> f32 outputs agree to the last bit or two
    np.testing.assert_allclose(got, ref, rtol=3e-7, atol=0)
    nz = ref != 0
    assert np.array_equal(got != 0, nz)


def test_chain_downstream_stages():
    """a13-a16 of the oracle vs the reference's own get_track_pixel_map2 / sum_pixel_signals / get_adc_values /
    digitize run on the golden chain (whose full-tick `signals` are oracle-made, spot-checked against the reference)."""
    H.load_cfg("module0")
    g = H.gold("chain_module0.npz")
    r = H.quench_drift(O, g["segments_in"])
    neigh, nrad = g["neigh"], g["nrad"]
    T = int(g["max_length"])
    sig = O.tracks_current(r, neigh, T, H.response_for(g["response_kind"]))
    assert np.array_equal(sig, g["signals"])
    upix = O.unique_pixels(neigh)
    assert np.array_equal(upix, g["unique_pix"])
    pim = O.pixel_index_map(neigh, upix)
    assert np.array_equal(pim, g["pixel_index_map"])
    M = consts.sim.MAX_TRACKS_PER_PIXEL
    tpm = O.track_pixel_map(upix, neigh, nrad, int(nrad.max()) + 1, M)
    assert np.array_equal(tpm, g["track_pixel_map"])
    ps, pts, ovf = O.sum_pixel_signals(g["signals"], g["track_starts"], pim, tpm, len(upix))
    np.testing.assert_allclose(ps, g["pixels_signals"], rtol=1e-13, atol=1e-13 * np.abs(g["pixels_signals"]).max())
    assert np.array_equal(ovf, g["overflow"])
    tt = np.linspace(0, consts.detector.TIME_INTERVAL[1], ps.shape[1] + 1)
    for name in ("default", "low"):
        thr = np.full(len(upix), float(g[f"threshold_{name}"]))
        adc, ticks, frac = O.get_adc_values(ps, pts, tt, thr)
        ref = g[f"adc_integral_{name}"]
        assert np.array_equal(adc != 0, ref != 0)
        np.testing.assert_allclose(adc, ref, rtol=1e-12)
        assert np.array_equal(ticks, g[f"adc_ticks_{name}"])
        hit = ref != 0
        np.testing.assert_allclose(frac[hit], g[f"adc_fractions_{name}"][hit], rtol=1e-10, atol=1e-14)
        assert np.array_equal(O.digitize(adc), g[f"adc_digit_{name}"])
    assert (g["adc_integral_low"] != 0).sum() >= 10


@pytest.mark.parametrize("variant", H.FEE_SCAN_VARIANTS)
def test_fee_scan_golden(variant):
    """The oracle's get_adc_values / digitize against the reference's own (fee.py:499-655) on the hand-made waveforms of
    oracle/gen_golden.py gen_fee: failed triggers, hits past the end of the waveform, the MAX_ADC_VALUES cap, true_q <= 0,
    no buffer rise time, interval / busy delay / reset longer than 64 ticks, thresholds <= 0 and, in `noisy`, the order in which
    the scan consumes its normals (the reference ran on the oracle's restated stream: same states afterwards)."""
    try:
        g, tt = H.load_fee_scan_case(variant)
        noisy = variant == "noisy"
        states = O.rng_create_states(len(g["thresholds"]), int(g["rng_seed"])) if noisy else None
        adc, ticks, frac = O.get_adc_values(g["pixels_signals"], g["pixels_signals_tracks"], tt, g["thresholds"],
                                            rng_states=states)
        H.assert_fee_scan_matches(g, adc, ticks, frac, O.digitize(adc), noisy)
        if noisy:
            assert np.array_equal(states.view("u8").reshape(-1, 2), g["rng_states_after"])
    finally:
        H.load_cfg("module0")


def test_numba_f32_typing_effect_is_recorded():
    """DESIGN.md §2 typing caveat: Numba keeps f32 (op) f32 in single precision for f4 record fields.  The oracle can
    emulate those spots; the induced current then moves by ~2e-7 of the waveform peak (median), <1e-3 worst case."""
    H.load_cfg("module0")
    from larndsim_amd import batching, synth
    seg = synth.make_segments(6, seed=77, segs_per_event=6)
    batching.swap_coordinates(seg)
    O.quench(seg, 2)
    O.drift(seg)
    nmax = O.max_pixels(seg)
    _, neigh, _, _ = O.get_pixels(seg, nmax, 3 * nmax + 6, 1)
    _, T = O.time_intervals(seg)
    resp = synth.make_response("dense")
    a = O.tracks_current(seg, neigh, T, resp).astype(np.float64)
    O.lib().o_set_numba_f32(1)
    try:
        b = O.tracks_current(seg, neigh, T, resp).astype(np.float64)
    finally:
        O.lib().o_set_numba_f32(0)
    pk = np.abs(a).max(-1)
    ok = (neigh >= 0) & (pk > 0)
    rel = np.abs(a - b).max(-1)[ok] / pk[ok]
    assert 0 < np.median(rel) < 5e-6 and rel.max() < 1e-3


@pytest.mark.parametrize("cfg", ["module0", "2x2_no_modvar"])
def test_light_golden(cfg):
    """a17/a18: light incidence (voxel lookup) and photon sum vs the reference on a synthetic LUT."""
    from larndsim_amd import synth
    H.load_cfg(cfg)
    g = H.gold(f"light_{cfg}.npz")
    r = H.quench_drift(O, g["segments_in"])
    lut = synth.make_lut((14, 26, 8), 48, int(g["n_prof"]), int(g["lut_seed"]))
    nph, t0d, vox = O.light_incidence(r, lut)
    assert np.array_equal(vox, g["voxel"])
    assert np.array_equal(nph, g["n_photons_det"])
    assert np.array_equal(t0d, g["t0_det"])
    n_ticks = int(g["n_ticks"])
    Mt = g["true_id"].shape[-1]
    out, tid, tph = O.sum_light_signals(r, vox, np.arange(len(r)), g["n_photons_det"], g["op_channel"], lut,
                                        float(g["t_start"]), n_ticks, g["sorted_indices"], max_truth=Mt)
    # the generator ran with f8 LUT mirrors (f64 product); the real f4 fields make Numba's product f32: <=1 ulp of f32
    np.testing.assert_allclose(out, g["light_sample_inc"], rtol=3e-7, atol=0)
    assert np.array_equal(tid, g["true_id"])
    assert g["light_sample_inc"].sum() > 0


@pytest.mark.parametrize("cfg", ["module0", "2x2_no_modvar"])
def test_light_response_golden(cfg):
    """light_sim.calc_scintillation_effect and calc_light_detector_response: the oracle is bit-identical
    to the reference's own functions -- f4 waveforms (every term's f4 store included), truth ids and truth photons -- for
    the RLC SiPM model (module0 case) and the measured-impulse model with interpolation (2x2 case)."""
    g = H.load_light_response_case(cfg)
    tid, tph = g["true_id"].astype(np.int64), g["true_photons"]
    scint, s_id, s_ph = O.scintillation_effect(g["light_sample_inc"], tid, tph)
    assert np.array_equal(scint, g["scint"]) and scint.dtype == np.float32
    assert np.array_equal(s_id, g["scint_true_id"]) and np.array_equal(s_ph, g["scint_true_photons"])
    assert (scint[-1] == 0).all() and scint.sum() > 0                      # the empty channel stays empty
    resp, r_id, r_ph = O.light_detector_response(g["disc"], consts.light.LIGHT_GAIN, consts.light.IMPULSE_MODEL,
                                                 g["scint_true_id"].astype(np.int64), g["scint_true_photons"])
    assert np.array_equal(resp, g["response"])
    assert np.array_equal(r_id, g["response_true_id"]) and np.array_equal(r_ph, g["response_true_photons"])
    # without truth slots the waveforms are the same
    assert np.array_equal(O.scintillation_effect(g["light_sample_inc"])[0], g["scint"])
    assert np.array_equal(O.light_detector_response(g["disc"], consts.light.LIGHT_GAIN, consts.light.IMPULSE_MODEL)[0],
                          g["response"])



@pytest.mark.parametrize("name", H.LIGHT_WVFM_CASES)
def test_light_waveform_chain_golden(name):
    """calc_stat_fluctuations, get_triggers, gen_light_detector_noise and sim_triggers/digitize_signal of the oracle against
    the reference's own functions (light_sim.py:186-238, 339-619; oracle/gen_golden.py gen_light_wvfm).  The random
    generator under calc_stat_fluctuations is the restated one on both sides (third-party, unpinned): what this pins is
    the Poisson logic, the state indexing and the number of draws."""
    g = H.load_light_wvfm_case(name)
    # Poisson fluctuations
    states = np.ascontiguousarray(g["fluct_states_before"]).view(O.RNG_DTYPE).reshape(-1)
    disc = O.stat_fluctuations(g["fluct_inc"], states)
    assert np.array_equal(disc, g["fluct_disc"])
    assert np.array_equal(states.view('u8').reshape(-1, 2), g["fluct_states_after"])
    assert (disc > 0).sum() > 500 and disc[0, 0] == 0 and disc[0, 1] == 0
    # triggers
    trig, trig_op, trig_type = O.get_triggers(g["response"], g["group_threshold"], g["op_channel"], 0)
    assert np.array_equal(trig, g["trigger_idx"]) and np.array_equal(trig_op, g["trigger_op_channel_idx"])
    assert np.array_equal(trig_type, g["trigger_type"])
    assert len(O.get_triggers(g["response"], g["group_threshold"], g["op_channel"], 1)[0]) == int(g["n_trig_subbatch1"])
    # noise with the recorded phases: the values are integers x 2**(16-NBIT); the FFT sizes are the reference's
    for n in (1500, 1501):
        ref = g[f"noise_{n}"]
        ph = H.det_phases((ref.shape[0], n // 2 + 1), int(g[f"noise_{n}_phase_seed"]))
        got = O.gen_light_detector_noise(ref.shape, g["noise_spectrum"][:ref.shape[0]], ph)
        assert np.array_equal(got, ref)
    # digitised waveforms
    keep = g["wvfm_keep_rows"]
    args = (g["response"][keep], g["op_channel"][keep], g["response_true_id"][keep].astype('i8'),
            g["response_true_photons"][keep], g["trigger_idx"], g["trigger_op_channel_idx"], int(g["digit_samples"]))
    d, dt, dp = O.sim_triggers(*args, np.zeros_like(g["noise_spectrum"]))
    assert np.array_equal(d, g["wvfm_quiet"]) and np.array_equal(dt, g["wvfm_true_id"])
    np.testing.assert_allclose(dp, g["wvfm_true_photons"], rtol=1e-15, atol=0)
    assert (dt >= 0).sum() > 100 and (d != 0).sum() > 100
    R = int(keep.sum())
    Tp = None
    # phases of the two noise calls: (rows, Tp//2+1) with Tp the padded length -- recompute it the way sim_triggers does
    l = consts.light
    pre = int(np.ceil(l.LIGHT_TRIG_WINDOW[0] / l.LIGHT_TICK_SIZE)); post = int(np.ceil(l.LIGHT_TRIG_WINDOW[1] / l.LIGHT_TICK_SIZE))
    tmin, tmax = int(g["trigger_idx"].min()), int(g["trigger_idx"].max())
    n0 = max(pre - tmin, 0)
    Tp = g["response"].shape[1] + n0
    Tp += max(post + tmax + n0 - Tp, 0)
    seeds = g["wvfm_noisy_phase_seeds"]
    n_missing = len(np.setdiff1d(np.unique(g["trigger_op_channel_idx"]), g["op_channel"][keep]))
    ph_sig = H.det_phases((R, Tp // 2 + 1), int(seeds[0]))
    ph_mis = H.det_phases((n_missing, Tp // 2 + 1), int(seeds[1])) if len(seeds) > 1 else None
    d2, _, _ = O.sim_triggers(*args, g["noise_spectrum"], phases_signal=ph_sig, phases_missing=ph_mis)
    assert np.array_equal(d2, g["wvfm_noisy"])


def _oracle_sim(sig, sop, tid, tph, trig, top, ns, tab, ph_sig, ph_mis):
    return O.sim_triggers(sig, sop, tid, tph, trig, top, ns, tab, phases_signal=ph_sig, phases_missing=ph_mis)


@pytest.mark.parametrize("name", H.LIGHT_WVFM_EDGE_TRIGGER_CASES)
def test_light_wvfm_edge_triggers(name):
    """The oracle's get_triggers against the reference's own (light_sim.py:380-477) at sample factors 1, 2, 3, 4, 7, 8, 13 and
    128, ratios that round half to even, an all-padding block, a block mean equal to its threshold, an f4 group sum that
    cancels, the re-slicing of a third trigger, a trigger on the last tick and groups of 64 rows across two modules
    (oracle/gen_golden.py gen_light_wvfm_edges)."""
    try:
        g = H.load_light_wvfm_edge_case(name)
        assert round(consts.light.LIGHT_DIGIT_SAMPLE_SPACING / consts.light.LIGHT_TICK_SIZE) == int(g["sample_factor"])
        H.assert_light_wvfm_edge_triggers(g, O.get_triggers)
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("name", H.LIGHT_WVFM_EDGE_NOISE_CASES)
def test_light_wvfm_edge_noise(name):
    """The oracle's gen_light_detector_noise against the reference's own (light_sim.py:339-377) for 2..17 and 1026..1028
    samples, desired frequencies that equal table frequencies, and a table that ends below most of them."""
    try:
        g = H.load_light_wvfm_edge_case(name)
        H.assert_light_wvfm_edge_noise(g, O.gen_light_detector_noise)
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("name", H.LIGHT_WVFM_EDGE_DIGIT_CASES)
def test_light_wvfm_edge_digitiser(name):
    """The oracle's sim_triggers against the reference's sim_triggers / digitize_signal (light_sim.py:480-619) at a spacing
    ratio of 2.5 and at tick 0.0007 (interp's lerp, truth photons interpolated between ticks, the next tick's slots
    searched), sample ticks past the end, an odd padded length under noise, and f4 signals with and without appended
    channels -- in the all-f64 mode and, where Numba's f4 typing cannot apply, in the numba_f32 mode too."""
    try:
        g = H.load_light_wvfm_edge_case(name)
        H.assert_light_wvfm_edge_digit(g, _oracle_sim)
        if name in ("all_rows_f4", "missing_rows_f4"):
            O.lib().o_set_numba_f32(1)
            try:
                typed = _oracle_sim(g["signal"], g["signal_op_channel"], np.zeros(g["signal"].shape + (0,), dtype='i8'),
                                    np.zeros(g["signal"].shape + (0,)), g["trigger_sets"][0], np.stack([np.arange(96)] * 2),
                                    int(g["digit_samples"]), np.zeros((96, 9)), None, None)[0]
            finally:
                O.lib().o_set_numba_f32(0)
            differ = int((typed != g["wvfm_0"]).sum())
            print(name, "numba_f32 mode differs from the reference in", differ, "of", typed.size, "values")
            if name == "missing_rows_f4":
                # appending the missing channels made the reference's array f8 (light_sim.py:601): no f4 difference is left
                assert differ == 0
            else:
                # the reference's run cannot type like Numba: this mode is pinned by the oracle alone; it must be another result
                assert differ > 0
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("name", H.LIGHT_EDGE_INCIDENCE_CASES)
def test_light_edge_incidence(name):
    """The oracle's light_incidence and get_nticks against the reference's own calculate_light_incidence and get_nticks
    (lightLUT.py:15-136, light_sim.py:24-41; oracle/gen_golden.py gen_light_edges) on voxel faces, borders, the 2e-2 margin and
    points beyond it in even and odd TPCs, LUTs of 1x1x1 to 14x26x8 voxels and of 6 and 48 detectors, a module's slice of the
    channels, trigger mode 1, efficiencies that are zero, negative and NaN, and records and voxels without light -- written
    into arrays that hold sentinels.  Voxels, n_photons_det and t0_det bit for bit (NaN where the reference has NaN, -0.0
    where it has -0.0); rows of segments outside every TPC, and t0_det in trigger mode 1, keep the sentinels."""
    from larndsim_amd import light_sim
    try:
        g = H.load_light_edge_case(name)
        s_nph, s_t0, s_vox = H.LIGHT_EDGE_SENTINELS
        for k in range(int(g["n_runs"])):
            pre = f"r{k}_"
            r, lut, n_out = H.light_edge_records(g, pre), H.light_edge_lut(g, pre), int(g[pre + "n_out"])
            n = len(r)
            init = (np.full((n, n_out), s_nph, dtype='f4'), np.full((n, n_out), s_t0, dtype='f4'), np.full((n, 3), s_vox, dtype='i4'))
            nph, t0d, vox = O.light_incidence(r, lut, n_out=n_out, init=init)
            assert np.array_equal(vox, g[pre + "voxel"]), (name, k)
            H.assert_same_floats(nph, g[pre + "n_photons_det"], f"{name} run {k} n_photons_det")
            H.assert_same_floats(t0d, g[pre + "t0_det"], f"{name} run {k} t0_det")
            inc = np.zeros((n, n_out), dtype=H.LIGHT_EDGE_INC_DTYPE)
            inc['n_photons_det'], inc['t0_det'] = nph, t0d
            n_ticks, start = light_sim.get_nticks(inc)
            assert n_ticks == int(g[pre + "n_ticks"]) and float(start) == float(g[pre + "start_time"]), (name, k)
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("name", H.LIGHT_EDGE_SUM_CASES)
def test_light_edge_photon_sum(name):
    """The oracle's light_incidence, get_nticks and sum_light_signals against the reference's own (light_sim.py:58-129) on
    arrival times that lie on the tick grid (most of them in no tick, some in two: reproduced, not repaired), start times
    get_nticks gives and others, the pre-filter without smearing, the ends of the axis and axes of one and two ticks, and the
    truth-slot rules (shared tracks, more tracks than slots, id -1, photons equal to the threshold, a visiting order that is not
    descending, arrays and slots that hold something already).  Every value is dyadic, so sums, ids and slot photons are
    compared bit for bit."""
    from larndsim_amd import light_sim
    try:
        g = H.load_light_edge_case(name)
        r, lut = H.light_edge_records(g), H.light_edge_lut(g)
        n = len(r)
        nph, t0d, vox = O.light_incidence(r, lut)
        assert np.array_equal(vox, g["voxel"])
        H.assert_same_floats(nph, g["n_photons_det"], name + " n_photons_det")
        H.assert_same_floats(t0d, g["t0_det"], name + " t0_det")
        inc = np.zeros(nph.shape, dtype=H.LIGHT_EDGE_INC_DTYPE)
        inc['n_photons_det'], inc['t0_det'] = nph, t0d
        n_ticks, start = light_sim.get_nticks(inc)
        assert n_ticks == int(g["own_n_ticks"]) and float(start) == float(g["own_start_time"])
        for k in range(int(g["n_runs"])):
            pre = f"r{k}_"
            T, M = int(g[pre + "n_ticks"]), int(g[pre + "max_truth"])
            out, tid, tph = O.sum_light_signals(r, vox, g["track_id"], nph, g["op_channel"], lut, float(g[pre + "start_time"]), T,
                                                g["sorted_indices"], max_truth=M, init=H.light_edge_sum_init(g, k))
            H.assert_same_floats(out, g[pre + "light_sample_inc"], f"{name} run {k} sum")
            assert np.array_equal(tid, g[pre + "true_id"]), (name, k)
            H.assert_same_floats(tph, g[pre + "true_photons"], f"{name} run {k} truth photons")
            assert g[pre + "light_sample_inc"].sum() > 0 and (g[pre + "true_id"] != -1).any()
            # without truth slots: the same sums
            out0, _, _ = O.sum_light_signals(r, vox, g["track_id"], nph, g["op_channel"], lut, float(g[pre + "start_time"]), T,
                                             g["sorted_indices"], max_truth=0, init=H.light_edge_sum_init(g, k))
            H.assert_same_floats(out0, g[pre + "light_sample_inc"], f"{name} run {k} sum without slots")
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("radius", H.WIDE_RADII)
@pytest.mark.parametrize("cfg", H.WIDE_CFGS)
def test_wide_neighbourhood_golden(cfg, radius):
    """get_pixels at radius 1-4 handed in as its argument, the unique pixels, the index map, get_track_pixel_map2 and
    sum_pixel_signals of the oracle against the reference's own (oracle/gen_golden.py gen_pixels_wide): neighbourhoods clipped by
    an edge and a corner of the pixel plane, a segment leaving the plane, one outside every TPC, ring codes 0-8, the -1 of
    |dx| + |dy| > 4 from radius 3 on (pixels that are unique pixels yet take no track), and the slots kept in ring order when
    MAX_TRACKS_PER_PIXEL is too small.  Integers exact; the sums to rtol 1e-12 and 1e-12 of the largest sum."""
    H.load_cfg(cfg)
    g, signals, starts = H.wide_case(cfg, radius)
    r = H.quench_drift(O, g["segments_in"])
    assert O.max_pixels(r) == int(g["max_pixels"])
    P = g["neigh"].shape[1]
    assert P == (2 * radius + 1) * int(g["max_pixels"]) + (1 + 2 * radius) * radius * 2
    active, neigh, nrad, nlist = O.get_pixels(r, int(g["max_pixels"]), P, radius)
    assert np.array_equal(active, g["active"])
    assert np.array_equal(neigh, g["neigh"])
    assert np.array_equal(nrad, g["nrad"])
    assert np.array_equal(nlist, g["n_pixels_list"])
    upix = O.unique_pixels(neigh)
    assert np.array_equal(upix, g["unique_pix"])
    pim = O.pixel_index_map(neigh, upix)
    assert np.array_equal(pim, g["pixel_index_map"])
    # what the fixture is there for
    codes = set(np.unique(nrad[neigh >= 0]).tolist())
    assert codes == {1: {0, 1, 2}, 2: {0, 1, 2, 3, 4, 6}, 3: set(range(-1, 8)), 4: set(range(-1, 9))}[radius]
    assert (active[3] == -1).any() and nlist[4] == 0 and (neigh[4] == -1).all()
    for tag, M in (("", consts.sim.MAX_TRACKS_PER_PIXEL), ("_low", int(g["max_tracks_low"]))):
        tpm = O.track_pixel_map(upix, neigh, nrad, int(nrad.max()) + 1, M)
        assert np.array_equal(tpm, g["track_pixel_map" + tag])
        ps, pts, ovf = O.sum_pixel_signals(signals, starts, pim, tpm, len(upix))
        top = H.sparse_field(g, "pixels_signals" + tag)[2].max()
        H.assert_sparse_close(ps, g, "pixels_signals" + tag, rtol=1e-12, atol=1e-12 * top)
        H.assert_sparse_close(pts, g, "pixels_tracks_signals" + tag, rtol=1e-12, atol=1e-12 * top)
        assert np.array_equal(ovf, g["overflow" + tag])
        no_slot = (tpm >= 0).sum(axis=1) == 0
        assert no_slot.any() == (radius >= 3) and not ps[no_slot].any()
        if tag:
            assert ((tpm >= 0).sum(axis=1) == M).any() and ovf.any()


@pytest.mark.parametrize("case", H.MC_CASES)
def test_mc_oracle_against_reference(case):
    """The oracle's tracks_current_mc against the reference's own (detsim.py:220-348, oracle/gen_golden.py gen_mc), both on the
    table streams this project defines (one per (segment, pixel, tick)): every entry of the unrounded sums to rtol 1e-12 and
    1e-12 of the case's largest entry (same host normals, same order of sums; libm's sqrt alone separates them), the same
    number of normals drawn by every entry, the same zero pattern.  The cases reach the z_start < z_end swap and its
    opposite, both clamps of overlapping_segment, nstep 1 / 3 / hundreds, MC_SAMPLE_MULTIPLIER 3, M = 2 (ndlar), time_tick < 0,
    an rr > impact row and a -1 slot per segment, and ticks past 256.  Not reached: k >= nk (TIME_WINDOW / RESPONSE_SAMPLING is
    below the tables' length: the generator counts 0 such look-ups) and a segment exactly along z (l == 0 divides by zero in
    the reference's pure-Python run; the kernel's "no signal" there is compared with the oracle alone)."""
    try:
        m, d, st = H.mc_oracle(case)
        S, P = m["pixels"].shape
        ref = m["signals"]
        assert np.array_equal(d["n_draws"], m["n_draws"])
        assert np.array_equal(d["signals64"] != 0, ref != 0) and (ref != 0).sum() > 500
        np.testing.assert_allclose(d["signals64"], ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
        # the unchanged entry point: the same bits, the float32 of the sums, every state stepped once
        st2 = O.rng_create_states(S * P, m["seed"])
        sig = O.tracks_current_mc(m["tracks"], m["pixels"], m["T"], m["response"], st2)
        assert np.array_equal(sig, d["signals"]) and np.array_equal(sig, d["signals64"].astype(np.float32))
        assert np.array_equal(st2.view("u8"), st.view("u8"))
        # the appended columns: a pixel beyond the impact radius and a -1, per segment
        assert (m["pixels"][:, -1] == -1).all() and (m["pixels"][:, -2] >= 0).all()
        assert not ref[:, -2:].any() and not m["n_draws"][:, -2:].any()
        nstep = {n: m["n_draws"][i][m["n_draws"][i] > 0].min() for i, n in enumerate(m["names"])}
        if case == "module0_plain":
            assert nstep["tiny"] == 1 and nstep["inside"] == 3 and nstep["steep"] > 256
            i, j = m["names"].index("diag"), m["names"].index("diag_swapped")
            assert m["tracks"]["z_start"][i] < m["tracks"]["z_end"][i] and m["tracks"]["z_start"][j] > m["tracks"]["z_end"][j]
        if case == "module0_multi":
            assert consts.sim.MC_SAMPLE_MULTIPLIER == 3 and all(v % 3 == 0 for v in nstep.values())
        if case == "ndlar_plain":
            assert round(consts.detector.TIME_SAMPLING / consts.detector.RESPONSE_SAMPLING) == 2
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("case", H.MC_CASES)
def test_mc_oracle_supplied_normals(case):
    """The supplied-normals entry fed the table streams' normals as arrays (segment by segment: the steep one draws up to 1050
    per entry) returns the table entry point's signals, sums and draw counts bit for bit, and with the radii its margins."""
    try:
        m, d, st = H.mc_oracle(case)
        S, P = m["pixels"].shape
        T = m["T"]
        states = O.rng_create_states(S * P, m["seed"])
        for i in range(S):
            cnt = d["n_draws"][i:i + 1]
            D = int(cnt.max())
            nrm, rad = O.mc_stream_normals(states, S, P, T, D, segments=(i, i + 1), count=cnt, want_radii=True)
            got = O.tracks_current_mc_normals(m["tracks"][i:i + 1], m["pixels"][i:i + 1], T, m["response"], nrm, rad)
            for k in ("signals", "signals64", "n_draws", "margin"):
                assert np.array_equal(got[k][0], d[k][i]), (m["names"][i], k)
            if D > 1:
                with pytest.raises(ValueError, match="more than the"):
                    O.tracks_current_mc_normals(m["tracks"][i:i + 1], m["pixels"][i:i + 1], T, m["response"], nrm[..., :D - 1])
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("case", H.MC_CASES)
def test_mc_fragile_entries_are_few(case):
    """At most 1 % of a case's non-zero entries may have a decision (window edge, reach cut, rounding of i, j, k) within 8
    float32 spacings of a draw's Box-Muller radius: those are the entries the device's normals may legitimately move (the
    GPU test leaves them out).  Shares: module0_plain 0.00061, module0_multi 0.00082, ndlar_plain 0.00129."""
    try:
        m, d, st = H.mc_oracle(case)
        nz = m["signals"] != 0
        fragile = float((d["margin"][nz] < H.MC_FRAGILE_MARGIN).mean())
        print(case, "share of non-zero entries with margin below", H.MC_FRAGILE_MARGIN, ":", fragile)
        assert fragile == m["fragile_share"]
        assert fragile <= H.MC_FRAGILE_CAP
        assert np.isinf(d["margin"][m["n_draws"] == 0]).all() and (d["margin"][m["n_draws"] > 0] < np.inf).all()
    finally:
        H.load_cfg("module0")
