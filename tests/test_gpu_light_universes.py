"""GPU: light universes (ChargeChain.light_universes, ldsim_dev_light_universes, simulate_pixels.py --light_universes).

The case is the one of test_gpu_parity.py::test_resident_light_waveform_chain_vs_oracle: module0, the light golden's 40 segments,
all 96 rows, keyed streams.  LIGHT_WINDOW = (0.2, 1.5): C = 1300 ticks, more than one 1024-tick chunk of the kernels; the tick
axis is cut to 1531 ticks (no multiple of 256 or 64; several workgroups per row), and to 1003 ticks for the case C > n_ticks.  The
oracle's loops are about 2e8 terms per stage (one to three seconds each)."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

import helpers as H
from larndsim_amd import consts, lib, light_sim, synth
from larndsim_amd import light_universes as LU
from larndsim_amd import rng as lrng
from larndsim_amd.chain import ChargeChain
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
CALL_KEY = lrng.call_key(1, 3, 0, 0)
WINDOW = (0.2, 1.5)
T_MAIN, T_SHORT = 1531, 1003
NU = 4                                     # tables per launch of light_plain_kernel (option light_universes_nu)


@pytest.fixture(autouse=True)
def _leave_the_context_as_found():
    yield
    H.load_cfg("module0")
    lib.set_option("light_universes_nu", NU)
    lib.check(lib.load().ldsim_rng_clear(lib.context()))


def _launch(model=1, n_ticks=T_MAIN, mt=0, keyed=True, impulse=None):
    """the photon sum of the case, resident: (chain, op channels, n_ticks)"""
    H.load_cfg("module0")
    light = consts.light
    light.LIGHT_WINDOW = WINDOW
    light.LIGHT_TRIG_WINDOW = (0.2, 0.5)
    light.SIPM_RESPONSE_MODEL = model
    if impulse is not None:
        light.IMPULSE_MODEL = np.asarray(light.IMPULSE_MODEL, dtype=float)[:impulse]
    consts.sim.MAX_MC_TRUTH_IDS = mt
    g = H.gold("light_module0.npz")
    r = H.quench_drift(O, g["segments_in"])
    n = len(r)
    lut = synth.make_lut((14, 26, 8), 48, int(g["n_prof"]), int(g["lut_seed"]))
    ch = ChargeChain()
    ch.upload(r, np.zeros(n, dtype=np.int32))
    ch.light_incidence(lut)
    opc = light.TPC_TO_OP_CHANNEL[:].ravel()
    nt, _ = ch.sum_light(0, n, opc, np.arange(n, dtype='i8'), max_ticks=n_ticks)
    assert nt == n_ticks and nt % 64 != 0 and LU.conv_ticks() == 1300 and opc.shape[0] == 96
    if keyed:
        ch.seed_keyed(77)
        ch.set_rng_key(CALL_KEY)
    return ch, opc, nt


def _knob(name, nominal):
    return {"photon_0.5": dict(photon_scale=0.5), "photon_50": dict(photon_scale=50.0), "singlet_0.2": dict(singlet_fraction=0.2),
            "tau_s_x2": dict(tau_s=nominal["tau_s"] * 2), "tau_t_x0.8": dict(tau_t=nominal["tau_t"] * 0.8),
            "gain_1.1": dict(gain_scale=1.1), "gain_-1": dict(gain_scale=-1.0),
            "response_time_x1.2": dict(response_time=nominal["response_time"] * 1.2),
            "oscillation_period_x0.9": dict(oscillation_period=nominal["oscillation_period"] * 0.9)}[name]


KNOBS = ("photon_0.5", "photon_50", "singlet_0.2", "tau_s_x2", "tau_t_x0.8", "gain_1.1", "gain_-1", "response_time_x1.2",
         "oscillation_period_x0.9")


def _model_of(name):
    return 0 if name.startswith(("response_time", "oscillation_period")) else 1


def _patch(v):
    """consts.light under variation v (the gain is the caller's); returns the patched row gains"""
    light = consts.light
    light.SINGLET_FRACTION, light.TAU_S, light.TAU_T = v["singlet_fraction"], v["tau_s"], v["tau_t"]
    light.LIGHT_RESPONSE_TIME, light.LIGHT_OSCILLATION_PERIOD = v["response_time"], v["oscillation_period"]
    return np.asarray(light.LIGHT_GAIN, dtype=np.float64) * v["gain_scale"]


def _thresholds(resp, n_ticks):
    per = consts.light.OP_CHANNEL_PER_TRIG
    gsum = resp.reshape(-1, per, n_ticks).sum(axis=1)
    nd = resp.shape[0]
    return np.full(nd // per, float(np.sort(gsum.min(axis=1))[nd // per // 2]) * 0.5)       # about half of the groups fire


def _digit_samples():
    light = consts.light
    return int(np.ceil((light.LIGHT_TRIG_WINDOW[1] + light.LIGHT_TRIG_WINDOW[0]) / light.LIGHT_DIGIT_SAMPLE_SPACING))


def _noise_spectrum():
    return np.abs(np.random.default_rng(3).normal(0, 4000.0, (consts.light.N_OP_CHANNEL, 65)))


# ---- nominal ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fluctuate,n_ticks", [(True, T_MAIN), (False, T_MAIN), (True, T_SHORT)])
def test_nominal_universe_is_the_launch(fluctuate, n_ticks):
    """[nominal] gives scint, disc and response byte-equal to the launch's own download (without fluctuations the launch leaves
    its disc array unwritten and the universe's disc is its scint); triggers and waveforms equal those of the resident launch,
    without noise and with a keyed noise spectrum"""
    ch, opc, nt = _launch(n_ticks=n_ticks)
    nominal = LU.nominal()
    assert ch.light_variation_nominal() == nominal
    ch.light_response(fluctuate=fluctuate)
    sc0, di0, rp0, _, _ = ch.download_light_response(stages=True)
    assert np.abs(rp0).max() > 0 and sc0.sum() > 0
    ch.light_universes([nominal], fluctuate=fluctuate, keep_stages=True)
    sc, di, rp = ch.download_light_universe(0, stages=True)
    assert sc.tobytes() == sc0.tobytes() and rp.tobytes() == rp0.tobytes()
    if fluctuate:
        assert di.tobytes() == di0.tobytes() and not np.array_equal(di, sc)
    else:
        assert di.tobytes() == sc.tobytes()
    assert np.array_equal(ch.download_light_universe(0), rp0)
    thr = _thresholds(rp0, nt)
    ns = _digit_samples()
    trig, trig_op, trig_type = light_sim.get_triggers(None, thr, opc, 0)
    u_trig, u_op, u_type = light_sim.get_triggers_universe(0, thr, opc, 0)
    assert len(trig) > 0 and np.array_equal(trig, u_trig) and np.array_equal(trig_op, u_op) and np.array_equal(trig_type, u_type)
    for noise in (None, _noise_spectrum()):
        d = light_sim.sim_triggers(None, None, None, opc, None, None, trig, trig_op, ns, noise)[0]
        u_d = light_sim.sim_triggers_universe(0, opc, trig, trig_op, ns, noise)
        assert d.tobytes() == u_d.tobytes() and (d != 0).sum() > 50
    ms = ch.light_universes_ms()
    assert ms["scintillation"] > 0 and ms["detector_response"] > 0 and ms["fluctuations"] >= 0


# ---- one universe per knob against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KNOBS)
def test_universe_against_the_oracle(name):
    """scint_k against the oracle's scintillation_effect on the host-scaled input under the patched constants, resp_k against the
    oracle's light_detector_response fed the device's own disc_k (a one-count difference cannot propagate): array_equal"""
    model = _model_of(name)
    ch, opc, nt = _launch(model=model)
    nominal = LU.nominal()
    v = dict(nominal, **_knob(name, nominal))
    ch.light_universes([v], fluctuate=True, keep_stages=True)
    sc, di, rp = ch.download_light_universe(0, stages=True)
    inc = ch.download_light()[0]
    x = LU.scaled_input(inc, v["photon_scale"])
    gain = _patch(v)
    o_sc = O.scintillation_effect(x)[0]
    assert np.array_equal(sc, o_sc) and o_sc.sum() > 0
    o_rp = O.light_detector_response(di, gain, consts.light.IMPULSE_MODEL)[0]
    assert np.array_equal(rp, o_rp) and np.abs(o_rp).max() > 0
    mean = sc.astype(np.float64) * consts.light.LIGHT_TICK_SIZE
    print(name, "largest Poisson mean", mean.max(), "elements below / above 30:", ((mean > 0) & (mean < 30)).sum(), (mean >= 30).sum())
    if name == "photon_50":          # both Poisson branches
        assert ((mean > 0) & (mean < 30)).sum() > 100 and (mean >= 30).sum() > 100


# ---- against a fresh launch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 0])
def test_universes_equal_fresh_launches(model):
    """every knob but photon_scale: constants (and gains) patched, refresh_constants, light_response under the same call key --
    all three stages byte-equal to the universe's"""
    ch, opc, nt = _launch(model=model)
    nominal = LU.nominal()
    names = [n for n in KNOBS if not n.startswith("photon") and (model == 0 or _model_of(n) == 1)]
    assert len(names) == (7 if model == 0 else 5)
    vs = [dict(nominal, **_knob(n, nominal)) for n in names]
    ch.light_universes(vs, fluctuate=True, keep_stages=True)
    got = [ch.download_light_universe(k, stages=True) for k in range(len(vs))]
    gain0 = np.asarray(consts.light.LIGHT_GAIN, dtype=np.float64).copy()
    for n, v, (sc, di, rp) in zip(names, vs, got):
        consts.light.LIGHT_GAIN = gain0
        consts.light.LIGHT_GAIN = _patch(v)
        ch.refresh_constants()
        ch.set_rng_key(CALL_KEY)
        ch.light_response(fluctuate=True)
        f_sc, f_di, f_rp, _, _ = ch.download_light_response(stages=True)
        assert sc.tobytes() == f_sc.tobytes(), n
        assert di.tobytes() == f_di.tobytes(), n
        assert rp.tobytes() == f_rp.tobytes(), n
    assert len({g[2].tobytes() for g in got}) == len(got)


# ---- Poisson under photon_scale -----------------------------------------------------------------------------------------------------------
def test_poisson_counts_under_photon_scale():
    """disc_k of the photon_scale 50 universe against the inversion / truncated-normal rule evaluated on the host from the keyed
    draws of the same stream keys (key_mix(key_mix(call key, row), tick), draw 0 of the fluctuation tag): the bar for the device's
    exp against libm of test_resident_light_waveform_chain_vs_oracle -- fewer than 1e-3 of the values differ, each by one count"""
    ch, opc, nt = _launch()
    v = dict(LU.nominal(), photon_scale=50.0)
    ch.light_universes([v], fluctuate=True, keep_stages=True)
    sc, di, _ = ch.download_light_universe(0, stages=True)
    rows, ticks = np.meshgrid(np.arange(sc.shape[0], dtype=np.int64), np.arange(nt, dtype=np.int64), indexing="ij")
    keys = lrng.key_mix(lrng.key_mix(np.uint64(CALL_KEY), rows.ravel()), ticks.ravel())
    u = lrng.keyed_draws(keys, 1, tag=lrng.TAG_LIGHT_FLUCT, normal=False, ctx=ch.ctx)[:, 0].reshape(sc.shape)
    z = lrng.keyed_draws(keys, 1, tag=lrng.TAG_LIGHT_FLUCT, normal=True, ctx=ch.ctx)[:, 0].reshape(sc.shape)
    want = LU.poisson_counts(sc, u, z)
    mean = sc.astype(np.float64) * consts.light.LIGHT_TICK_SIZE
    assert ((mean > 0) & (mean < 30)).sum() > 100 and (mean >= 30).sum() > 100
    d = np.abs(di.astype(np.float64) - want.astype(np.float64))
    bad = d != 0
    print("Poisson: fraction that differs", bad.mean(), "distinct differences", np.unique(d[bad])[:4])
    assert bad.mean() < 1e-3 and np.all(d[bad] == np.float32(1.0 / consts.light.LIGHT_TICK_SIZE)), (bad.mean(), np.unique(d[bad])[:4])
    assert np.array_equal(di[sc <= 0], np.zeros((sc <= 0).sum(), dtype='f4')) and (di > 0).sum() > 100


# ---- grouping ---------------------------------------------------------------------------------------------------------------------------
def _grouping_universes(nominal):
    """64 universes over three inputs, interleaved: input 1.0 holds NU + 1 distinct scintillation keys, input 0.5 holds NU, input
    2.0 holds one; the first scintillation key of input 1.0 holds NU + 1 distinct response keys, its second NU, the others one;
    everything else repeats earlier universes"""
    sc_keys = [dict(), dict(singlet_fraction=0.2), dict(tau_s=nominal["tau_s"] * 2), dict(tau_t=nominal["tau_t"] * 0.8),
               dict(singlet_fraction=0.6, tau_t=nominal["tau_t"] * 1.1)]
    rs_keys = [dict(), dict(gain_scale=1.1), dict(response_time=nominal["response_time"] * 1.2),
               dict(oscillation_period=nominal["oscillation_period"] * 0.9), dict(gain_scale=-1.0)]
    distinct = []
    for i, s in enumerate(sc_keys):                                   # input 1.0
        n_rs = NU + 1 if i == 0 else NU if i == 1 else 1
        distinct += [dict(nominal, **s, **r) for r in rs_keys[:n_rs]]
    distinct += [dict(nominal, photon_scale=0.5, **s) for s in sc_keys[:NU]]
    distinct += [dict(nominal, photon_scale=2.0, tau_s=nominal["tau_s"] * 3, gain_scale=0.9)]
    rs = np.random.default_rng(11)
    order = rs.permutation(len(distinct))
    vs = [distinct[i] for i in order]
    while len(vs) < 64:
        vs.append(distinct[int(rs.integers(len(distinct)))])
    return vs


def test_grouping_gives_each_universe_what_it_gives_alone():
    """n = 1, NU, NU + 1, 9 and 64 universes with inputs, scintillation keys and response keys interleaved (groups of 1, NU and
    NU + 1 distinct tables at both stages): every universe byte-equal to itself run alone, duplicates byte-equal to each other; the
    same bits at every setting of the option light_universes_nu.  The settings select instances of one kernel (light_plain_kernel
    <RESPONSE, NU>, which the launch runs at NU = 1 too), so this sweep checks the grouping and that a pass does not read what the pool
    buffers held, not the sum itself: the plain sum is pinned independently by the golden files and the oracle tests of
    test_gpu_parity.py and by the Python twin of the universes in this file."""
    ch, opc, nt = _launch(model=0)
    nominal = LU.nominal()
    vs = _grouping_universes(nominal)
    assert len(vs) == 64 and len({tuple(v.items()) for v in vs}) == NU + 1 + NU + 3 + NU + 1
    alone = {}
    for v in vs:
        key = tuple(v.items())
        if key not in alone:
            ch.light_universes([v], fluctuate=True, keep_stages=True)
            alone[key] = tuple(a.tobytes() for a in ch.download_light_universe(0, stages=True))
    assert len({a[2] for a in alone.values()}) == len(alone)          # (distinct constants: distinct responses)
    for n in (1, NU, NU + 1, 9, 64):
        ch.light_universes(vs[:n], fluctuate=True, keep_stages=True)
        for k in range(n):
            got = tuple(a.tobytes() for a in ch.download_light_universe(k, stages=True))
            assert got == alone[tuple(vs[k].items())], (n, k)
    for nu in (1, 2, 3):
        lib.set_option("light_universes_nu", nu)
        ch.light_universes(vs[:24], fluctuate=True, keep_stages=True)
        for k in range(24):
            got = tuple(a.tobytes() for a in ch.download_light_universe(k, stages=True))
            assert got == alone[tuple(vs[k].items())], (nu, k)
    with pytest.raises(lib.LdsimError, match="light_universes_nu must be 1, 2, 3 or 4"):
        lib.set_option("light_universes_nu", 5)


def test_impulse_model_and_short_tick_axis():
    """SIPM_RESPONSE_MODEL 1 with a short impulse model (60 of 1300 ticks), on the tick axis shorter than the window (C > n_ticks):
    [nominal, gain 1.1, tau_s x 2, gain 1.1 again] -- each what it gives alone, the nominal the launch's, the response the
    oracle's on the device's counts; the RLC constants are refused by name"""
    ch, opc, nt = _launch(model=1, n_ticks=T_SHORT, impulse=60)
    nominal = LU.nominal()
    vs = [nominal, dict(nominal, gain_scale=1.1), dict(nominal, tau_s=nominal["tau_s"] * 2), dict(nominal, gain_scale=1.1)]
    ch.light_response(fluctuate=True)
    sc0, di0, rp0, _, _ = ch.download_light_response(stages=True)
    alone = []
    for v in vs:
        ch.light_universes([v], fluctuate=True, keep_stages=True)
        alone.append(tuple(a.tobytes() for a in ch.download_light_universe(0, stages=True)))
    ch.light_universes(vs, fluctuate=True, keep_stages=True)
    got = [ch.download_light_universe(k, stages=True) for k in range(4)]
    for k in range(4):
        assert tuple(a.tobytes() for a in got[k]) == alone[k], k
    assert alone[1] == alone[3] and alone[0] == (sc0.tobytes(), di0.tobytes(), rp0.tobytes())
    o_rp = O.light_detector_response(got[1][1], np.asarray(consts.light.LIGHT_GAIN, dtype=np.float64) * 1.1, consts.light.IMPULSE_MODEL)[0]
    assert np.array_equal(got[1][2], o_rp) and np.abs(o_rp).max() > 0
    with pytest.raises(ValueError, match="universe 1: response_time = .* is not read under SIPM_RESPONSE_MODEL 1"):
        ch.light_universes([nominal, dict(nominal, response_time=nominal["response_time"] * 1.2)])
    arr = LU.pack([dict(nominal, oscillation_period=nominal["oscillation_period"] * 0.9)])
    with pytest.raises(lib.LdsimError, match="universe 0: oscillation_period = .* is not read under SIPM_RESPONSE_MODEL 1"):
        _raw_call(ch, arr, 1)
    assert ch.download_light_universe(3).tobytes() == alone[3][2]          # (the refused calls left the result in place)


# ---- common random numbers ----------------------------------------------------------------------------------------------------------------
def test_common_random_numbers():
    """photon_scale 1.2 against 1.0: the same uniform per element, so counts drawn by inversion never decrease"""
    ch, opc, nt = _launch()
    nominal = LU.nominal()
    ch.light_universes([nominal, dict(nominal, photon_scale=1.2)], fluctuate=True, keep_stages=True)
    sc0, di0, _ = ch.download_light_universe(0, stages=True)
    sc1, di1, _ = ch.download_light_universe(1, stages=True)
    tick = consts.light.LIGHT_TICK_SIZE
    assert np.all(sc1 >= sc0) and (sc1 > sc0).sum() > 100
    inv = (sc0 > 0) & (sc1.astype(np.float64) * tick < 30)
    assert inv.sum() > 100 and np.all(di1[inv] >= di0[inv]) and (di1[inv] > di0[inv]).sum() > 0


# ---- triggers and waveforms of a universe --------------------------------------------------------------------------------------------------
def test_triggers_and_waveforms_of_a_universe():
    """get_triggers_universe / sim_triggers_universe equal the host-array calls on the downloaded resp_k (empty truth);
    trig_threshold_scale and noise_scale equal those calls with the scaled arguments; a threshold scale changes the trigger count"""
    ch, opc, nt = _launch()
    nominal = LU.nominal()
    vs = [nominal, dict(nominal, photon_scale=2.0, trig_threshold_scale=3.0, noise_scale=0.5),
          dict(nominal, gain_scale=-1.0, trig_threshold_scale=-1.0, noise_scale=0.0),
          dict(nominal, tau_t=nominal["tau_t"] * 0.8, trig_threshold_scale=0.05, noise_scale=2.0)]
    ch.light_universes(vs, fluctuate=True)
    resp = [ch.download_light_universe(k) for k in range(len(vs))]
    thr = _thresholds(resp[0], nt)
    ns = _digit_samples()
    noise = _noise_spectrum()
    empty_id, empty_ph = np.zeros((96, nt, 0), dtype=np.int64), np.zeros((96, nt, 0))
    counts = []
    for k, v in enumerate(vs):
        for scale in (1.0, v["trig_threshold_scale"]):
            trig, trig_op, trig_type = light_sim.get_triggers_universe(k, thr * scale, opc, 0)
            h_trig, h_op, h_type = light_sim.get_triggers(resp[k], thr * scale, opc, 0)
            assert np.array_equal(trig, h_trig) and np.array_equal(trig_op, h_op) and np.array_equal(trig_type, h_type), (k, scale)
            counts.append((k, scale, len(trig)))
            if not len(trig):
                continue
            for spectrum in (None, noise, noise * v["noise_scale"]):
                d = light_sim.sim_triggers_universe(k, opc, trig, trig_op, ns, spectrum)
                h_d = light_sim.sim_triggers(None, None, resp[k], opc, empty_id, empty_ph, trig, trig_op, ns, spectrum)[0]
                assert d.tobytes() == h_d.tobytes(), (k, scale)
    print("trigger counts (universe, threshold scale, triggers):", counts)
    by_k = {}
    for k, scale, n in counts:
        by_k.setdefault(k, []).append(n)
    assert any(len(set(ns_)) > 1 for ns_ in by_k.values()), counts          # a threshold scale changed a trigger count
    assert sum(n for _, _, n in counts) > 4
    trig, trig_op, _ = light_sim.get_triggers_universe(0, thr, opc, 0)
    quiet, loud, half = (light_sim.sim_triggers_universe(0, opc, trig, trig_op, ns, s) for s in (None, noise, noise * 0.5))
    assert len(trig) > 0 and (loud - quiet).std() > 1.5 * (half - quiet).std() > 0


# ---- the launch is left alone -----------------------------------------------------------------------------------------------------------------
def test_launch_untouched_and_result_invalidated():
    """around a 9-universe call everything of the launch is byte-identical: the three stages, the truth arrays (MAX_MC_TRUTH_IDS
    2), triggers and waveforms of the resident response (noise from the call key: the key is unchanged); the universes are refused
    after the next sum_light"""
    ch, opc, nt = _launch(mt=2)
    nominal = LU.nominal()
    ch.light_response(fluctuate=True)
    noise = _noise_spectrum()
    ns = _digit_samples()

    def snapshot():
        stages = ch.download_light_response(stages=True)
        thr = _thresholds(stages[2], nt)
        trig, trig_op, trig_type = light_sim.get_triggers(None, thr, opc, 0)
        wv = light_sim.sim_triggers(None, None, None, opc, None, None, trig, trig_op, ns, noise)
        return [a.tobytes() for a in stages] + [trig.tobytes(), trig_op.tobytes()] + [a.tobytes() for a in wv], len(trig), stages

    before, n_trig, stages = snapshot()
    assert n_trig > 0 and (stages[3] >= 0).sum() > 10
    vs = [nominal] + [dict(nominal, **_knob(n, nominal)) for n in KNOBS[:7]] + [dict(nominal, photon_scale=3.0, gain_scale=2.0)]
    assert len(vs) == 9
    ch.light_universes(vs, fluctuate=True, keep_stages=True)
    after, _, _ = snapshot()
    assert before == after
    sc, di, rp = ch.download_light_universe(0, stages=True)
    assert (sc.tobytes(), di.tobytes(), rp.tobytes()) == tuple(before[:3])          # (the plain sums of a launch with truth slots)
    g = H.gold("light_module0.npz")
    ch.sum_light(0, len(g["segments_in"]), opc, np.arange(len(g["segments_in"]), dtype='i8'), max_ticks=T_MAIN)
    with pytest.raises(lib.LdsimError, match="no resident light universes"):
        ch.download_light_universe(0)
    with pytest.raises(lib.LdsimError, match="no resident light universes"):
        light_sim.get_triggers_universe(0, _thresholds(stages[2], nt), opc, 0)
    # ... and after the next light_response
    ch.light_universes(vs[:2], fluctuate=True)
    assert ch.download_light_universe(1).shape == (96, nt)
    ch.light_response(fluctuate=True)
    with pytest.raises(lib.LdsimError, match="no resident light universes"):
        ch.download_light_universe(1)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def _raw_call(ch, arr, n, fluctuate=1, keep=1):
    light = consts.light
    gain = np.ascontiguousarray(light.LIGHT_GAIN, dtype=np.float64)
    imp = np.ascontiguousarray(light.IMPULSE_MODEL, dtype=np.float64)
    lib.check(lib.load().ldsim_dev_light_universes(ch.ctx, arr, C.c_int32(n), lib.ptr(gain), lib.ptr(imp), C.c_int32(imp.shape[0]),
                                                   C.c_int32(fluctuate), C.c_int32(keep)))


def test_errors_and_the_earlier_result_survives():
    ch, opc, nt = _launch(model=0)
    nominal = LU.nominal()
    vs = [nominal, dict(nominal, tau_s=nominal["tau_s"] * 2)]
    ch.light_universes(vs, fluctuate=True, keep_stages=False)
    kept = ch.download_light_universe(1).tobytes()
    # stages asked for but not kept, k out of range
    with pytest.raises(lib.LdsimError, match="ldsim error -4: .*were not kept"):
        ch.download_light_universe(1, stages=True)
    for k in (-1, 2):
        with pytest.raises(lib.LdsimError, match=f"ldsim error -1: .*universe {k} out of range, the last pass made 2"):
            ch.download_light_universe(k)
        with pytest.raises(lib.LdsimError, match="out of range"):
            light_sim.get_triggers_universe(k, np.full(16, -1e3), opc, 0)
    # n = 0 and 65: the Python layer and the library
    for n in (0, 65):
        with pytest.raises(ValueError, match=f"n = {n} universes"):
            ch.light_universes([nominal] * n)
        with pytest.raises(lib.LdsimError, match=rf"ldsim error -1: light universes: n = {n} universes, must lie in \[1, 64\]"):
            _raw_call(ch, LU.pack([nominal] * max(n, 1)), n)
    # each invalid field, by universe and name
    bad = dict(photon_scale=(0.0, -1.0, float("nan"), float("inf")), singlet_fraction=(-0.01, 1.01, float("nan")),
               tau_s=(0.0, -1.0, float("inf")), tau_t=(0.0, float("nan")), gain_scale=(0.0, float("nan"), float("inf")),
               response_time=(0.0, -0.1, float("nan")), oscillation_period=(0.0, float("inf")))
    assert set(bad) == set(LU.C_FIELDS)
    for f, values in bad.items():
        for x in values:
            with pytest.raises(ValueError, match=f"universe 2: {f} = "):
                ch.light_universes([nominal, nominal, dict(nominal, **{f: x})])
            with pytest.raises(lib.LdsimError, match=f"ldsim error -1: light universes: universe 2: {f} = "):
                _raw_call(ch, LU.pack([nominal, nominal, dict(nominal, **{f: x})]), 3)
    assert ch.download_light_universe(1).tobytes() == kept               # every refusal left the earlier result in place
    # fluctuations need keyed streams; without them the deterministic stages run
    ch.seed_rng(5, 1024)
    with pytest.raises(lib.LdsimError, match="ldsim error -4: light universes: fluctuations need keyed streams"):
        ch.light_universes(vs, fluctuate=True)
    assert ch.download_light_universe(1).tobytes() == kept
    ch.light_universes(vs, fluctuate=False, keep_stages=True)
    sc, di, rp = ch.download_light_universe(1, stages=True)
    assert sc.tobytes() == di.tobytes() and rp.tobytes() != kept
    # no resident photon sum: a fresh context
    lib.destroy_context()
    H.load_cfg("module0")
    ch2 = ChargeChain()
    with pytest.raises(lib.LdsimError, match="ldsim error -4: light universes: no resident photon sum"):
        _raw_call(ch2, LU.pack([LU.nominal()]), 1, fluctuate=0)
    with pytest.raises(lib.LdsimError, match="no resident light universes"):
        lib.check(lib.load().ldsim_dev_light_universe_download(ch2.ctx, C.c_int32(0), None, None, None))


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_light_universes_gpu", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _same(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and all(
        np.ascontiguousarray(x if f is None else x[f]).tobytes() == np.ascontiguousarray(y if f is None else y[f]).tobytes()
        for f in (x.dtype.names or [None]))


def test_driver_writes_the_universes(tmp_path, monkeypatch, capsys):
    """simulate_pixels.py --light_universes with [nominal, TAU_T x 0.8] on a two-event module0 input: the nominal universe's rows
    of light_universe_wvfm / light_universe_trig are light_wvfm / light_trig of the same file, which the option leaves as it
    was; the varied universe's rows are light_wvfm / light_trig of a second run under the varied configuration"""
    cli = _cli()
    H.load_cfg("module0")
    tau_t = consts.light.TAU_T * 0.8
    seg = synth.make_segments(60, seed=10, segs_per_event=30)
    np.save(tmp_path / "in.npy", seg)
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    np.savez(tmp_path / "lut.npz", arr=synth.make_lut((14, 26, 8), 48, 40, 3))
    np.save(tmp_path / "noise.npy", _noise_spectrum())
    json.dump([{"name": "nominal"}, {"name": "fast triplet", "TAU_T": tau_t}], open(tmp_path / "u.json", "w"))
    common = dict(input_filename=str(tmp_path / "in.npy"), config="module0", rand_seed=7, rng="keyed", light_simulated=True,
                  response_file=str(tmp_path / "resp.npy"), light_lut_filename=str(tmp_path / "lut.npz"),
                  light_det_noise_filename=str(tmp_path / "noise.npy"))

    def run(name, **kw):
        cli.run_simulation(output_filename=str(tmp_path / name), **common, **kw)
        with np.load(tmp_path / name) as f:
            return {k: f[k] for k in f.files}, capsys.readouterr().out

    try:
        plain, _ = run("plain.npz")
        uni, log = run("uni.npz", light_universes=str(tmp_path / "u.json"))
        load = consts.load_snapshot

        def patched(*a, **kw):
            load(*a, **kw)
            consts.light.TAU_T = tau_t

        monkeypatch.setattr(consts, "load_snapshot", patched)
        varied, _ = run("varied.npz")
        monkeypatch.setattr(consts, "load_snapshot", load)
    finally:
        H.load_cfg("module0")
    assert "Light universes:" in log and "--light_universes" in log
    new = {"light_universes", "light_universe_trig", "light_universe_wvfm"}
    assert set(uni) == set(plain) | new
    for k in plain:                                       # the option changes nothing else of the file (field by field: padding)
        assert _same(uni[k], plain[k]), k
    rows = uni["light_universes"]
    assert rows.dtype == LU.FILE_UNIVERSE and rows["name"].tolist() == [b"nominal", b"fast triplet"]
    assert rows["tau_t"].tolist() == [consts.light.TAU_T, tau_t] and rows["photon_scale"].tolist() == [1.0, 1.0]
    trig, wv = uni["light_universe_trig"], uni["light_universe_wvfm"]
    assert len(trig) == len(wv) and set(trig["universe"].tolist()) == {0, 1}
    u0, u1 = trig["universe"] == 0, trig["universe"] == 1
    assert wv[u0].tobytes() == uni["light_wvfm"].tobytes() and len(uni["light_wvfm"]) >= 2
    assert np.array_equal(trig["op_channel"][u0], uni["light_trig"]["op_channel"])
    assert wv[u1].tobytes() == varied["light_wvfm"].tobytes()
    assert np.array_equal(trig["op_channel"][u1], varied["light_trig"]["op_channel"])
    assert wv[u1].shape != wv[u0].shape or wv[u1].tobytes() != wv[u0].tobytes()
    # trigger times: light_trig's ts_s is the universe's start time + tick, in seconds, behind the event's own time
    rel = (trig["start_time"][u0] + trig["trigger_idx"][u0] * consts.light.LIGHT_TICK_SIZE) * consts.units.mus / consts.units.s
    same_event = np.diff(trig["event_id"][u0].astype(int)) == 0
    assert np.all(np.abs(np.diff(uni["light_trig"]["ts_s"] - rel)[same_event]) < 1e-9)
