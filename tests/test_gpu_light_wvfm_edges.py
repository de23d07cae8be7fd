"""
GPU: the second half of the light chain (csrc/light_wvfm.hip: light_trig_mask_kernel + the host trigger scan,
light_noise_spec_kernel, light_idft_kernel, light_sample_kernel, light_digitize_kernel) against the reference's own
get_triggers, gen_light_detector_noise and sim_triggers / digitize_signal at constants no shipped configuration has.

tests/golden/light_wvfm_edge_<case>.npz (oracle/gen_golden.py gen_light_wvfm_edges) hold the inputs, the overridden constants
and what the reference made of them; every fixture counts how often its run took the branch it is there for (`reach_*`,
checked on loading).  tests/test_oracle_golden.py pins the oracle to the same files.  Trigger ticks and channels, digitised
values and truth ids are compared exactly (the library is built with -ffp-contract=off: the lerp is bit-comparable), noise
exactly too (the generator kept every value it rounds >= 1e-6 LSB from a tie), truth photons to rtol 1e-15.
"""
import numpy as np
import pytest

import helpers as H
from larndsim_amd import consts, lib, light_sim
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _hip_sim(sig, sop, tid, tph, trig, top, ns, tab, ph_sig, ph_mis):
    return light_sim.sim_triggers(None, None, sig, sop, tid, tph, trig, top, ns, tab, phases_signal=ph_sig, phases_missing=ph_mis)


def _hip_noise(shape, spectrum, phases):
    return light_sim.gen_light_detector_noise(shape, spectrum, phases=phases)


@pytest.mark.parametrize("name", H.LIGHT_WVFM_EDGE_TRIGGER_CASES)
def test_triggers_vs_reference(name):
    """light_sim.get_triggers: the straight-sum path of the block mean (sample factor < 8), 8, 13 and the array bound 128,
    ratios 2.5 and 3.5 rounded half to even, tick 0.0007, the all-padding block, zero padding inside the last block's mean,
    `<` against a mean equal to the threshold and one ulp beside it, the f4 row-order group sum, the reference's re-slicing
    at a third trigger, a trigger on the last tick, and 64-row groups that span two modules."""
    try:
        g = H.load_light_wvfm_edge_case(name)
        sf = int(g["sample_factor"])
        assert round(consts.light.LIGHT_DIGIT_SAMPLE_SPACING / consts.light.LIGHT_TICK_SIZE) == sf
        n_blocks = (g["signal"].shape[1] + sf - g["signal"].shape[1] % sf) // sf
        if name == "trig_sf1":
            assert n_blocks > 128 and n_blocks % 64          # more than two workgroups of 64 blocks, the last one ragged
        if name == "trig_sf7_allpad":
            assert n_blocks * sf == g["signal"].shape[1] + sf
        H.assert_light_wvfm_edge_triggers(g, light_sim.get_triggers)
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("ratio", [0.4, 129.0])
def test_sample_factor_out_of_range_is_refused(ratio):
    """A spacing ratio that rounds to 0 or to 129 (the mask kernel's array holds 128 ticks) raises; the context works
    afterwards."""
    try:
        g = H.load_light_wvfm_edge_case("trig_sf8")
        good = consts.light.LIGHT_DIGIT_SAMPLE_SPACING
        consts.light.LIGHT_DIGIT_SAMPLE_SPACING = ratio * consts.light.LIGHT_TICK_SIZE
        assert round(consts.light.LIGHT_DIGIT_SAMPLE_SPACING / consts.light.LIGHT_TICK_SIZE) in (0, 129)
        with pytest.raises(lib.LdsimError, match="must round to 1..128"):
            light_sim.get_triggers(g["signal"], g["group_threshold"][0], g["op_channel"], 0)
        consts.light.LIGHT_DIGIT_SAMPLE_SPACING = good
        H.assert_light_wvfm_edge_triggers(g, light_sim.get_triggers)
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("name", H.LIGHT_WVFM_EDGE_NOISE_CASES)
def test_noise_vs_reference(name):
    """light_sim.gen_light_detector_noise with given phases: transforms of 2, 3, 4, 16 and 17 samples (every desired
    frequency a table frequency for 2, 4, 16: the dxp == 0 branch, the last table point included), 64 samples against a
    table that ends below most desired frequencies, and 1026 / 1027 / 1028 samples (512 and 513 terms: one full LDS chunk,
    and one term more; the odd size gets a zero appended)."""
    try:
        g = H.load_light_wvfm_edge_case(name)
        for n in g["n_samples"]:
            m = int(n) // 2 + 1
            if name == "noise_tiny" and n in (2, 4, 16):
                assert int(g[f"exact_freq_{n}"]) == m
            if name == "noise_beyond_table":
                assert int(g[f"beyond_table_{n}"]) > m // 2
        if name == "noise_chunk":
            assert int(g["reach_terms_1026"]) == 512 and int(g["reach_terms_1028"]) == 513
        H.assert_light_wvfm_edge_noise(g, _hip_noise)
    finally:
        H.load_cfg("module0")


@pytest.mark.parametrize("name", H.LIGHT_WVFM_EDGE_DIGIT_CASES)
def test_digitiser_vs_reference(name):
    """light_sim.sim_triggers: interp's lerp (mode 2) and zero branches (mode 0) in light_digitize_kernel, the truth photons
    interpolated at frac != 0 with the next tick's slots searched, the operation order of the sample tick at tick 0.0007, an
    odd padded length under noise, and the typing switch of `v1 - v0`: with option numba_f32 an f4 signal that the reference
    neither pads nor extends by missing channels keeps Numba's f4 difference (pinned by the oracle), any other is f8."""
    try:
        g = H.load_light_wvfm_edge_case(name)
        if name == "lerp_2p5":
            for k in ("same_slot", "other_slot", "no_match", "below_threshold", "minus1_end", "all_full", "frac_samples"):
                assert int(g["reach_" + k]) > 0, k
        if name == "lerp_order":
            assert int(g["reach_off_grid"]) > 0
        if name == "beyond_end":
            assert int(g["reach_zero_past_end"]) > 0 and int(g["reach_zero_last_tick"]) > 0
        H.assert_light_wvfm_edge_digit(g, _hip_sim)
        if name in ("all_rows_f4", "missing_rows_f4"):
            no_id, no_ph = np.zeros(g["signal"].shape + (0,), dtype='i8'), np.zeros(g["signal"].shape + (0,))
            args = (g["signal"], g["signal_op_channel"], no_id, no_ph, g["trigger_sets"][0], np.stack([np.arange(96, dtype='i4')] * 2),
                    int(g["digit_samples"]), np.zeros((96, 9)), None, None)
            lib.set_option("numba_f32", 1)
            O.lib().o_set_numba_f32(1)
            try:
                typed = _hip_sim(*args)[0]
                oracle_typed = _oracle_sim(*args)[0]
            finally:
                O.lib().o_set_numba_f32(0)
                lib.set_option("numba_f32", 0)
            differ = int((typed != g["wvfm_0"]).sum())
            print(name, "option numba_f32: differs from the all-f64 result in", differ, "of", typed.size, "values")
            assert np.array_equal(typed, oracle_typed)
            if name == "missing_rows_f4":
                assert int(g["reach_missing_rows"]) == 84 and differ == 0       # an f8 array in the reference: both modes agree
            else:
                assert differ > 0                                               # the two modes are two results
    finally:
        H.load_cfg("module0")


def _oracle_sim(sig, sop, tid, tph, trig, top, ns, tab, ph_sig, ph_mis):
    return O.sim_triggers(sig, sop, tid, tph, trig, top, ns, tab, phases_signal=ph_sig, phases_missing=ph_mis)
