"""
GPU: light incidence and the photon sum (csrc/kernels_light.hip: light_incidence_kernel, light_incidence4_kernel, the record
builders light_count_ordered_kernel / light_fill_ordered_kernel / light_emit_wave_kernel, light_replay_wave_kernel,
sum_light_scatter_kernel, sum_light_list_kernel) against the reference's own calculate_light_incidence, get_nticks and
sum_light_signals where these kernels are delicate.

tests/golden/light_edge_<case>.npz (oracle/gen_golden.py gen_light_edges) hold the inputs in the form each stage reads them, the
overridden constants and what the reference made of them; every fixture counts, by the reference's expressions on its inputs,
how often it met what it is there for (`reach_*`, checked on loading).  tests/test_oracle_golden.py pins the oracle to the same
files.

Every comparison is bit for bit (NaN where the reference has NaN, -0.0 where it has -0.0):
  * incidence: kernel and reference do the same f64 operations in the same order (the library is built with -ffp-contract=off)
    and round once to f4;
  * photon sum: every value of these fixtures is dyadic -- visibilities, time profiles and efficiencies powers of two, photon
    counts small integers, times whole nanoseconds -- so the f4 product, every f4 running sum and every f8 slot sum are exact
    (the generator asserts that no sum leaves 24 bits) and the order of the additions, which differs between the record replay,
    the f64 tick tiles of the kernels without truth slots and the reference's loop, cannot show.
"""
import numpy as np
import pytest

import helpers as H
from larndsim_amd import consts, lib, light_sim, lightLUT
from larndsim_amd.chain import ChargeChain

pytestmark = pytest.mark.gpu


def _stage_incidence(r, lut, n_out, scalar):
    """the stage call into arrays that hold the sentinels, one channel per lane (scalar = 1) or the launcher's own choice"""
    s_nph, s_t0, s_vox = H.LIGHT_EDGE_SENTINELS
    inc = np.zeros((len(r), n_out), dtype=H.LIGHT_EDGE_INC_DTYPE)
    inc['n_photons_det'], inc['t0_det'] = s_nph, s_t0
    vox = np.full((len(r), 3), s_vox, dtype='i4')
    lib.context()
    try:
        lib.set_option("light_incidence_scalar", scalar)
        lightLUT.calculate_light_incidence[1, 256](r, lut, inc, vox)
    finally:
        lib.set_option("light_incidence_scalar", 0)
    return inc, vox


@pytest.mark.parametrize("name", H.LIGHT_EDGE_INCIDENCE_CASES)
def test_incidence_vs_reference(name):
    """calculate_light_incidence on both borders of every axis, 1.9e-2 either side of them (inside get_voxel's margin), a voxel
    and a half beyond either end (clamped), every interior voxel face and its two neighbouring doubles, in even and odd TPCs
    (x measured from x_max in the odd ones) of module0 and 2x2, for LUTs of 1x1x1, 3x5x2 and 14x26x8 voxels; a LUT of 6
    detectors (lut_index = o % 6: the one-channel kernel) and its twin of 48; one module's slice of the channels; trigger mode
    1; efficiencies that are zero, negative and NaN (the launcher's fall-back to the one-channel kernel: NaN and -0.0 in the
    channels of other TPCs); records and voxels without light.  Stage call in both kernel forms: rows of segments outside
    every TPC, and t0_det in trigger mode 1, keep the sentinels.  Resident leg: the same values, those rows zero."""
    try:
        g = H.load_light_edge_case(name)
        trig0 = consts.light.LIGHT_TRIG_MODE == 0
        for k in range(int(g["n_runs"])):
            pre = f"r{k}_"
            r, lut, n_out = H.light_edge_records(g, pre), H.light_edge_lut(g, pre), int(g[pre + "n_out"])
            for scalar in (0, 1):
                inc, vox = _stage_incidence(r, lut, n_out, scalar)
                what = f"{name} run {k} scalar {scalar}"
                assert np.array_equal(vox, g[pre + "voxel"]), what
                H.assert_same_floats(inc['n_photons_det'], g[pre + "n_photons_det"], what + " n_photons_det")
                H.assert_same_floats(inc['t0_det'], g[pre + "t0_det"], what + " t0_det")
                n_ticks, start = light_sim.get_nticks(inc)
                assert n_ticks == int(g[pre + "n_ticks"]) and float(start) == float(g[pre + "start_time"]), what
            ch = ChargeChain()
            ch.upload(r, np.zeros(len(r), dtype=np.int32))
            ch.light_incidence(lut, n_out=n_out)
            rinc, rvox = ch.download_light_incidence()
            inside = r["pixel_plane"] != consts.detector.DEFAULT_PLANE_INDEX
            what = f"{name} run {k} resident"
            assert np.array_equal(rvox[inside], g[pre + "voxel"][inside]) and (rvox[~inside] == 0).all(), what
            H.assert_same_floats(rinc['n_photons_det'][inside], g[pre + "n_photons_det"][inside], what + " n_photons_det")
            assert not rinc['n_photons_det'][~inside].any() and not np.signbit(rinc['n_photons_det'][~inside]).any(), what
            if trig0:
                H.assert_same_floats(rinc['t0_det'][inside], g[pre + "t0_det"][inside], what + " t0_det")
                assert not rinc['t0_det'][~inside].any(), what
        if name == "trig_mode_1" or name == "faces_2x2":
            assert not trig0 and (g["r0_t0_det"] == H.LIGHT_EDGE_SENTINELS[1]).all()
        if name == "efficiency_fallback":
            assert np.isnan(g["r0_n_photons_det"]).any() and (np.signbit(g["r0_n_photons_det"]) & (g["r0_n_photons_det"] == 0)).any()
    finally:
        H.load_cfg("module0")


def _stage_sum(g, k, r, M):
    """run k of a photon-sum fixture through the stage call with M truth slots (the fixture's count, or 0: the kernels without
    slots), into the arrays the fixture says the sum adds into"""
    pre = f"r{k}_"
    out, tid, tph = H.light_edge_sum_init(g, k)
    if not M:
        tid, tph = tid[..., :0], tph[..., :0]
    inc = np.zeros(g["n_photons_det"].shape, dtype=H.LIGHT_EDGE_INC_DTYPE)
    inc['n_photons_det'], inc['t0_det'] = g["n_photons_det"], g["t0_det"]
    light_sim.sum_light_signals[1, 64](r, g["voxel"], g["track_id"], inc, g["op_channel"], H.light_edge_lut(g),
                                       float(g[pre + "start_time"]), out, tid, tph, g["sorted_indices"], int(g["n_prof"]))
    return out, tid, tph


@pytest.mark.parametrize("name", H.LIGHT_EDGE_SUM_CASES)
def test_photon_sum_vs_reference(name):
    """sum_light_signals on arrival times that lie on the tick grid (t0 = k / 1000 in f64 from start_time = -1.0: most arrivals
    in no tick, many in two -- the reference's behaviour, reproduced), from start times get_nticks gives and others, without
    smearing (t0_avg in whole ns, one beyond the profile length: dropped by the pre-filter), at the ends of the axis and on axes
    of two ticks and of one, and under the truth-slot rules (segments sharing a track, more tracks than slots, id -1 taken over,
    photons equal to MC_TRUTH_THRESHOLD and a step above, a visiting order that is not descending, sums and slots that hold
    something already).  Stage call with the fixture's slots (record replay) and without (f64 tick tiles: sums only); where the
    fixture's start time and visiting order are the resident leg's own, ChargeChain.sum_light with and without slots too."""
    try:
        g = H.load_light_edge_case(name)
        r, lut = H.light_edge_records(g), H.light_edge_lut(g)
        n = len(r)
        for k in range(int(g["n_runs"])):
            pre = f"r{k}_"
            M = int(g[pre + "max_truth"])
            assert M > 0 and g[pre + "light_sample_inc"].sum() > 0 and (g[pre + "true_id"] != -1).any()
            out, tid, tph = _stage_sum(g, k, r, M)
            what = f"{name} run {k} stage call"
            H.assert_same_floats(out, g[pre + "light_sample_inc"], what + " sum")
            assert np.array_equal(tid, g[pre + "true_id"]), what
            H.assert_same_floats(tph, g[pre + "true_photons"], what + " truth photons")
            out0, _, _ = _stage_sum(g, k, r, 0)
            H.assert_same_floats(out0, g[pre + "light_sample_inc"], f"{name} run {k} stage call without slots")
        assert int(g["resident"]) == (name in ("grid_smear", "grid_no_smear"))
        if int(g["resident"]):
            T, M = int(g["r0_n_ticks"]), int(g["r0_max_truth"])
            opc = g["op_channel"]
            ch = ChargeChain()
            ch.upload(r, np.zeros(n, dtype=np.int32))
            ch.light_incidence(lut)
            rinc, rvox = ch.download_light_incidence()
            assert np.array_equal(rvox, g["voxel"])
            H.assert_same_floats(rinc['n_photons_det'], g["n_photons_det"], name + " resident n_photons_det")
            H.assert_same_floats(rinc['t0_det'], g["t0_det"], name + " resident t0_det")
            n_ticks, t_start = ch.sum_light(0, n, opc, g["track_id"], max_truth=M, max_ticks=T)
            assert n_ticks == T and float(t_start) == float(g["r0_start_time"]) == float(g["own_start_time"])
            assert int(g["own_n_ticks"]) >= T
            out, tid, tph = ch.download_light()
            H.assert_same_floats(out, g["r0_light_sample_inc"], name + " resident sum")
            assert np.array_equal(tid, g["r0_true_id"]), name
            H.assert_same_floats(tph, g["r0_true_photons"], name + " resident truth photons")
            ch.sum_light(0, n, opc, max_truth=0, max_ticks=T)
            out0, _, _ = ch.download_light()
            H.assert_same_floats(out0, g["r0_light_sample_inc"], name + " resident sum without slots")
            # and with slots again after it: the arrays start clean
            ch.sum_light(0, n, opc, g["track_id"], max_truth=M, max_ticks=T)
            out, tid, tph = ch.download_light()
            H.assert_same_floats(out, g["r0_light_sample_inc"], name + " resident sum, second")
            assert np.array_equal(tid, g["r0_true_id"]), name
            H.assert_same_floats(tph, g["r0_true_photons"], name + " resident truth photons, second")
    finally:
        H.load_cfg("module0")
