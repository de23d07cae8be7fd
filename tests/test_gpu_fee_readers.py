"""The passes that read a chain launch afterwards -- pixel truth, pixel waveforms, FEE and charge universes -- read its FEE set-up
record through one reader (csrc/fee_reader.h).  Their own tests pin each of them to the oracle or to a fresh launch; this one ties
them to each other on one small launch, under both layouts of the record's headers."""
import numpy as np
import pytest

import helpers as H
from larndsim_amd import batching, consts, lib, synth
from larndsim_amd import charge_universes as CU
from larndsim_amd import fee_universes as FU
from larndsim_amd.chain import ChargeChain

pytestmark = pytest.mark.gpu

SEED, SIZES, M = 31, (25, 35), 4      # test_gpu_pixel_truth.py's synthetic module0 segments, in two batches; MAX_TRACKS_PER_PIXEL


def _segments(n):
    seg = synth.make_segments(n, seed=SEED, segs_per_event=n, spill=bool(consts.sim.IS_SPILL_SIM))
    batching.swap_coordinates(seg)
    return seg


@pytest.mark.parametrize("one_class", (0, 1))
def test_the_readers_agree_on_one_launch(one_class):
    """60 segments in two batches at MAX_TRACKS_PER_PIXEL = 4, the record as two lists and as headers [U]: the dense pixel waveforms
    are float32 of the universes' f64 S bit for bit (plain and with the nominal charge weights, all exactly 1.0), and pixel truth's
    slots are track_pixel_map's"""
    H.load_cfg("module0")
    assert not consts.sim.IS_SPILL_SIM
    consts.sim.MAX_TRACKS_PER_PIXEL = M
    try:
        lib.set_option("fee_one_class", one_class)
        seg = _segments(sum(SIZES))
        bid = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int32)
        ch = ChargeChain(synth.make_response("survey"))
        ch.upload(seg.copy(), bid)
        ch.quench_drift()
        st = ch.run(want_fractions=False)
        out = ch.download()
        tpm = out["track_pixel_map"]
        U, n_slots = int(st.n_unique), (tpm >= 0).sum(axis=1)
        S32 = ch.pixel_waveforms(dense=True)
        truth, rows = ch.pixel_truth(dense=True), ch.pixel_truth(0.0)
        ch.fee_universes([FU.nominal()])
        S_plain = ch.universe_waveforms(0)
        u = ch.universes(charge=[CU.nominal(CU.BIRKS)])[0]
        S_unit = ch.universe_waveforms(0)
    finally:
        lib.set_option("fee_one_class", 0)
        H.load_cfg("module0")
    # the launch holds what the readers can differ on: a pixel with more pairs than slots, one with free slots, and a pixel whose
    # signal lies in more than one 64-tick word
    assert tpm.shape == (U, M) and sorted(set(out["batch"].tolist())) == [0, 1]
    assert st.n_overflow > 0 and (n_slots == M).any()
    assert (n_slots < M).any() and (n_slots > 0).all()
    assert max(len(set(np.flatnonzero(r) // 64)) for r in S32 != 0) > 1
    # waveforms against the universes' sum
    assert (u["weights"] == 1.0).all() and u["n_unweightable"] == 0
    assert S32.dtype == np.float32 and S_plain.dtype == np.float64 and S_plain.shape == S32.shape == S_unit.shape
    assert S_plain.tobytes() == S_unit.tobytes()
    assert S32.tobytes() == S_plain.astype(np.float32).tobytes()
    # pixel truth against the launch's map
    assert ((tpm >= 0) == (np.arange(M) < n_slots[:, None])).all()          # (a pixel's slots come first)
    assert (truth["q_track"][tpm < 0] == 0).all() and (truth["q_track"][tpm >= 0] != 0).any()
    px = rows["pixels"]
    assert np.array_equal(px["row"], np.arange(U)) and np.array_equal(px["n_tracks"], n_slots)
    assert np.array_equal(rows["tracks"]["segment"], tpm[tpm >= 0])
