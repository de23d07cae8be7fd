"""
GPU: gcorr_fused_kernel -- a pair of two node batches whose second stores four or eight rows (17 .. 24 quadrature nodes), both
batches in one pass over the cell rows (kernels_gcorr.hip) -- against the f64 oracle at every tick and against the two-pass form
of the launch over all pairs (debug_gform 131072 turns the fused launches off; 4096, the 16-node product everywhere, does so too).

One hand-placed set of 16 segments (module0: TIME_SAMPLING = RESPONSE_SAMPLING, M = 1, the only M the fused launches serve).
The node rule of pair_setup_kernel is NQ = ceil(3.4 + 1.38 r), r = the length of the part of the segment that can reach the
pixel, in Gaussian widths along the segment: the lengths below are chosen from it so that whole segments (close to the anode the
cloud is far narrower than a pixel's reach: nothing is clipped) get 17, 20 (second batch of four rows), 21, 24 (eight rows),
26 (twelve: not eligible) and at most 16 nodes (one batch).  The census of the launch tells what the pairs really were.

What the two forms may differ by: the fused form adds the same products in another order (the second batch joins the P step
before the tick sum), f64 sums ahead of ONE rounding to the f4 the rows are stored in -- two f4 ulps of the waveform's peak,
2^-22 peak, bound the difference.

Which pairs the fused kernels took, and what the two batches of a pair list, comes from ``detsim.gform_fused`` (the marks
gbig_list_kernel left, checked by the library against the counts the kernels were launched over, and the two cell lists of every
two-batch pair read back from the launch's records): the masks below are the launch's own, not a re-derivation, and the test of
the merged cell list asserts on the lists themselves -- a pruned weight is 1e-10 of the peak, below every tolerance here.
"""
import functools

import numpy as np
import pytest

import helpers as H
from larndsim_amd import batching, consts, detsim, lib, synth
from larndsim_amd.abi import GFORM_CENSUS_SLOTS
from larndsim_amd.chain import ChargeChain
from oracle import oracle as O
from test_gpu_parity import _reset_current_options, _tracks_current_on, _two_event_set

pytestmark = pytest.mark.gpu

CFG = "module0"
OFF = 131072                                     # debug_gform: no fused launches
KINDS = {"survey": 128, "narrow": 128, "trimmed": 256, "dense": 512}      # tick tile the launch must choose
QN0, QSLOPE = 3.4, 1.38                          # pair_setup_kernel's node rule at the default accuracy

# (r, d): r Gaussian widths long at its midpoint, d cm from the anode; the node count of the whole segment by the rule
PLAN = [(9.6, 0.12), (10.4, 0.12), (11.2, 0.12), (11.9, 0.12), (12.4, 0.12), (14.6, 0.12), (16.0, 0.12), (5.0, 0.12),
        (9.6, 0.6), (11.9, 0.6), (12.4, 0.6), (7.0, 0.6), (10.4, 15.0), (13.0, 15.0), (11.2, 29.8), (12.4, 29.8)]
SHORT_PLAN = [(2.0, 0.12), (5.0, 0.12), (8.0, 0.6), (8.5, 0.12)]          # at most 16 nodes: no eligible pair
# the merged cell list: 20 and 24 nodes on segments several response bins long, where the first nodes and the last ones lie over
# different bins (the second batch of a 24-node rule starts 0.72 of the way along, five widths past the first batch's last node)
CELLS_PLAN = [(11.9, 2.0), (14.6, 2.0), (11.9, 6.0), (14.6, 6.0), (11.5, 1.0), (14.0, 1.0), (11.9, 0.3), (14.6, 0.3)]
PLANS = {"main": PLAN, "short": SHORT_PLAN, "cells": CELLS_PLAN}


def rule_nodes(r):
    return int(np.ceil(QN0 + QSLOPE * r))


def make_response(kind):
    """`survey` / `dense`: the project's synthetic tables; `trimmed` (~140 ticks of support, eleven ticks under the top edge of
    the time window) and `narrow` (~40 ticks, four ticks under it): built here, so that the window-edge columns carry weight."""
    if kind in ("survey", "dense"):
        return H.response_for(kind)
    det = consts.detector
    dt = det.RESPONSE_SAMPLING
    I, J, K = 45, 45, 1950
    i = np.arange(I, dtype=np.float64)[:, None, None]
    j = np.arange(J, dtype=np.float64)[None, :, None]
    k = np.arange(K, dtype=np.float64)[None, None, :]
    top = np.floor(det.TIME_WINDOW / dt)
    centre, s1, s2, lag = (top - 11.0, 6.0, 11.0, 25.0) if kind == "trimmed" else (top - 4.0, 2.0, 3.5, 7.0)
    g = np.exp(-0.5 * ((k - centre) / s1) ** 2)
    g = g / (g.sum() * dt)
    g2 = np.exp(-0.5 * ((k - (centre - lag)) / s2) ** 2)
    g2 = g2 / (g2.sum() * dt)
    spatial = np.exp(-(i * i + 2.0 * j * j) / 60.0)
    skew = (i + 2.0 * j) / (I + 2.0 * J)
    return spatial * (g * (1.0 - 0.3 * skew) - 0.45 * skew * g2)


def build_segments(plan):
    H.load_cfg(CFG)
    det = consts.detector
    B = det.TPC_BORDERS[0]
    sgn = np.sign(B[2][1] - B[2][0])
    seg = synth.make_segments(len(plan), seed=37, segs_per_event=len(plan))
    batching.swap_coordinates(seg)
    x0, y0 = B[0][0] + 0.29 * (B[0][1] - B[0][0]), B[1][0] + 0.41 * (B[1][1] - B[1][0])
    for k, (rr, d) in enumerate(plan):
        a = np.array([x0 + 4.3 * (k % 4) + 0.017 * k, y0 + 5.1 * (k // 4) + 0.023 * k, B[2][0] + sgn * d])
        ang, tilt = 0.5 + 0.41 * k, 0.0998
        L = rr * np.sqrt(2 * det.TRAN_DIFF * d / det.V_DRIFT)
        for _ in range(4):                                   # rr widths of the cloud at the segment's midpoint
            L = rr * np.sqrt(2 * det.TRAN_DIFF * (d + 0.5 * tilt * L) / det.V_DRIFT)
        b = a + L * np.array([np.cos(ang) * np.sqrt(1 - tilt * tilt), np.sin(ang) * np.sqrt(1 - tilt * tilt), sgn * tilt])
        for i, ax in enumerate("xyz"):
            seg[ax + "_start"][k] = a[i]; seg[ax + "_end"][k] = b[i]
            seg[ax][k] = 0.5 * (np.float32(a[i]).astype(np.float64) + np.float32(b[i]))
        seg["dx"][k] = max(float(np.linalg.norm(b - a)), 1e-4); seg["dEdx"][k] = 2.1; seg["dE"][k] = 2.1 * seg["dx"][k]
        for f in ("t0", "t0_start", "t0_end"):
            seg[f][k] = 9.0 if d > 29.0 else 0.0             # (the last two: the drift window cut by the end of the time window)
    return seg


@functools.lru_cache(maxsize=None)
def _inputs(which="main"):
    r = H.quench_drift(O, build_segments(PLANS[which]))
    nmax = O.max_pixels(r)
    _, neigh, _, _ = O.get_pixels(r, nmax, 3 * nmax + 6, 1)
    _, T = O.time_intervals(r)
    return r, np.ascontiguousarray(neigh), int(T)


@functools.lru_cache(maxsize=None)
def _case(kind, which="main"):
    """(records, pixels, T, response, oracle waveforms): computed once, never written to."""
    r, neigh, T = _inputs(which)
    H.load_cfg(CFG)
    resp = make_response(kind)
    ref = O.tracks_current(r, neigh, T, resp)
    assert np.isfinite(ref).all()
    for a in (r, neigh, resp, ref):
        a.setflags(write=False)
    return r, neigh, T, resp, ref


def _bit(slots, name):
    return ((slots >> GFORM_CENSUS_SLOTS.index(name)) & 1).astype(bool)


def _launch(r, neigh, T, resp, **opts):
    """(waveforms, counters, census, per-pair census slots, fused report) of one launch."""
    H.load_cfg(CFG)
    sig, st = _tracks_current_on("gform", neigh, r, resp, T, **opts)
    c = detsim.gform_census(per_pair=True, n_pairs=neigh.size)
    slots = c.pop("pair_slots").reshape(neigh.shape)
    f = detsim.gform_fused(neigh.size)
    for k in ("mark", "only0", "only1", "both"):
        f[k] = f[k].reshape(neigh.shape)
    # the marks and the launched counts agree (the library refuses the report otherwise), and only pairs the census calls
    # two-batch, first-class, with a second batch of 4 (8) rows are marked 1 (2)
    assert f["launched"] == (int((f["mark"] == 1).sum()), int((f["mark"] == 2).sum()))
    for na, rows in ((1, "rows4"), (2, "rows8")):
        assert not ((f["mark"] == na) & ~(_bit(slots, "emitted") & _bit(slots, "nb2") & _bit(slots, rows) & _bit(slots, "cls0"))).any()
    return sig, st, c, slots, f


@functools.lru_cache(maxsize=None)
def _on_off(kind, pad_kb=0, which="main"):
    r, neigh, T, resp, ref = _case(kind, which)
    extra = dict(debug_lds_pad_kb=pad_kb) if pad_kb else {}
    on = _launch(r, neigh, T, resp, **extra)
    off = _launch(r, neigh, T, resp, debug_gform=OFF, **extra)
    assert off[4]["launched"] == (0, 0) and not off[4]["mark"].any()
    return on, off


def _check(kind, pad_kb=0, which="main"):
    """Fused launches on: every tick of every pair against the oracle (project tolerance) and against the two-pass form.
    Returns the census slots, the live pairs gcorr_fused_kernel<1> and <2> took, and the fused report."""
    r, neigh, T, resp, ref = _case(kind, which)
    (sig, st, c, slots, f), (sig0, st0, c0, slots0, f0) = _on_off(kind, pad_kb, which)
    assert c["m"] == 1 and c["tt"] == KINDS[kind] and np.array_equal(slots, slots0)
    live = np.abs(ref).max(axis=-1) > 0
    el4, el8 = (f["mark"] == 1) & live, (f["mark"] == 2) & live
    print(f"{which} {kind} pad {pad_kb}: live {int(live.sum())}, fused launches over {f['launched']}, live of them {int(el4.sum())} + "
          f"{int(el8.sum())}, one batch {int((_bit(slots, 'nb1') & live).sum())}, rows12 "
          f"{int((_bit(slots, 'rows12') & _bit(slots, 'nb2') & live).sum())}, n_dfma {st.n_dfma} / {st0.n_dfma}, useful "
          f"{st.n_dfma_useful} / {st0.n_dfma_useful}")
    assert el4.sum() >= 3 and el8.sum() >= 1, "the set holds too few live pairs for the fused launches"
    # the path ran: fewer issued FMAs (4 x 4 x 4 products for the short batch), the same algorithmic ones
    assert st.n_dfma < st0.n_dfma and st.n_dfma_useful == st0.n_dfma_useful
    # against the oracle: the per-pair bar of tests/test_gpu_gform_classes.py
    pair_peak = np.abs(ref).max(axis=-1, keepdims=True)
    charge_scale = r["n_electrons"].astype(np.float64)[:, None, None] * np.abs(resp).max()
    main = pair_peak >= 1e-5 * charge_scale
    err = np.abs(sig.astype(np.float64) - ref)
    bad = ((err > 1e-5 * np.abs(ref) + 1e-7 * charge_scale) | (main & (err > 1e-5 * np.abs(ref) + 1e-7 * pair_peak))).any(axis=-1)
    assert not bad.any(), f"{kind}: {int(bad.sum())} pairs out of tolerance, {int((bad & (el4 | el8)).sum())} of them fused"
    # against the two-pass form: two f4 ulps of the peak; pairs outside the fused launches keep their bits
    d = np.abs(sig.astype(np.float64) - sig0.astype(np.float64))
    peak0 = np.abs(sig0.astype(np.float64)).max(axis=-1, keepdims=True)
    fused = f["mark"] != 0
    print(f"{kind}: largest |on - off| / peak over the fused pairs {float((d / np.maximum(peak0, 1e-300))[fused].max()):.3e}")
    assert (d <= 2.0 ** -22 * peak0).all()
    assert np.array_equal(sig[~fused], sig0[~fused])
    return slots, el4, el8, f


def test_plan_follows_the_node_rule():
    """The lengths of PLAN by the node rule: 17 and 20 (eligible, four rows), 21 and 24 (eight), 26 (twelve), <= 16 (one batch)."""
    nq = [rule_nodes(r) for r, _ in PLAN]
    assert {17, 20, 21, 24, 26} <= set(nq) and min(nq) <= 16
    assert all(rule_nodes(r) <= 16 for r, _ in SHORT_PLAN)
    assert {rule_nodes(r) for r, _ in CELLS_PLAN} <= set(range(17, 25))


def test_survey_table_odd_tile_pairs():
    """module0, survey table: 82 staged ticks are three tile pairs, the odd one shared by the pair's two waves by cell groups.
    The set also holds live pairs the fused launches must leave alone: one batch, and a second batch of twelve rows."""
    slots, el4, el8, f = _check("survey")
    live = np.abs(_case("survey")[4]).max(axis=-1) > 0
    assert (_bit(slots, "nb1") & live).any() and (_bit(slots, "nb2") & _bit(slots, "rows12") & live).any()


@pytest.mark.parametrize("kind", ["narrow", "trimmed"])
def test_window_edge_columns(kind):
    """A response under the top edge of the time window: fused pairs carry window-edge columns (emask)."""
    slots, el4, el8, f = _check(kind)
    edge = _bit(slots, "emask1") | _bit(slots, "emask2")
    assert (el4 & edge).sum() >= 3 and (el8 & edge).any()


def test_dense_table_z_from_the_record():
    """TT = 512, several tick tiles per pair; the Z table of fused pairs read from the record."""
    slots, el4, el8, f = _check("dense")
    assert (el4 & _bit(slots, "cls0_zrec")).any()


def test_z_from_the_record_on_a_smaller_budget():
    """debug_lds_pad_kb 2 on the survey table: a first class of 10 KB -- Z of most fused pairs no longer fits."""
    slots, el4, el8, f = _check("survey", pad_kb=2)
    assert ((el4 | el8) & _bit(slots, "cls0_zrec")).any()


def test_batches_that_list_different_cells():
    """The merged cell list.  The tables kernels prune the cell list per batch; the fused kernel walks the union and gives a
    cell that one batch does not list the zero column for that batch's product.  Asserted on the lists of the launch's records:
    among the live pairs each fused kernel took, at least one has a cell only the FIRST batch lists and at least one has a cell
    only the SECOND batch lists (the branch of the merge that writes a cell from the second list).  Those pairs are then among
    the ones compared, every tick, with the oracle and with the two-pass form."""
    slots, el4, el8, f = _check("survey", which="cells")
    for name, el in (("gcorr_fused_kernel<1>", el4), ("gcorr_fused_kernel<2>", el8)):
        n0, n1, nb = int((el & (f["only0"] > 0)).sum()), int((el & (f["only1"] > 0)).sum()), int((el & (f["only0"] > 0) & (f["only1"] > 0)).sum())
        print(f"{name}: {int(el.sum())} live pairs; with cells of the first batch alone {n0} (up to {int(f['only0'][el].max())} cells), of the "
              f"second alone {n1} (up to {int(f['only1'][el].max())}), of both kinds {nb}; cells in both lists up to {int(f['both'][el].max())}")
        assert n0 >= 1 and n1 >= 1, f"{name}: no live pair whose batches list different cells ({n0} / {n1})"


def test_off_switches_same_bits():
    """Three ways without fused pairs.  debug_gform 131072 (no fused launches) and 262144 (fused launches on, their lists forced
    empty: nothing is marked, nothing launched, the launch over all pairs keeps every pair) are the same bits for ALL pairs.
    4096 (the 16-node product in every launch) is off as well: the same bits for the pairs of the first class -- it also moves
    the listed classes from the 4-node-block instance to the 16-node one, whose sums take another order -- and adding 131072 to
    it changes nothing."""
    r, neigh, T, resp, ref = _case("survey")
    _, (sig0, st0, c0, slots0, f0) = _on_off("survey")
    sige, ste, ce, slotse, fe = _launch(r, neigh, T, resp, debug_gform=262144)
    assert fe["launched"] == (0, 0) and not fe["mark"].any()
    assert np.array_equal(sige, sig0) and ste.n_dfma == st0.n_dfma and ste.n_dfma_useful == st0.n_dfma_useful and ce == c0
    sig1, st1, c1, slots1, f1 = _launch(r, neigh, T, resp, debug_gform=4096)
    sig2, st2, c2, slots2, f2 = _launch(r, neigh, T, resp, debug_gform=4096 | OFF)
    assert f1["launched"] == (0, 0) and not f1["mark"].any()
    cls0 = _bit(slots0, "cls0")
    assert cls0.sum() >= 10 and np.array_equal(slots0, slots1)
    assert np.array_equal(sig0[cls0], sig1[cls0]) and np.array_equal(sig1, sig2)
    assert st1.n_dfma == st2.n_dfma and st1.n_dfma_useful == st0.n_dfma_useful


def test_no_eligible_pair_launches_nothing():
    """A set of short segments (one batch each): on and off are the same launch, and the census agrees with its lists."""
    r, neigh, T = _inputs("short")
    H.load_cfg(CFG)
    resp = make_response("survey")
    sig, st, c, slots, f = _launch(r, neigh, T, resp)
    sig0, st0, c0, slots0, f0 = _launch(r, neigh, T, resp, debug_gform=OFF)
    assert c["emitted"] >= 10 and c["nb2"] == 0 and c["nb3p"] == 0 and c == c0
    assert f["launched"] == (0, 0) and not f["mark"].any()
    assert np.array_equal(sig, sig0) and st.n_dfma == st0.n_dfma and st.n_dfma_useful == st0.n_dfma_useful


def test_through_the_chain():
    """ChargeChain.run (the kernels write a pair's window only): two small events, fused launches on against off -- the same
    hits, charges within the tolerance tests/test_gpu_parity.py::test_split_kernels_equal_monolithic uses."""
    seg, bid = _two_event_set(CFG, 41, n=400)
    ch = ChargeChain(H.response_for("survey"))
    ch.upload(seg, bid)
    ch.quench_drift()
    res, dfma = {}, {}
    try:
        for name, dbg in (("on", 0), ("off", OFF)):
            lib.set_option("debug_gform", dbg)
            st = ch.run(0, len(seg), want_fractions=True)
            res[name] = ch.download()
            dfma[name] = (st.n_dfma, st.n_dfma_useful)
    finally:
        _reset_current_options()
    a, b = res["off"], res["on"]
    assert dfma["on"][0] < dfma["off"][0] and dfma["on"][1] == dfma["off"][1]
    assert (a["adc_list"] != 0).sum() > 100
    assert np.array_equal(a["unique_pix"], b["unique_pix"]) and np.array_equal(a["track_pixel_map"], b["track_pixel_map"])
    assert np.array_equal(a["adc_list"] != 0, b["adc_list"] != 0)
    np.testing.assert_allclose(b["adc_list"], a["adc_list"], rtol=2e-8)
    assert np.array_equal(a["adc_ticks_list"], b["adc_ticks_list"])
    assert np.array_equal(a["adc_digit"], b["adc_digit"])
    np.testing.assert_allclose(b["current_fractions"], a["current_fractions"], rtol=1e-7, atol=1e-10)
