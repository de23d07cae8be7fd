"""
GPU: every kernel class of the node-separable current path (weights_mode 2: pair_setup_kernel, gtables_wave_kernel / gtables_kernel,
gcorr_kernel) against the f64 oracle at every tick, with the class named.

``gform_launch`` deals the (segment, pixel) pairs of a launch into a dozen code paths -- four instances of gcorr_kernel, three LDS
classes, tick tiles of 128 / 256 / 512, the Z table in LDS or read from the record, one or more node batches with a short last
one, three tables kernels, window-edge columns.  ``detsim.gform_census(per_pair=True)`` tells which pairs took which; every test here
compares all ticks of all pairs with ``O.tracks_current`` (pinned to the reference's source by tests/test_oracle_golden.py) under
the project's tolerance |d| <= 1e-5 |ref| + 1e-7 peak(waveform), and asserts from the census that the setting reached what it
names.  ``test_floor_*`` asserts that, over the settings of one (config, response), every slot of FLOOR_SLOTS held at least
three pairs with a non-zero oracle waveform that the named kernels (not the monolithic fallback) emitted.

One hand-placed set of 16 segments per config (module0: TIME_SAMPLING = RESPONSE_SAMPLING, M = 1; ndlar: M = 2), one oracle run
per (config, response), cached for the module.

Response tables and the tick tile the launch derives from their staged support (read from the census, asserted):
  dense    full support                                                                      TT 512
  golden   its 1/(d + 10)^2 far-field term is 1e-6 of the peak at the far end of the table, above the e^-23 trim: full
           support as well                                                                   TT 512
  trimmed  `golden` without that term (same (i, j) asymmetry, same bipolar shape in time): ~140 ticks of support     TT 256
  narrow   the same shape with time widths of 2 and 3.5 ticks, next to the top edge of the time window: ~40 ticks    TT 128

Slots no input reaches (UNREACHABLE, with the reason): the workgroup tables kernel for more than 80 X | Y bins.
"""
import functools

import numpy as np
import pytest

import helpers as H
from larndsim_amd import batching, consts, detsim, lib, synth
from oracle import oracle as O
from test_gpu_parity import _tracks_current_on

pytestmark = pytest.mark.gpu

CFGS = ["module0", "ndlar"]                       # M = 1, M = 2
RESPONSES = {"dense": 512, "golden": 512, "trimmed": 256, "narrow": 128}      # tick tile the launch must choose
# slots that every (config, response) must have filled with >= 3 compared, live pairs over its settings
FLOOR_SLOTS = ("nb1", "nb2", "nb3p", "rows4", "rows8", "rows12", "rows16", "cls0", "cls1", "cls2", "cls0_zrec", "listed_zrec",
               "nu_over_cap", "t_wave", "t_wide", "t_wg", "wg_shifts", "wg_bins", "emask_top")
# slot -> why no input reaches it (detector geometry: the kernels' own caps, G_NCOL + NJ_MAX = 88, would allow it).  The sample box of a pair (pair_geometry, detsim.py:366-414) is the chord of the segment's line
# inside the pixel's impact circle, radius `impact` = 2 max(5 sqrt(2) sigma_T, pitch / sqrt(2)), plus 4 sigma_T either side: with the
# chord at angle a to the x axis and the pixel at most `impact` from its midpoint, ncol + NJ <= (sqrt(2) impact (cos a + sin a) +
# 8 sigma_T) / RESPONSE_BIN_SIZE + 2 <= (2 impact + 8 sigma_T) / bin + 2.  sigma_T is largest at the cathode: 0.058 cm in module0
# (bound 50 bins; 48 met), 0.075 cm in ndlar (bound 74; 70 met).  So no pair has more than 80 X | Y bins, and gtables_kernel gets its
# pairs for their shifts or slices; the wide wave kernel gets pairs by their bins in ndlar, by their shifts alone in module0.
UNREACHABLE = {"wg_bins": "ncol + NJ <= (2 impact + 8 sigma_T) / bin + 2 = 50 (module0) / 74 (ndlar) at the cathode, below 81"}
SETTINGS = {
    "defaults": {},
    "qb_everywhere": dict(debug_gform=65536),
    "qb_nowhere": dict(debug_gform=4096),
    "qb_nowhere_listed": dict(debug_gform=4096, debug_lds_pad_kb=8, debug_lds_b1_kb=12),
    "small_first_class": dict(debug_lds_pad_kb=8),
    "small_first_and_second_class": dict(debug_lds_pad_kb=8, debug_lds_b1_kb=12),
    "workgroup_tables": dict(gform_wave_tables=0),
}


def make_response(kind):
    """`dense` / `golden`: the project's synthetic tables; `trimmed` / `narrow`: built here (module docstring)."""
    if kind in ("dense", "golden"):
        return H.response_for(kind)
    det = consts.detector
    dt = det.RESPONSE_SAMPLING
    I, J, K = (45, 45, 1950) if dt >= 0.1 - 1e-12 else (45, 45, 3800)
    i = np.arange(I, dtype=np.float64)[:, None, None]
    j = np.arange(J, dtype=np.float64)[None, :, None]
    k = np.arange(K, dtype=np.float64)[None, None, :]
    if kind == "trimmed":
        # golden's widths in ticks of TIME_SAMPLING, eleven of them under the top edge of the time window (module0: K - 70, where
        # `golden` has it), so that the edge columns carry weight at M = 2 as well
        M = round(det.TIME_SAMPLING / dt)
        centre, s1, s2, lag = np.floor(det.TIME_WINDOW / dt) - 11.0 * M, 6.0 * M, 11.0 * M, 25.0 * M
    else:
        # four ticks under the top edge of the time window (k = TIME_WINDOW / RESPONSE_SAMPLING), so that the edge columns carry weight
        centre, s1, s2, lag = np.floor(det.TIME_WINDOW / dt) - 4.0, 2.0, 3.5, 7.0
    g = np.exp(-0.5 * ((k - centre) / s1) ** 2)
    g = g / (g.sum() * dt)
    g2 = np.exp(-0.5 * ((k - (centre - lag)) / s2) ** 2)
    g2 = g2 / (g2.sum() * dt)
    spatial = np.exp(-(i * i + 2.0 * j * j) / 60.0)
    skew = (i + 2.0 * j) / (I + 2.0 * J)
    return spatial * (g * (1.0 - 0.3 * skew) - 0.45 * skew * g2)


# (kind, ...): "r" = r Gaussian widths long at its midpoint, d cm from the anode, shallow tilt along the drift (the length sweep of
# test_gpu_parity.py); "line" = (dx, dy, dz) from a point d cm from the anode, t0 in microseconds; "off" = leaves the pixel plane
def _plan(cfg):
    m0 = cfg == "module0"
    drift = 30.0 if m0 else 50.0
    return [("r", 2.0, 0.12), ("r", 8.0, 0.6), ("r", 10.0, 0.12), ("r", 13.0, 0.6), ("r", 16.0, 0.12), ("r", 21.0, 0.6),
            ("r", 30.0, 0.12), ("r", 60.0, 0.6),
            ("r", 8.0, 15.0),                                                        # shallow, few shifts, far from both window edges
            ("line", (0.05, 0.0, 1.9 if m0 else 1.0), 10.0, 0.0),                    # steep: more than 128 shifts
            ("line", (0.4, 0.3, 4.2 if m0 else 2.4), 12.0, 0.0),                     # steep: more than 256 shifts
            ("line", (1.3, 0.75, 0.02), 8.0, 0.0),                                   # in the pixel plane: X | Y bins > 54
            ("line", (2.9, 2.7, 0.03), 25.0, 0.0),                                   # ... > 80
            ("r", 190.0, 0.03),                                                      # drift window cut by the start of the time window; beyond the 256-node cap
            ("line", (0.3, 0.2, 0.15), drift - 0.2, 9.0 if m0 else 4.0),             # ... by its end
            ("off",)]


def build_segments(cfg, plan=None):
    H.load_cfg(cfg)
    det = consts.detector
    plan = _plan(cfg) if plan is None else plan
    B = det.TPC_BORDERS[0]
    sgn = np.sign(B[2][1] - B[2][0])
    seg = synth.make_segments(len(plan), seed=31, segs_per_event=len(plan))
    batching.swap_coordinates(seg)
    x0, y0 = B[0][0] + 0.31 * (B[0][1] - B[0][0]), B[1][0] + 0.43 * (B[1][1] - B[1][0])
    for k, item in enumerate(plan):
        a = np.array([x0 + 4.3 * (k % 4) + 0.013 * k, y0 + 5.1 * (k // 4) + 0.029 * k, 0.0])
        t0 = 0.0
        if item[0] == "r":
            _, rr, d = item
            a[2] = B[2][0] + sgn * d
            ang, tilt = 0.7 + 0.37 * k, 0.0998
            L = rr * np.sqrt(2 * det.TRAN_DIFF * d / det.V_DRIFT)
            for _ in range(4):                                   # rr widths of the cloud at the segment's MIDPOINT (drifting.py:47-52)
                L = rr * np.sqrt(2 * det.TRAN_DIFF * (d + 0.5 * tilt * L) / det.V_DRIFT)
            b = a + L * np.array([np.cos(ang) * np.sqrt(1 - tilt * tilt), np.sin(ang) * np.sqrt(1 - tilt * tilt), sgn * tilt])
        elif item[0] == "line":
            _, (dx, dy, dz), d, t0 = item
            a[2] = B[2][0] + sgn * d
            b = a + np.array([dx, dy, sgn * dz])
        else:
            zmid = 0.5 * (B[2][0] + B[2][1])
            a = np.array([B[0][0] + 0.5, a[1], zmid])
            b = np.array([B[0][0] - 0.3, a[1] + 0.2, zmid + 0.1])
        for i, ax in enumerate("xyz"):
            seg[ax + "_start"][k] = a[i]; seg[ax + "_end"][k] = b[i]
            seg[ax][k] = 0.5 * (np.float32(a[i]).astype(np.float64) + np.float32(b[i]))
        L = float(np.linalg.norm(b - a))
        seg["dx"][k] = max(L, 1e-4); seg["dEdx"][k] = 2.1; seg["dE"][k] = 2.1 * seg["dx"][k]
        for f in ("t0", "t0_start", "t0_end"):
            seg[f][k] = t0
    return seg


@functools.lru_cache(maxsize=None)
def _inputs(cfg):
    seg = build_segments(cfg)
    r = H.quench_drift(O, seg)
    assert (r["pixel_plane"] == 0).all()
    nmax = O.max_pixels(r)
    P = 3 * nmax + 6
    _, neigh, _, _ = O.get_pixels(r, nmax, P, 1)
    _, T = O.time_intervals(r)
    assert (neigh[-1] == -1).any() and (neigh[-1] != -1).any()      # the last segment leaves the pixel plane
    return r, np.ascontiguousarray(neigh), int(T)


@functools.lru_cache(maxsize=None)
def _case(cfg, kind):
    """(records, pixels, T, response, oracle waveforms): computed once, never written to."""
    r, neigh, T = _inputs(cfg)
    H.load_cfg(cfg)
    resp = make_response(kind)
    ref = O.tracks_current(r, neigh, T, resp)
    assert np.isfinite(ref).all()
    for a in (r, neigh, resp, ref):
        a.setflags(write=False)
    return r, neigh, T, resp, ref


_seen = {}            # (cfg, kind) -> {setting: per-pair slot sets, 0 for pairs that were not live, compared and emitted by the form}


def _run(cfg, kind, setting, extra=None):
    """One launch under SETTINGS[setting]: waveforms asserted against the oracle, census returned."""
    r, neigh, T, resp, ref = _case(cfg, kind)
    H.load_cfg(cfg)
    opts = dict(SETTINGS[setting], **(extra or {}))
    census = {}

    def launch(**o):
        # (_tracks_current_on restores the options before it returns: the census is of the launch, not of the options now)
        sig, st = _tracks_current_on("gform", neigh, r, resp, T, **o)
        census.update(detsim.gform_census(per_pair=True, n_pairs=neigh.size))
        return sig, st

    sig, st = launch(**opts)
    c = dict(census)
    live = np.abs(ref).max(axis=-1) > 0
    slots = c.pop("pair_slots").reshape(neigh.shape)
    print(f"{cfg} {kind} {setting}: live pairs {int(live.sum())}, fallback {st.n_fallback}, census {c}")
    assert c["pairs"] == neigh.size and c["m"] == (1 if cfg == "module0" else 2)
    # Per-pair bar for every pair above 1e-5 of the scale (segment charge x largest response entry); below it a pair can be made of
    # pruned weights only (test_tracks_current_length_sweep_vs_oracle: the one allowed floor, 1e-7 of that scale) ...
    pair_peak = np.abs(ref).max(axis=-1, keepdims=True)
    charge_scale = r["n_electrons"].astype(np.float64)[:, None, None] * np.abs(resp).max()
    main = pair_peak >= 1e-5 * charge_scale
    err = np.abs(sig.astype(np.float64) - ref)
    tol_floor = 1e-5 * np.abs(ref) + 1e-7 * charge_scale
    bad = ((err > tol_floor) | (main & (err > 1e-5 * np.abs(ref) + 1e-7 * pair_peak))).any(axis=-1)
    assert not bad.any(), f"{cfg} {kind} {setting}: {_blame(bad, live, slots)}"
    H.assert_wave_close(np.where(main, sig, ref), ref, rtol=1e-5, atol_peak=1e-7, what=f"{cfg} {kind} {setting}")
    # the fallback carries at most a tenth of the live pairs, and at least one pair sits flagged next to unflagged ones
    flagged = (slots >> detsim_slot("flagged")) & 1
    assert 1 <= int((flagged & live).sum()) <= 0.1 * live.sum(), f"{int((flagged & live).sum())} flagged of {int(live.sum())} live pairs"
    emitted = ((slots >> detsim_slot("emitted")) & 1).astype(bool) & live & main[..., 0]
    _seen.setdefault((cfg, kind), {})[setting + repr(sorted((extra or {}).items()))] = np.where(emitted, slots, 0)
    return sig, c, slots, live


def _blame(bad, live, slots):
    """Names the classes a mismatch sits in: per census slot, failing / live pairs, the slots whose every live pair fails first."""
    from larndsim_amd.abi import GFORM_CENSUS_SLOTS
    rows = []
    for k, name in enumerate(GFORM_CENSUS_SLOTS[1:28], start=1):
        member = ((slots >> k) & 1).astype(bool) & live
        if (member & bad).any():
            rows.append((int((member & bad).sum()) / int(member.sum()), f"{name} {int((member & bad).sum())}/{int(member.sum())}"))
    rows.sort(key=lambda t: -t[0])
    return (f"{int(bad.sum())} of {int(live.sum())} live pairs out of tolerance, first at {tuple(int(v) for v in np.argwhere(bad)[0])}; "
            "failing / live pairs by census slot: " + ", ".join(t[1] for t in rows))


def detsim_slot(name):
    from larndsim_amd.abi import GFORM_CENSUS_SLOTS
    return GFORM_CENSUS_SLOTS.index(name)


def _count(slot_sets, name):
    return int(((slot_sets >> detsim_slot(name)) & 1).sum())


@pytest.mark.parametrize("kind", list(RESPONSES))
@pytest.mark.parametrize("cfg", CFGS)
def test_defaults_and_prune_zero(cfg, kind):
    """Default options: the tick tile the table's support asks for, the 16-node product over all pairs at M = 1 and 4-node blocks
    elsewhere; then with every weight kept (prune_log 0) the per-pair bar for every pair the form emitted, however small, and for
    the pairs flagged for the monolithic kernel down to 1e-12 of the charge scale (below that its erf differences show their
    cancellation noise, 1e-16 absolute: test_tracks_current_length_sweep_vs_oracle)."""
    sig, c, slots, live = _run(cfg, kind, "defaults")
    assert c["tt"] == RESPONSES[kind]
    assert c["qb0"] == (0 if cfg == "module0" else 1) and c["qb12"] == 1
    r, neigh, T, resp, ref = _case(cfg, kind)
    sig0, _ = _tracks_current_on("gform", neigh, r, resp, T, prune_log=0.0)
    flagged0 = ((detsim.gform_census(per_pair=True, n_pairs=neigh.size)["pair_slots"].reshape(neigh.shape) >> detsim_slot("flagged")) & 1).astype(bool)
    pair_peak = np.abs(ref).max(axis=-1, keepdims=True)
    charge_scale = r["n_electrons"].astype(np.float64)[:, None, None] * np.abs(resp).max()
    deep = (pair_peak >= 1e-12 * charge_scale) | ~flagged0[..., None]
    n_main, n_deep = int((pair_peak >= 1e-5 * charge_scale).sum()), int((deep & (pair_peak > 0)).sum())
    print(f"{cfg} {kind} prune_log 0: {n_deep} live pairs at the per-pair bar ({n_main} above 1e-5 of the charge scale), {int(flagged0.sum())} flagged")
    assert n_deep >= n_main and flagged0.sum() <= 0.1 * live.sum()
    H.assert_wave_close(np.where(deep, sig0, ref), ref, rtol=1e-5, atol_peak=1e-7, what=f"{cfg} {kind} prune_log 0")


@pytest.mark.parametrize("cfg", CFGS)
def test_defaults_twice_same_bits(cfg):
    """gcorr_kernel promises results that do not depend on timing: two launches, the same bits."""
    a, *_ = _run(cfg, "dense", "defaults")
    b, *_ = _run(cfg, "dense", "defaults")
    assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", list(RESPONSES))
@pytest.mark.parametrize("cfg", CFGS)
def test_four_node_blocks_in_every_launch(cfg, kind):
    """debug_gform 65536: gcorr_kernel<M, true> also for the launch over all pairs (M = 1: by default only the listed classes)."""
    _, c, slots, live = _run(cfg, kind, "qb_everywhere")
    assert c["qb0"] == 1 and c["qb12"] == 1 and c["cls0"] >= 10


@pytest.mark.parametrize("kind", list(RESPONSES))
@pytest.mark.parametrize("cfg", CFGS)
def test_sixteen_node_product_in_every_launch(cfg, kind):
    """debug_gform 4096: gcorr_kernel<M, false> also for the listed classes and at M = 2; the smaller first class fills the lists."""
    _, c, slots, live = _run(cfg, kind, "qb_nowhere")
    assert c["qb0"] == 0 and c["qb12"] == 0
    _, c, slots, live = _run(cfg, kind, "qb_nowhere_listed")
    assert c["qb0"] == 0 and c["qb12"] == 0 and c["cls1"] >= 10 and c["cls2"] >= 5


@pytest.mark.parametrize("kind", list(RESPONSES))
@pytest.mark.parametrize("cfg", CFGS)
def test_small_first_lds_class(cfg, kind):
    """debug_lds_pad_kb 8: most pairs leave class 0 for the first listed launch."""
    _, c, slots, live = _run(cfg, kind, "small_first_class")
    assert c["cls1"] >= 10 and c["cls0"] < 0.5 * c["emitted"]


@pytest.mark.parametrize("kind", list(RESPONSES))
@pytest.mark.parametrize("cfg", CFGS)
def test_small_first_and_second_lds_class(cfg, kind):
    """... and with the second class at 12 KB the launch at the caps' size gets pairs."""
    _, c, slots, live = _run(cfg, kind, "small_first_and_second_class")
    assert c["cls2"] >= 5


@pytest.mark.parametrize("cfg", CFGS)
def test_256_tick_tiles_on_full_support(cfg):
    """debug_gform 8192 on the dense table: 256-tick tiles over a support of ~1900 ticks, eight tiles per pair instead of four."""
    _, c, slots, live = _run(cfg, "dense", "defaults", extra=dict(debug_gform=8192))
    assert c["tt"] == 256


@pytest.mark.parametrize("kind", list(RESPONSES))
@pytest.mark.parametrize("cfg", CFGS)
def test_workgroup_tables_kernel_for_every_pair(cfg, kind):
    _, c, slots, live = _run(cfg, kind, "workgroup_tables")
    assert c["t_wave"] == 0 and c["t_wide"] == 0 and c["t_wg"] == c["emitted"] >= 30 and c["wg_forced"] >= 10


@pytest.mark.parametrize("kind", list(RESPONSES))
@pytest.mark.parametrize("cfg", CFGS)
def test_floor_every_named_slot_held_live_pairs(cfg, kind):
    """Over the settings of this (config, response): every slot of FLOOR_SLOTS held >= 3 pairs with a non-zero oracle waveform
    that were emitted by the named kernels and compared at the per-pair bar.  (Runs the settings itself where an earlier test of
    this module has not: any order, any selection.)"""
    for setting in SETTINGS:
        if setting + "[]" not in _seen.get((cfg, kind), {}):
            _run(cfg, kind, setting)
    union = functools.reduce(np.bitwise_or, _seen[(cfg, kind)].values())      # a pair counts once, whatever the setting it met the slot under
    held = {}
    for name in FLOOR_SLOTS:
        if name == "listed_zrec":
            parts = ("cls1_zrec", "cls2_zrec")
        elif name == "emask_top":      # an edge at the top of the time window, where the tables carry weight (k = 0: emask0, is their far tail)
            parts = ("emask1", "emask2")
        else:
            parts = (name,)
        held[name] = int(np.any([((union >> detsim_slot(p)) & 1).astype(bool) for p in parts], axis=0).sum())
    print(f"{cfg} {kind} floor: {held}")
    short = {k: v for k, v in held.items() if v < 3 and k not in UNREACHABLE}
    assert not short, f"slots with fewer than 3 live, compared pairs: {short}"
    # a slot declared unreachable is empty: an input or a config that reaches it one day fails here, and gets its floor
    assert all(held[k] == 0 for k in UNREACHABLE), f"declared unreachable, but met: { {k: held[k] for k in UNREACHABLE} }"
    assert not set(UNREACHABLE) & {"cls0", "cls1", "cls2", "nb1", "nb2", "nb3p", "t_wave", "t_wide", "t_wg"}


def test_census_refused_after_another_current_path():
    """The census describes the last launch of the node-separable form only: after the monolithic kernel ran it is refused."""
    r, neigh, T, resp, ref = _case("module0", "narrow")
    H.load_cfg("module0")
    _tracks_current_on("gform", neigh, r, resp, T)
    assert detsim.gform_census()["tables"] > 0
    _tracks_current_on("mono", neigh, r, resp, T)
    with pytest.raises(lib.LdsimError, match="node-separable"):
        detsim.gform_census()
