"""CPU: charge universes -- the ctypes mirror of LdsimChargeVariation against the header text, the variations of
larndsim_amd/charge_universes.py (nominal, every refusal of validate and parse), the driver's argument checks, the numpy twin
``segment_weights`` against the oracle's quench + drift under patched constants (bit for bit, u4 and f4 n_electrons columns), and
the linearity the feature rests on, shown on the oracle: ``weighted_sums`` of the oracle's nominal per-slot signals against the
oracle's sums of a fresh run under the patched constants, and the hits of both.  No GPU.

The case is the 300-segment module0 case of test_gpu_fee_universes.py (seed 31, batches 0, 1, 2 of 90, 47 and 133 segments, the
survey response, its synthetic segments); the few helper lines are copied from there.  The oracle's currents of the three
batches take about a minute on eight cores: the nominal run is made once, every knob adds one fresh run."""
import contextlib
import ctypes as C
import functools
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import helpers as H
from larndsim_amd import abi, batching, consts, synth
from larndsim_amd import charge_universes as CU
from larndsim_amd import fee_universes as FU
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
SEED = 31
ECHO_TICKS = (90, 400)
LONE_SHIFT, LONE_DE = (5.0, -20.0), 30.0
LATE_SHIFT, LATE_US = (10.0, -20.0), 100.0
SIZES = [(0, 90), (1, 47), (-1, 30), (2, 133)]          # (batch id, segments)
MAX_LEFT_OUT = 0.02
KNOBS = ("lifetime_half", "lifetime_tenth", "birks_ab", "birks_kb", "box", "box_alpha", "w_ion_half")


def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_charge_universes", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


# ---- 1. the struct, nominal, the refusals -----------------------------------------------------------------------------------------
def test_abi_variation_is_the_header_struct():
    """LdsimChargeVariation against the declaration in include/ldsim.h: 56 bytes, the fields in order at the offsets the C
    declaration gives them; the entry points are declared, LdsimFeeVariation and the ABI version are what they were"""
    text = open(os.path.join(REPO, "include", "ldsim.h")).read()
    body = re.search(r"typedef struct LdsimChargeVariation \{(.*?)\} LdsimChargeVariation;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        size = 8 if ctype == "double" else 4
        for n in names.split(","):
            off = (off + size - 1) // size * size
            fields.append((n.strip(), size, off))
            off += size
    assert off == 56 and C.sizeof(abi.LdsimChargeVariation) == 56
    assert [f[0] for f in fields] == [f[0] for f in abi.LdsimChargeVariation._fields_]
    for name, size, o in fields:
        d = getattr(abi.LdsimChargeVariation, name)
        assert (d.offset, d.size) == (o, size), name
    assert tuple(f[0] for f in fields[:-1]) == CU.FIELDS and fields[-1][0] == "pad" and len(CU.FIELDS) == 7
    for fn in ("ldsim_charge_variation_nominal", "ldsim_chain_universes", "ldsim_chain_universe_weights_download",
               "ldsim_chain_universe_waveforms_dense"):
        assert f"int {fn}(" in text, fn
    assert re.search(r"#define LDSIM_ABI_VERSION 8\b", text) and C.sizeof(abi.LdsimFeeVariation) == 112


def test_nominal_is_the_constants_and_pack_round_trips():
    H.load_cfg("module0")
    det, phys = consts.detector, consts.physics
    v = CU.nominal()
    assert set(v) == set(CU.FIELDS)
    assert v == dict(electron_lifetime=det.ELECTRON_LIFETIME, w_ion=phys.W_ION, box_alpha=phys.BOX_ALPHA, box_beta=phys.BOX_BETA,
                     birks_ab=phys.BIRKS_Ab, birks_kb=phys.BIRKS_kb, recomb_mode=phys.BIRKS)
    assert CU.nominal(phys.BOX)["recomb_mode"] == 1 == CU.BOX and CU.BIRKS == phys.BIRKS
    w = CU.variation(v, W_ION=1e-5, recomb_model="box", Birks_Ab=0.7)
    assert (w["w_ion"], w["recomb_mode"], w["birks_ab"]) == (1e-5, 1, 0.7) and v["w_ion"] == phys.W_ION
    assert CU.variation(RECOMB_MODEL="birks")["recomb_mode"] == 2
    for bad, word in ((dict(E_FIELD=0.4), "unknown key 'E_FIELD'"), (dict(recomb_model="thomas"), "must be \"box\" or \"birks\"")):
        with pytest.raises(ValueError, match=word):
            CU.variation(**bad)
    arr = CU.pack([v, w])
    assert len(arr) == 2 and CU.unpack(arr[0]) == v and CU.unpack(arr[1]) == w and arr[1].pad == 0
    rows = CU.universe_rows(["a", "b"], [v, w], [FU.nominal(), FU.variation(gain=5.0)])
    assert rows.dtype == CU.FILE_UNIVERSE and rows["w_ion"].tolist() == [phys.W_ION, 1e-5] and rows["gain"][1] == 5.0
    assert rows["recomb_mode"].tolist() == [2, 1] and rows["name"].tolist() == [b"a", b"b"] and CU.FILE_HIT == FU.FILE_HIT
    assert CU.file_rows is FU.file_rows


def test_validate_refuses():
    H.load_cfg("module0")
    n = CU.nominal()
    assert CU.validate([n] * 64)
    for vs, word in (([], r"n = 0 universes, must lie in \[1, 64\]"), ([n] * 65, r"n = 65 universes"),
                     ([n, {k: x for k, x in n.items() if k != "w_ion"}], "universe 1: missing fields .'w_ion'."),
                     ([dict(n, e_field=0.5)], "universe 0: .*unknown key .'e_field'."),
                     ([n, dict(n, electron_lifetime=0.0)], "universe 1: electron_lifetime 0.0 must be > 0"),
                     ([dict(n, electron_lifetime=-3.0)], "universe 0: electron_lifetime -3.0 must be > 0"),
                     ([dict(n, w_ion=0)], "universe 0: w_ion 0 must be > 0"),
                     ([dict(n, recomb_mode=0)], "universe 0: recomb_mode 0 must be 1 .box. or 2 .Birks."),
                     ([dict(n, recomb_mode=3)], "recomb_mode 3"), ([dict(n, recomb_mode=2.0)], "recomb_mode 2.0"),
                     ([dict(n, recomb_mode=True)], "recomb_mode True")):
        with pytest.raises(ValueError, match=word):
            CU.validate(vs)
    for f in CU.FLOAT_FIELDS:
        for x in (float("nan"), float("inf"), -float("inf"), "1", None, True):
            with pytest.raises(ValueError, match=f"universe 2: {f} = .* is not finite"):
                CU.validate([n, n, dict(n, **{f: x})])


def test_parse_refuses_and_splits_the_keys(tmp_path):
    H.load_cfg("module0")
    got = CU.parse([{"name": "a"}, {"W_ION": 2e-5, "gain": 4.5, "recomb_model": "box"}, {"name": "c", "BIRKS_KB": 0.05}])
    assert got == [("a", {}, {}), ("universe1", {"W_ION": 2e-5, "recomb_model": "box"}, {"gain": 4.5}), ("c", {"BIRKS_KB": 0.05}, {})]
    for entries, word in (({}, "must hold a JSON list of objects"), ([1], "must hold a JSON list of objects"), ([], "n = 0 universes"),
                          ([{}] * 65, "n = 65 universes"), ([{}, {"E_FIELD": 0.5}], "universe 1: unknown key 'E_FIELD'"),
                          ([{"V_DRIFT": 0.1}], "universe 0: unknown key 'V_DRIFT'"), ([{"LAR_DENSITY": 1.4}], "unknown key"),
                          ([{"RECOMB_MODEL": 1}], "universe 0: RECOMB_MODEL 1 must be"), ([{"RECOMB_MODEL": "modified box"}], "RECOMB_MODEL"),
                          ([{"name": "x" * 65}], "name longer than 64 bytes")):
        with pytest.raises(ValueError, match=word):
            CU.parse(entries)
    path = tmp_path / "u.json"
    json.dump([{"name": "nominal"}, {"name": "both", "ELECTRON_LIFETIME": 500.0, "RECOMB_MODEL": "box", "RESET_CYCLES": 6}], open(path, "w"))
    names, cs, fs = CU.load(str(path))
    assert names == ["nominal", "both"] and cs[0] == CU.nominal() and fs[0] == FU.nominal()
    assert cs[1] == CU.variation(electron_lifetime=500.0, recomb_mode=1) and fs[1] == FU.variation(reset_cycles=6)
    json.dump([{"W_ION": -1.0}], open(path, "w"))
    with pytest.raises(ValueError, match="universe 0: w_ion -1.0 must be > 0"):
        CU.load(str(path))
    json.dump([{"V_REF": consts.detector.V_CM}], open(path, "w"))
    with pytest.raises(ValueError, match="v_ref == v_cm"):
        CU.load(str(path))


def test_cli_charge_universes_argument_checks(tmp_path, monkeypatch, capsys):
    """--n_gpus 2, --charge_statistics and --tracks_current_mc are refused, noisy universes without --rng keyed are refused, an
    unknown key or an unreadable file is an argument error; the option may stand beside --fee_universes"""
    cli = _cli()
    base = ["--input_filename", "x.npy", "--output_filename", str(tmp_path / "y.npz")]
    assert cli._parse_args(base).charge_universes is None
    quiet, noisy, unknown, fee = (str(tmp_path / n) for n in ("quiet.json", "noisy.json", "unknown.json", "fee.json"))
    json.dump([{"name": "nominal"}, {"name": "short", "ELECTRON_LIFETIME": 500.0, "GAIN": 4.2}], open(quiet, "w"))
    json.dump([{"name": "nominal"}, {"name": "loud", "W_ION": 2e-5, "DISCRIMINATOR_NOISE": 900.0}], open(noisy, "w"))
    json.dump([{"name": "x", "E_FIELD": 0.2}], open(unknown, "w"))
    json.dump([{"name": "low", "DISCRIMINATION_THRESHOLD": 3500.0}], open(fee, "w"))
    assert cli._parse_args(base + ["--charge_universes", quiet]).charge_universes == quiet
    assert cli._parse_args(base + ["--charge_universes", noisy, "--rng", "keyed"]).charge_universes == noisy
    a = cli._parse_args(base + ["--charge_universes", quiet, "--fee_universes", fee])
    assert (a.charge_universes, a.fee_universes) == (quiet, fee)
    for args, word in ((["--charge_universes", noisy], "universe 1 (loud) has a non-zero noise charge"),
                       (["--charge_universes", noisy, "--rng", "table"], "give --rng keyed as well"),
                       (["--charge_universes", unknown], "unknown key 'E_FIELD'"),
                       (["--charge_universes", str(tmp_path / "missing.json")], "missing.json"),
                       (["--charge_universes", quiet, "--charge_statistics", "--rng", "keyed"],
                        "--charge_universes is not available with --charge_statistics"),
                       (["--charge_universes", quiet, "--tracks_current_mc"],
                        "--charge_universes is not available with --tracks_current_mc")):
        with pytest.raises(SystemExit):
            cli._parse_args(base + args)
        assert word in capsys.readouterr().err.replace("\n", " ").replace("  ", " "), word
    help_text = " ".join(cli._parser().format_help().split())
    assert "--charge_universes FILE.json" in help_text and "RECOMB_MODEL" in help_text
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    with pytest.raises(SystemExit, match="--charge_universes is not available with --n_gpus > 1"):
        cli.launch_ranks_if_asked(base + ["--charge_universes", quiet, "--n_gpus", "2"])
    assert cli.launch_ranks_if_asked(base + ["--charge_universes", quiet]) is None
    out = str(tmp_path / "y.npz")
    with pytest.raises(ValueError, match="universe 1 .loud. has a non-zero noise charge.*--rng keyed"):
        cli.run_simulation("x.npy", out, charge_universes=noisy)
    with pytest.raises(ValueError, match="--charge_universes is not available with --charge_statistics"):
        cli.run_simulation("x.npy", out, charge_universes=quiet, charge_statistics=True, rng="keyed")
    with pytest.raises(ValueError, match="--charge_universes is not available with --tracks_current_mc"):
        cli.run_simulation("x.npy", out, charge_universes=quiet, tracks_current_mc=True)
    with pytest.raises(ValueError, match="--charge_universes is not available with --n_gpus > 1"):
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("RANK", "0")
        cli.run_simulation("x.npy", out, n_gpus=2, charge_universes=quiet)


# ---- the module0 case ----------------------------------------------------------------------------------------------------------------
def _segments(cfg="module0", n=300, seed=SEED):
    H.load_cfg(cfg)
    spill = bool(consts.sim.IS_SPILL_SIM)
    seg = synth.make_segments(n, seed=seed, segs_per_event=n, spill=spill)
    if spill:                            # the driver removes the spill offset
        loc = seg["event_id"] % consts.sim.MAX_EVENTS_PER_FILE
        for f in ("t0", "t0_start", "t0_end"):
            seg[f] = seg[f] - loc * consts.sim.SPILL_PERIOD
    batching.swap_coordinates(seg)
    return seg


def _add_synthetic(seg):
    """test_gpu_fee_universes.py's: segments 1 and 2 echoes of segment 0 along the drift axis, segment 3 a copy moved in the
    pixel plane with LONE_DE times the energy, segment 4 a copy LATE_US later whose signal is cut off by the last tick"""
    det = consts.detector
    z = float(seg["z"][0])
    for k, ticks in enumerate(ECHO_TICKS, start=1):
        dz = ticks * det.TIME_SAMPLING * det.V_DRIFT
        inside = [b for b in np.sort(np.asarray(det.TPC_BORDERS, dtype=np.float64)[:, 2, :], axis=-1) if b[0] <= z <= b[1]]
        assert len(inside) == 1, "segment 0 lies in one TPC"
        lo, hi = inside[0]
        step = dz if z + dz + 1.0 < hi else -dz
        assert lo < z + step - 1.0 and z + step + 1.0 < hi, "the echo stays inside the TPC"
        sid = seg["segment_id"][k]
        seg[k] = seg[0]
        seg["segment_id"][k] = sid
        for f in ("z", "z_start", "z_end"):
            seg[f][k] += step
    tpc = [b for b in np.sort(np.asarray(det.TPC_BORDERS, dtype=np.float64), axis=-1) if b[2][0] <= z <= b[2][1]][0]
    for k, shift in ((3, LONE_SHIFT), (4, LATE_SHIFT)):
        sid = seg["segment_id"][k]
        seg[k] = seg[0]
        seg["segment_id"][k] = sid
        for a, d in zip("xy", shift):
            for f in (a, a + "_start", a + "_end"):
                seg[f][k] += d
            i = "xyz".index(a)
            assert tpc[i][0] + 1.0 < seg[a][k] < tpc[i][1] - 1.0, "the moved segment stays inside the TPC"
    seg["dE"][3] *= LONE_DE
    for f in ("t0", "t0_start", "t0_end"):
        seg[f][4] += LATE_US
    return seg


@functools.lru_cache(maxsize=None)
def _module0_case():
    """the segments, their batch ids and the response: made once, read only"""
    seg = _add_synthetic(_segments())
    bid = np.concatenate([np.full(n, b) for b, n in SIZES]).astype(np.int32)
    resp = synth.make_response("survey")
    for a in (seg, bid, resp):
        a.setflags(write=False)
    return seg, bid, resp


_CONSTS = {"electron_lifetime": ("detector", "ELECTRON_LIFETIME"), "w_ion": ("physics", "W_ION"),
           "box_alpha": ("physics", "BOX_ALPHA"), "box_beta": ("physics", "BOX_BETA"), "birks_ab": ("physics", "BIRKS_Ab"),
           "birks_kb": ("physics", "BIRKS_kb")}


@contextlib.contextmanager
def _patched(v):
    """``consts`` with the six constants of the charge variation ``v``"""
    places = [(getattr(consts, ns), name, v[f]) for f, (ns, name) in _CONSTS.items()]
    was = [(o, n, getattr(o, n)) for o, n, _ in places]
    try:
        for o, n, x in places:
            setattr(o, n, x)
        yield
    finally:
        for o, n, x in was:
            setattr(o, n, x)


def knobs():
    """{name: charge variation}: each knob alone, moved from module0's constants under Birks"""
    H.load_cfg("module0")
    n = CU.nominal(CU.BIRKS)
    return {
        "lifetime_half": CU.variation(n, electron_lifetime=0.5 * n["electron_lifetime"]),
        "lifetime_tenth": CU.variation(n, electron_lifetime=0.1 * n["electron_lifetime"]),
        "birks_ab": CU.variation(n, birks_ab=0.9 * n["birks_ab"]),
        "birks_kb": CU.variation(n, birks_kb=1.2 * n["birks_kb"]),
        "box": CU.variation(n, recomb_mode=CU.BOX),
        "box_alpha": CU.variation(n, recomb_mode=CU.BOX, box_alpha=0.9 * n["box_alpha"]),
        "w_ion_half": CU.variation(n, w_ion=0.5 * n["w_ion"]),
    }


def _quench_drift(seg, v):
    """the oracle's quench and drift of ``seg`` under ``consts`` patched to ``v``"""
    ref = seg.copy()
    with _patched(v):
        O.quench(ref, v["recomb_mode"])
        O.drift(ref)
    return ref


def _twin_weights(v, seg, ref):
    """segment_weights of ``v`` from the records ``seg`` and their nominal quench + drift ``ref``"""
    det = consts.detector
    in_tpc = ref["pixel_plane"] != det.DEFAULT_PLANE_INDEX
    plane = np.where(in_tpc, ref["pixel_plane"], 0)
    z_anode = np.asarray(det.TPC_BORDERS, dtype=np.float64)[plane, 2, 0]
    return CU.segment_weights(v, ref["n_electrons"], seg["dE"], seg["dEdx"], det.E_FIELD, np.abs(seg["z"].astype(np.float64) - z_anode),
                              in_tpc, seg.dtype["n_electrons"], det.LAR_DENSITY, det.V_DRIFT)


# ---- 2. the segment_weights twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u4", "f4"])
def test_segment_weights_twin_is_the_oracles_quench_and_drift(kind):
    """n_k of the twin equals the n_electrons of the oracle's quench + drift under the patched constants bit for bit, for every
    knob, with a u4 and with an f4 n_electrons column; the nominal weights are exactly 1"""
    seg, bid, _ = _module0_case()
    H.load_cfg("module0")
    dt = np.dtype([(n, kind if n == "n_electrons" else seg.dtype[n]) for n in seg.dtype.names])
    s = np.zeros(len(seg), dtype=dt)
    for n in seg.dtype.names:
        s[n] = seg[n]
    det, phys = consts.detector, consts.physics
    recomb = phys.BIRKS_Ab / (1 + phys.BIRKS_kb * float(s["dEdx"][7]) / (det.E_FIELD * det.LAR_DENSITY))
    s["dE"][7] = 0.95 * phys.W_ION / recomb                      # under one electron: none in a u4 column; over three at W_ion / 4
    nominal = CU.nominal(CU.BIRKS)
    ref = _quench_drift(s, nominal)
    assert (ref["pixel_plane"] != consts.detector.DEFAULT_PLANE_INDEX).sum() > 250
    w, n_k, unw = _twin_weights(nominal, s, ref)
    assert n_k.tobytes() == ref["n_electrons"].astype(np.float64).tobytes() and unw == 0
    live = ref["n_electrons"] != 0
    assert (w[live] == 1.0).all() and (w[~live] == 0.0).all() and live.sum() >= len(s) - 1
    if kind == "u4":
        assert ref["n_electrons"][7] == 0
    for name, v in knobs().items():
        want = _quench_drift(s, v)["n_electrons"].astype(np.float64)
        w, n_k, unw = _twin_weights(v, s, ref)
        assert n_k.tobytes() == want.tobytes(), name
        assert not np.array_equal(want, ref["n_electrons"]), name
        n_res = ref["n_electrons"].astype(np.float64)
        back = w * n_res
        back = np.rint(back) if kind == "u4" else back.astype(np.float32).astype(np.float64)
        assert np.array_equal(back[live], want[live]), name
        assert unw == int(((n_res == 0) & (want != 0)).sum()), name
        print(f"{kind} {name}: weights {w[live].min():.6f} ... {w[live].max():.6f}")
    # W_ion / 4 gives the segment without resident charge an electron: counted, weight 0
    if kind == "u4":
        v = CU.variation(nominal, w_ion=0.25 * nominal["w_ion"])
        w, n_k, unw = _twin_weights(v, s, ref)
        assert unw == 1 and w[7] == 0 and n_k[7] > 0


def test_weights_outside_every_tpc_and_unsimulated_are_one():
    H.load_cfg("module0")
    n = CU.nominal(CU.BIRKS)
    v = CU.variation(n, electron_lifetime=100.0)
    n_res = np.array([1000.0, 0.0, 1000.0, 1000.0, 0.0])
    w, n_k, unw = CU.segment_weights(v, n_res, np.full(5, 0.05), np.full(5, 2.0), 0.5, np.full(5, 20.0),
                                     [True, True, False, True, True], "u4", 1.38, 0.16, simulated=[True, True, True, False, False])
    assert w[2] == 1.0 and w[3] == 1.0 and w[4] == 1.0 and w[1] == 0.0 and 0 < w[0] < 2 and unw == 1 and (n_k > 0).all()


def test_weighted_sums_twin_windows_and_order():
    """the twin on hand-made slots: clipping to the row, to the window and to [0, n_ticks); products rounded before they are added"""
    row = np.arange(1, 9, dtype=np.float32)
    S = CU.weighted_sums([[(0, -3, 0, 8, row), (1, 4, 2, 6, row)], []], [2.0, 0.5], 8)
    want = np.zeros((2, 8))
    want[0, 0:5] = 2.0 * row[3:8]
    want[0, 6:8] += 0.5 * row[2:4]
    assert np.array_equal(S, want)
    w = np.array([1 / 3, 1e-17 / 3])
    S = CU.weighted_sums([[(0, 0, 0, 1, np.float32([3.0])), (1, 0, 0, 1, np.float32([3e17]))]], w, 1)
    assert S[0, 0] == w[0] * 3.0 + w[1] * np.float64(np.float32(3e17))


# ---- 3. linearity on the oracle --------------------------------------------------------------------------------------------------
def _oracle_run(seg, resp, v, want_slots):
    """the oracle's chain of one batch under ``consts`` patched to ``v``: the unique pixels, the sums S [U][N_t] and, asked for,
    per pixel its slots (segment, start tick, 0, T, row) in the order sum_pixel_signals adds them"""
    det = consts.detector
    ref = _quench_drift(seg, v)
    nmax = O.max_pixels(ref)
    r = int(np.ceil(ref["tran_diff"].max() * 5 / det.PIXEL_PITCH))
    P = (2 * r + 1) * nmax + (1 + 2 * r) * r * 2
    _, neigh, nrad, _ = O.get_pixels(ref, nmax, P, r)
    upix = O.unique_pixels(neigh)
    starts, T = O.time_intervals(ref)
    sig = O.tracks_current(ref, neigh, T, resp)
    pim = O.pixel_index_map(neigh, upix)
    tpm = O.track_pixel_map(upix, neigh, nrad, int(nrad.max()) + 1, consts.sim.MAX_TRACKS_PER_PIXEL)
    ps, _, _ = O.sum_pixel_signals(sig, starts, pim, tpm, len(upix), want_tracks=False)
    out = dict(upix=upix, S=ps, ref=ref)
    if want_slots:
        pixels = [[] for _ in upix]
        for itrk, ipix in zip(*np.nonzero(pim >= 0)):            # (row-major: segment by segment, as the oracle adds)
            u = int(pim[itrk, ipix])
            if itrk in tpm[u]:
                pixels[u].append((int(itrk), int(np.rint(starts[itrk] / det.TIME_SAMPLING)), 0, int(T), sig[itrk, ipix].copy()))
        out["pixels"] = pixels
    return out


@functools.lru_cache(maxsize=None)
def _nominal_runs():
    """the oracle's nominal run of the three batches with its per-slot signals: made once, read only"""
    seg, bid, resp = _module0_case()
    H.load_cfg("module0")
    return {b: _oracle_run(seg[bid == b], resp, CU.nominal(CU.BIRKS), True) for b in (0, 1, 2)}


def _oracle_hits(S):
    det = consts.detector
    tt = np.linspace(0, det.TIME_INTERVAL[1], len(det.TIME_TICKS) + 1)
    adc, ticks, _ = O.get_adc_values(S, None, tt, np.full(len(S), float(det.DISCRIMINATION_THRESHOLD)), want_fractions=False)
    return adc, ticks, O.digitize(adc)


def test_nominal_weighted_sums_are_the_oracles_sums():
    """weights 1: the twin fed with the oracle's per-slot signals is the oracle's sum_pixel_signals bit for bit"""
    for b, r in _nominal_runs().items():
        S = CU.weighted_sums(r["pixels"], np.ones(len(r["ref"])), r["S"].shape[1])
        assert S.tobytes() == r["S"].tobytes(), b


@pytest.mark.parametrize("knob", KNOBS)
def test_a_universe_is_the_oracles_fresh_run(knob):
    """weighted_sums of the oracle's nominal per-slot signals, the weights from segment_weights, against the oracle's sums of a
    fresh run under the patched constants within helpers.assert_wave_close (1e-5 |ref| + 1e-7 peak); the knob changes a hit
    count or an ADC code; the oracle's hits on both sums: the pixels whose hit count or a hit tick differs are left out and may
    be at most 2 % of the pixels with hits, the three batches together; on the others adc_list agrees at 1e-5 and the ADC
    codes are equal (the bars of test_fused_chain_vs_oracle_two_batches)"""
    seg, bid, resp = _module0_case()
    v = knobs()[knob]
    nominal = _nominal_runs()
    H.load_cfg("module0")
    n_has = n_out = 0
    changed = False
    for b in (0, 1, 2):
        nom = nominal[b]
        sb = seg[bid == b]
        fresh = _oracle_run(sb, resp, v, False)
        assert np.array_equal(fresh["upix"], nom["upix"]), (knob, b)
        w, n_k, unw = _twin_weights(v, sb, nom["ref"])
        assert n_k.tobytes() == fresh["ref"]["n_electrons"].astype(np.float64).tobytes() and unw == 0, (knob, b)
        S = CU.weighted_sums(nom["pixels"], w, nom["S"].shape[1])
        H.assert_wave_close(S, fresh["S"], what=f"{knob}, batch {b}")
        adc_u, ticks_u, digit_u = _oracle_hits(S)
        adc_f, ticks_f, digit_f = _oracle_hits(fresh["S"])
        adc_n, _, digit_n = _oracle_hits(nom["S"])
        changed = changed or not np.array_equal(adc_f != 0, adc_n != 0) or not np.array_equal(digit_f, digit_n)
        has = ((adc_u != 0) | (adc_f != 0)).any(axis=1)
        same = ((adc_u != 0).sum(axis=1) == (adc_f != 0).sum(axis=1)) & (ticks_u == ticks_f).all(axis=1)
        n_has += int(has.sum())
        n_out += int((has & ~same).sum())
        assert np.array_equal(adc_u[same] != 0, adc_f[same] != 0), (knob, b)
        np.testing.assert_allclose(adc_u[same], adc_f[same], rtol=1e-5, err_msg=f"{knob}, batch {b}")
        assert np.array_equal(digit_u[same], digit_f[same]), (knob, b)
    print(f"{knob}: {n_out} of {n_has} pixels with hits left out ({100 * n_out / max(n_has, 1):.2f} %)")
    assert changed, knob
    assert n_has > 100 and n_out <= MAX_LEFT_OUT * n_has, (knob, n_out, n_has)
