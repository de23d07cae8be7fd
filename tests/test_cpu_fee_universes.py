"""CPU: FEE universes -- the ctypes mirror of LdsimFeeVariation against the header text, the variations of
larndsim_amd/fee_universes.py (nominal, load, every refusal of the validation), the row conversion of the driver's two datasets
and the driver's argument checks.  No GPU."""
import ctypes as C
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import helpers as H
from larndsim_amd import abi, consts
from larndsim_amd import fee_universes as FU
from larndsim_amd.comm import HIT_ROW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")


def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_fee_universes", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_abi_variation_is_the_header_struct():
    """LdsimFeeVariation against the declaration in include/ldsim.h: 112 bytes, the fields in order at the offsets the C
    declaration gives them; the five entry points and the limit are declared"""
    text = open(os.path.join(REPO, "include", "ldsim.h")).read()
    body = re.search(r"typedef struct LdsimFeeVariation \{(.*?)\} LdsimFeeVariation;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        size = 8 if ctype == "double" else 4
        for n in names.split(","):
            off = (off + size - 1) // size * size
            fields.append((n.strip(), size, off))
            off += size
    assert off == 112 and C.sizeof(abi.LdsimFeeVariation) == 112
    assert [f[0] for f in fields] == [f[0] for f in abi.LdsimFeeVariation._fields_]
    for name, size, o in fields:
        d = getattr(abi.LdsimFeeVariation, name)
        assert (d.offset, d.size) == (o, size), name
    assert tuple(f[0] for f in fields[:-1]) == FU.FIELDS and fields[-1][0] == "pad"
    assert int(re.search(r"#define LDSIM_FEE_UNIVERSES_MAX (\d+)", text).group(1)) == abi.FEE_UNIVERSES_MAX == FU.MAX_UNIVERSES == 64
    for fn in ("ldsim_fee_variation_nominal", "ldsim_chain_fee_universes", "ldsim_chain_fee_universe_download",
               "ldsim_chain_fee_universe_hits_download", "ldsim_chain_fee_universes_ms"):
        assert f"int {fn}(" in text, fn
    assert re.search(r"#define LDSIM_ABI_VERSION 8\b", text)


def test_nominal_is_the_constants_and_pack_round_trips():
    H.load_cfg("module0", noise_zero=False)
    try:
        det = consts.detector
        v = FU.nominal()
        assert set(v) == set(FU.FIELDS) and len(FU.FIELDS) == 15
        for f in FU.FIELDS:
            if f in FU.TABLE_DEFAULTS:
                assert v[f] == FU.TABLE_DEFAULTS[f]
            else:
                assert v[f] == getattr(det, f.upper()), f
        assert (v["threshold_table_scale"], v["threshold_table_offset"], v["gain_table_scale"]) == (1.0, 0.0, 1.0)
        assert FU.is_noisy(v) and v["reset_noise_charge"] > 0
        c = abi.pack_consts()
        for f in FU.FIELDS:
            if f not in FU.TABLE_DEFAULTS:
                assert v[f] == getattr(c, f), f
        arr = FU.pack([v, FU.variation(v, gain=0.005, ADC_HOLD_DELAY=3)])
        assert FU.unpack(arr[0]) == v and arr[0].pad == 0
        w = FU.unpack(arr[1])
        assert w["gain"] == 0.005 and w["adc_hold_delay"] == 3 and {k: x for k, x in w.items() if k not in ("gain", "adc_hold_delay")} \
            == {k: x for k, x in v.items() if k not in ("gain", "adc_hold_delay")}
        H.load_cfg("module0")
        assert not FU.is_noisy(FU.nominal())
        with pytest.raises(ValueError, match="unknown key 'TIME_SAMPLING'"):
            FU.variation(TIME_SAMPLING=0.05)
    finally:
        H.load_cfg("module0")


def test_load_round_trip_and_unknown_keys(tmp_path):
    H.load_cfg("module0")
    det = consts.detector
    path = str(tmp_path / "u.json")
    with open(path, "w") as f:
        json.dump([{"name": "nominal"}, {"name": "low", "DISCRIMINATION_THRESHOLD": 3500.0, "ADC_BUSY_DELAY": 4},
                   {"RESET_NOISE_CHARGE": 100.0, "THRESHOLD_TABLE_SCALE": 1.2}], f)
    names, vs = FU.load(path)
    assert names == ["nominal", "low", "universe2"]
    assert vs[0] == FU.nominal()
    assert vs[1] == FU.variation(discrimination_threshold=3500.0, adc_busy_delay=4) and vs[1]["gain"] == det.GAIN
    assert vs[2]["reset_noise_charge"] == 100.0 and vs[2]["threshold_table_scale"] == 1.2 and FU.is_noisy(vs[2])
    # what the file alone says about noise (the driver's early check)
    assert [FU.changes_noisy(c) for _, c in FU.read(path)] == [None, None, True]
    assert FU.changes_noisy({"RESET_NOISE_CHARGE": 0, "UNCORRELATED_NOISE_CHARGE": 0.0, "DISCRIMINATOR_NOISE": 0}) is False
    # dump -> load gives the same names and variations
    again = str(tmp_path / "again.json")
    FU.dump(again, names, vs)
    assert FU.load(again) == (names, vs)
    rows = FU.universe_rows(names, vs)
    assert rows.dtype == FU.FILE_UNIVERSE and rows["index"].tolist() == [0, 1, 2] and rows["name"][1] == b"low"
    assert len(FU.FILE_UNIVERSE.names) == 2 + 15
    for f in FU.FIELDS:
        assert rows[f].tolist() == [v[f] for v in vs], f
    for bad, word in (([{"name": "x", "TIME_SAMPLING": 0.05}], "unknown key 'TIME_SAMPLING'"),
                      ([{"name": "x", "MAX_ADC_VALUES": 10}], "unknown key"), ([{"name": "x", "threshold": 1}], "unknown key"),
                      ([], r"must lie in \[1, 64\]"), ([{}] * 65, r"must lie in \[1, 64\]"), ({"name": "x"}, "JSON list"),
                      ([{"name": "x", "GAIN": "high"}], "not finite")):
        with open(path, "w") as f:
            json.dump(bad, f)
        with pytest.raises(ValueError, match=word):
            FU.load(path)


def test_every_refusal_of_the_validation():
    H.load_cfg("module0")
    n = FU.nominal()
    dt = consts.detector.TIME_SAMPLING
    assert FU.validate([n]) == [n] and FU.validate([n] * 64)
    for count in (0, 65):
        with pytest.raises(ValueError, match=r"n = \d+ universes, must lie in \[1, 64\]"):
            FU.validate([n] * count)
    for f in FU.FLOAT_FIELDS:
        for x in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match=rf"universe 1: {f} = .* is not finite"):
                FU.validate([n, dict(n, **{f: x})])
    with pytest.raises(ValueError, match="universe 0: v_ref == v_cm"):
        FU.validate([dict(n, v_ref=n["v_cm"])])
    for f in FU.INT_FIELDS:
        with pytest.raises(ValueError, match=f"negative {f}"):
            FU.validate([dict(n, **{f: -1})])
        with pytest.raises(ValueError, match="not an integer"):
            FU.validate([dict(n, **{f: 1.5})])
        assert FU.validate([dict(n, **{f: 0})])
    for f in FU.NOISE_FIELDS:
        with pytest.raises(ValueError, match=f"negative noise charge {f}"):
            FU.validate([dict(n, **{f: -0.5})])
    # the rise time the kernels hold taps for: 10 * rt / dt <= 62
    assert FU.validate([dict(n, buffer_risetime=6.0 * dt), dict(n, buffer_risetime=0.0)])
    with pytest.raises(ValueError, match="exceeds the kernel's 62 taps"):
        FU.validate([dict(n, buffer_risetime=6.21 * dt)])
    with pytest.raises(ValueError, match="exceeds the kernel's 62 taps"):
        FU.validate([dict(n, buffer_risetime=6.0 * dt)], time_sampling=0.5 * dt)
    with pytest.raises(ValueError, match="missing fields"):
        FU.validate([{k: x for k, x in n.items() if k != "gain"}])
    with pytest.raises(ValueError, match="unknown key"):
        FU.validate([dict(n, clock_cycle=0.1)])


def test_file_rows_map_batches_to_events_universe_after_universe():
    hr0 = np.zeros(3, dtype=HIT_ROW)
    hr0["batch"], hr0["pixel"], hr0["adc"], hr0["slot"], hr0["tick"] = [0, 0, 2], [11, 11, 40], [70, 71, 90], [0, 1, 0], [5.5, 25.5, 7.0]
    hr1 = np.zeros(1, dtype=HIT_ROW)
    hr1["batch"], hr1["pixel"], hr1["adc"], hr1["slot"], hr1["tick"] = [1], [12], [99], [0], [100.25]
    us = [dict(hit_rows=hr0, hit_charge=np.array([1e4, 2e4, 3e4])), dict(hit_rows=hr0[:0], hit_charge=np.zeros(0)),
          dict(hit_rows=hr1, hit_charge=np.array([5e3]))]
    rows = FU.file_rows(us, event_of_batch=[7, 7, 9])
    assert rows.dtype == FU.FILE_HIT
    assert FU.FILE_HIT.descr == [("universe", "<u2"), ("event_id", "<u4"), ("pixel_id", "<i4"), ("slot", "<i4"), ("adc", "<i4"),
                                 ("tick", "<f8"), ("charge", "<f8")]
    assert rows["universe"].tolist() == [0, 0, 0, 2] and rows["event_id"].tolist() == [7, 7, 9, 7]
    assert rows["pixel_id"].tolist() == [11, 11, 40, 12] and rows["slot"].tolist() == [0, 1, 0, 0]
    assert rows["adc"].tolist() == [70, 71, 90, 99] and rows["tick"].tolist() == [5.5, 25.5, 7.0, 100.25]
    assert rows["charge"].tolist() == [1e4, 2e4, 3e4, 5e3]
    assert len(FU.file_rows([], [0])) == 0 and FU.file_rows([], [0]).dtype == FU.FILE_HIT
    with pytest.raises(ValueError, match="3 hit rows, 2 charges"):
        FU.file_rows([dict(hit_rows=hr0, hit_charge=np.zeros(2))], [0, 0, 0])


def test_cli_fee_universes_argument_checks(tmp_path, monkeypatch, capsys):
    """--n_gpus 2 is refused, noisy universes without --rng keyed are refused by the argument check (it says so), an unknown key
    or an unreadable file is an argument error, and the help text says that packets per universe are out of scope"""
    cli = _cli()
    base = ["--input_filename", "x.npy", "--output_filename", str(tmp_path / "y.npz")]
    assert cli._parse_args(base).fee_universes is None
    quiet, noisy, unknown = (str(tmp_path / n) for n in ("quiet.json", "noisy.json", "unknown.json"))
    json.dump([{"name": "nominal"}, {"name": "low", "DISCRIMINATION_THRESHOLD": 3500.0}], open(quiet, "w"))
    json.dump([{"name": "nominal"}, {"name": "loud", "DISCRIMINATOR_NOISE": 900.0}], open(noisy, "w"))
    json.dump([{"name": "x", "CLOCK_CYCLE": 0.2}], open(unknown, "w"))
    assert cli._parse_args(base + ["--fee_universes", quiet]).fee_universes == quiet
    assert cli._parse_args(base + ["--fee_universes", noisy, "--rng", "keyed"]).fee_universes == noisy
    for args, word in ((["--fee_universes", noisy], "universe 1 (loud) has a non-zero noise charge"),
                       (["--fee_universes", noisy, "--rng", "table"], "give --rng keyed as well"),
                       (["--fee_universes", unknown], "unknown key 'CLOCK_CYCLE'"),
                       (["--fee_universes", str(tmp_path / "missing.json")], "missing.json")):
        with pytest.raises(SystemExit):
            cli._parse_args(base + args)
        assert word in capsys.readouterr().err.replace("\n", " ").replace("  ", " "), word
    help_text = " ".join(cli._parser().format_help().split())
    assert "--fee_universes FILE.json" in help_text and "packets per universe are out of scope" in help_text
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    with pytest.raises(SystemExit, match="--fee_universes is not available with --n_gpus > 1"):
        cli.launch_ranks_if_asked(base + ["--fee_universes", quiet, "--n_gpus", "2"])
    assert cli.launch_ranks_if_asked(base + ["--fee_universes", quiet]) is None
    with pytest.raises(ValueError, match="universe 1 .loud. has a non-zero noise charge.*--rng keyed"):
        cli.run_simulation("x.npy", str(tmp_path / "y.npz"), fee_universes=noisy)
    with pytest.raises(ValueError, match="--fee_universes is not available with --n_gpus > 1"):
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("RANK", "0")
        cli.run_simulation("x.npy", str(tmp_path / "y.npz"), n_gpus=2, fee_universes=quiet)
