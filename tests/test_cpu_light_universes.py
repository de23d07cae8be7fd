"""CPU: light universes -- the ctypes mirror of LdsimLightVariation against the header text, the variations of
larndsim_amd/light_universes.py (nominal, every refusal of validate and parse), the driver's argument checks, and the definition
of a universe stated in numpy (``scaled_input``, ``scintillation_table`` / ``response_table``, ``convolve``) against the oracle's
``scintillation_effect`` and ``light_detector_response`` under patched ``consts.light``, bit for bit, on a small random photon
sum: "universe = the oracle under those constants on the scaled input" is what the documents say.  The host statement of the
Poisson rule (``poisson_counts``) is held against a scalar restatement with libm's exp under the bar the GPU test uses.  No GPU."""
import ctypes as C
import importlib.util
import json
import math
import os
import re
import sys

import numpy as np
import pytest

import helpers as H
from larndsim_amd import abi, consts
from larndsim_amd import light_universes as LU
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")


def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_light_universes", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


# ---- 1. the struct, nominal, the refusals -----------------------------------------------------------------------------------------
def test_abi_variation_is_the_header_struct():
    """LdsimLightVariation against the declaration in include/ldsim.h: seven doubles, 56 bytes, in order; the entry points are
    declared; the other variation structs and the ABI version are what they were"""
    text = open(os.path.join(REPO, "include", "ldsim.h")).read()
    body = re.search(r"typedef struct LdsimLightVariation \{(.*?)\} LdsimLightVariation;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        size = 8 if ctype == "double" else 4
        for n in names.split(","):
            off = (off + size - 1) // size * size
            fields.append((n.strip(), size, off))
            off += size
    assert off == 56 and C.sizeof(abi.LdsimLightVariation) == 56 and len(fields) == 7
    assert [f[0] for f in fields] == [f[0] for f in abi.LdsimLightVariation._fields_]
    for name, size, o in fields:
        d = getattr(abi.LdsimLightVariation, name)
        assert (d.offset, d.size) == (o, size), name
    assert tuple(f[0] for f in fields) == LU.C_FIELDS and LU.FIELDS == LU.C_FIELDS + ("trig_threshold_scale", "noise_scale")
    assert len(LU.FIELDS) == 9
    for fn in ("ldsim_light_variation_nominal", "ldsim_dev_light_universes", "ldsim_dev_light_universe_download",
               "ldsim_dev_light_universe_triggers", "ldsim_dev_light_universe_waveforms", "ldsim_light_universes_ms"):
        assert f"int {fn}(" in text, fn
    assert re.search(r"#define LDSIM_ABI_VERSION 8\b", text) and abi.ABI_VERSION == 8
    assert re.search(r"#define LDSIM_LIGHT_UNIVERSES_MAX 64\b", text) and LU.MAX_UNIVERSES == abi.LIGHT_UNIVERSES_MAX == 64
    assert C.sizeof(abi.LdsimFeeVariation) == 112 and C.sizeof(abi.LdsimChargeVariation) == 56


def test_module_imports_the_standard_library_only():
    """the driver's self-launching parent reads a universes file before numpy is loaded"""
    code = ("import sys; sys.path.insert(0, %r); import larndsim_amd.light_universes as m; "
            "assert 'numpy' not in sys.modules, 'numpy loaded'; print(len(m.FIELDS))") % os.path.join(REPO, "larnd-sim_amd")
    import subprocess
    r = subprocess.run([sys.executable, "-S", "-c", code], capture_output=True)
    assert r.returncode == 0 and r.stdout.strip() == b"9", r.stderr.decode()[-800:]


def test_nominal_is_the_constants_and_pack_round_trips():
    H.load_cfg("module0")
    light = consts.light
    v = LU.nominal()
    assert tuple(v) == LU.FIELDS
    assert v == dict(photon_scale=1.0, singlet_fraction=light.SINGLET_FRACTION, tau_s=light.TAU_S, tau_t=light.TAU_T,
                     gain_scale=1.0, response_time=light.LIGHT_RESPONSE_TIME, oscillation_period=light.LIGHT_OSCILLATION_PERIOD,
                     trig_threshold_scale=1.0, noise_scale=1.0)
    w = LU.variation(v, TAU_S=0.002, photon_scale=0.5, Light_Gain_Scale=-1, NOISE_SCALE=0.0, trig_threshold_scale=2.0,
                     light_response_time=0.07, LIGHT_OSCILLATION_PERIOD=0.08, singlet_fraction=0.2, tau_t=0.6)
    assert w == dict(photon_scale=0.5, singlet_fraction=0.2, tau_s=0.002, tau_t=0.6, gain_scale=-1, response_time=0.07,
                     oscillation_period=0.08, trig_threshold_scale=2.0, noise_scale=0.0) and v["tau_s"] == light.TAU_S
    for bad in ("W_PH", "gain_scale", "LIGHT_GAIN", "response_time", "LIGHT_NBIT", "LIGHT_WINDOW"):
        with pytest.raises(ValueError, match=f"light universes: unknown key '{bad}'"):
            LU.variation(**{bad: 1.0})
    arr = LU.pack([v, w])
    assert len(arr) == 2 and LU.unpack(arr[0]) == v and LU.unpack(arr[1], w) == w
    assert LU.unpack(arr[1]) == dict(w, trig_threshold_scale=1.0, noise_scale=1.0)
    rows = LU.universe_rows(["a", "b"], [v, w])
    assert rows.dtype == LU.FILE_UNIVERSE and rows.dtype.names == ("name",) + LU.FIELDS
    assert rows["name"].tolist() == [b"a", b"b"] and rows["tau_s"].tolist() == [light.TAU_S, 0.002]
    assert rows["noise_scale"].tolist() == [1.0, 0.0]
    t = LU.file_rows(3, 7, 0.25, np.array([5, 900]), np.array([0, 0]), np.arange(96).reshape(2, 48))
    assert t.dtype.names == LU.FILE_TRIG.names + ("op_channel",) and t["op_channel"].shape == (2, 48)
    assert t["universe"].tolist() == [3, 3] and t["event_id"].tolist() == [7, 7] and t["trigger_idx"].tolist() == [5, 900]
    assert t["start_time"].tolist() == [0.25, 0.25] and t["op_channel"][1, 0] == 48
    with pytest.raises(ValueError, match="2 triggers, op_channel of shape"):
        LU.file_rows(0, 0, 0.0, np.array([1, 2]), np.array([0, 0]), np.arange(48))


def test_validate_refuses():
    H.load_cfg("module0")
    n = LU.nominal()
    assert LU.validate([n] * 64)
    for vs, word in (([], r"n = 0 universes, must lie in \[1, 64\]"), ([n] * 65, r"n = 65 universes"),
                     ([n, {k: x for k, x in n.items() if k != "tau_t"}], "universe 1: missing fields .'tau_t'."),
                     ([dict(n, w_ph=0.5)], "universe 0: .*unknown key .'w_ph'."),
                     ([n, dict(n, photon_scale=0.0)], "universe 1: photon_scale = 0.0 must be finite and > 0"),
                     ([dict(n, photon_scale=-2.0)], "universe 0: photon_scale = -2.0 must be finite and > 0"),
                     ([dict(n, singlet_fraction=1.5)], r"universe 0: singlet_fraction = 1.5 must be finite and in \[0, 1\]"),
                     ([dict(n, singlet_fraction=-0.1)], "universe 0: singlet_fraction = -0.1"),
                     ([dict(n, tau_s=0)], "universe 0: tau_s = 0 must be finite and > 0"),
                     ([dict(n, tau_t=-1.0)], "universe 0: tau_t = -1.0 must be finite and > 0"),
                     ([dict(n, gain_scale=0.0)], "universe 0: gain_scale = 0.0 must be finite and != 0"),
                     ([dict(n, noise_scale=-0.5)], "universe 0: noise_scale = -0.5 must be finite and >= 0")):
        with pytest.raises(ValueError, match=word):
            LU.validate(vs)
    assert LU.validate([dict(n, singlet_fraction=0), dict(n, singlet_fraction=1), dict(n, gain_scale=-1.0),
                        dict(n, trig_threshold_scale=-3.0), dict(n, trig_threshold_scale=0.0), dict(n, noise_scale=0.0)])
    for f in LU.FIELDS:
        for x in (float("nan"), float("inf"), -float("inf"), "1", None, True):
            with pytest.raises(ValueError, match=f"universe 2: {f} = .* must be finite"):
                LU.validate([n, n, dict(n, **{f: x})])
    # the RLC constants: > 0 under model 0; under model 1 (module0's) they are not read, and a changed value is refused
    assert int(consts.light.SIPM_RESPONSE_MODEL) == 1
    for f in ("response_time", "oscillation_period"):
        with pytest.raises(ValueError, match=f"universe 0: {f} = .* is not read under SIPM_RESPONSE_MODEL 1 and differs"):
            LU.validate([dict(n, **{f: n[f] * 1.2})])
        assert LU.validate([dict(n, **{f: n[f] * 1.2})], sipm_response_model=0)
        with pytest.raises(ValueError, match=f"universe 0: {f} = 0.0 must be finite and > 0"):
            LU.validate([dict(n, **{f: 0.0})], sipm_response_model=0)


def test_parse_refuses(tmp_path):
    H.load_cfg("module0")
    got = LU.parse([{"name": "a"}, {"TAU_S": 2e-3, "photon_scale": 1.1}, {"name": "c", "NOISE_SCALE": 0}])
    assert got == [("a", {}), ("universe1", {"TAU_S": 2e-3, "photon_scale": 1.1}), ("c", {"NOISE_SCALE": 0})]
    for entries, word in (({}, "must hold a JSON list of objects"), ([1], "must hold a JSON list of objects"), ([], "n = 0 universes"),
                          ([{}] * 65, "n = 65 universes"), ([{}, {"W_PH": 2e-5}], "universe 1: unknown key 'W_PH'"),
                          ([{"LIGHT_NBIT": 12}], "universe 0: unknown key 'LIGHT_NBIT'"), ([{"GAIN": 4.0}], "unknown key 'GAIN'"),
                          ([{"ELECTRON_LIFETIME": 500.0}], "unknown key 'ELECTRON_LIFETIME'"),
                          ([{"name": "x" * 65}], "name longer than 64 bytes")):
        with pytest.raises(ValueError, match=word):
            LU.parse(entries)
    path = tmp_path / "u.json"
    json.dump([{"name": "nominal"}, {"name": "slow", "TAU_T": 0.9, "TRIG_THRESHOLD_SCALE": 0.5}], open(path, "w"))
    names, vs = LU.load(str(path))
    assert names == ["nominal", "slow"] and vs[0] == LU.nominal() and vs[1] == LU.variation(tau_t=0.9, trig_threshold_scale=0.5)
    LU.dump(str(path), names, vs)
    assert LU.load(str(path)) == (names, vs)
    json.dump([{"PHOTON_SCALE": -1.0}], open(path, "w"))
    with pytest.raises(ValueError, match="universe 0: photon_scale = -1.0 must be finite and > 0"):
        LU.load(str(path))
    json.dump([{"LIGHT_RESPONSE_TIME": 0.07}], open(path, "w"))
    with pytest.raises(ValueError, match="response_time = 0.07 is not read under SIPM_RESPONSE_MODEL 1"):
        LU.load(str(path))
    # the FEE and charge parsers keep refusing the light keys
    from larndsim_amd import charge_universes as CU
    from larndsim_amd import fee_universes as FU
    with pytest.raises(ValueError, match="unknown key 'TAU_S'"):
        FU.parse([{"TAU_S": 0.002}])
    with pytest.raises(ValueError, match="unknown key 'PHOTON_SCALE'"):
        CU.parse([{"PHOTON_SCALE": 1.2}])


def test_cli_light_universes_argument_checks(tmp_path, monkeypatch, capsys):
    """--light_universes is refused without --rng keyed, with --n_gpus > 1, with module variation, when light is not simulated,
    for an unreadable file and for an unknown key, each with the reason; --help names the option"""
    cli = _cli()
    base = ["--input_filename", "x.npy", "--output_filename", str(tmp_path / "y.npz")]
    assert cli._parse_args(base).light_universes is None
    good, unknown = (str(tmp_path / n) for n in ("good.json", "unknown.json"))
    json.dump([{"name": "nominal"}, {"name": "bright", "PHOTON_SCALE": 1.2}], open(good, "w"))
    json.dump([{"name": "x", "W_PH": 2e-5}], open(unknown, "w"))
    assert cli._parse_args(base + ["--light_universes", good, "--rng", "keyed"]).light_universes == good
    for args, word in ((["--light_universes", good], "--light_universes draws every universe's fluctuations"),
                       (["--light_universes", good, "--rng", "table"], "give --rng keyed as well"),
                       (["--light_universes", unknown, "--rng", "keyed"], "unknown key 'W_PH'"),
                       (["--light_universes", str(tmp_path / "missing.json"), "--rng", "keyed"], "missing.json"),
                       (["--light_universes", good, "--rng", "keyed", "--mod2mod_variation", "true"],
                        "--light_universes is not available with module variation"),
                       (["--light_universes", good, "--rng", "keyed", "--light_simulated", "false"],
                        "light is not simulated in this run")):
        with pytest.raises(SystemExit):
            cli._parse_args(base + args)
        assert word in capsys.readouterr().err.replace("\n", " ").replace("  ", " "), word
    help_text = " ".join(cli._parser().format_help().split())
    assert "--light_universes FILE.json" in help_text and "PHOTON_SCALE" in help_text and "TRIG_THRESHOLD_SCALE" in help_text
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    with pytest.raises(SystemExit, match="--light_universes is not available with --n_gpus > 1"):
        cli.launch_ranks_if_asked(base + ["--light_universes", good, "--rng", "keyed", "--n_gpus", "2"])
    assert cli.launch_ranks_if_asked(base + ["--light_universes", good, "--rng", "keyed"]) is None
    out = str(tmp_path / "y.npz")
    with pytest.raises(ValueError, match="--light_universes draws .* give --rng keyed as well"):
        cli.run_simulation("x.npy", out, light_universes=good)
    with pytest.raises(ValueError, match="unknown key 'W_PH'"):
        cli.run_simulation("x.npy", out, light_universes=unknown, rng="keyed")
    with pytest.raises(ValueError, match="missing.json"):
        cli.run_simulation("x.npy", out, light_universes=str(tmp_path / "missing.json"), rng="keyed")
    with pytest.raises(ValueError, match="--light_universes is not available with --n_gpus > 1"):
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("RANK", "0")
        cli.run_simulation("x.npy", out, n_gpus=2, light_universes=good, rng="keyed")


# ---- 2. the definition against the oracle ------------------------------------------------------------------------------------------
def _small_case(model):
    """module0 with a 40-tick window; a random photon sum [3][150] with stretches of zeros and one bright stretch"""
    H.load_cfg("module0")
    light = consts.light
    light.LIGHT_WINDOW = (0.01, 0.05)
    light.SIPM_RESPONSE_MODEL = model
    rs = np.random.default_rng(20241020)
    inc = (rs.random((3, 150)) * 400).astype(np.float32)
    inc[rs.random((3, 150)) < 0.4] = 0
    inc[1, 60:90] *= 300
    inc[2, :20] = 0
    return inc


@pytest.mark.parametrize("model", [0, 1])
def test_definition_equals_the_oracle_under_patched_constants(model):
    """steps 1, 2 and 4 of the definition (scaled input, scintillation under (singlet_fraction, tau_s, tau_t), detector response
    under (gain_scale, response_time, oscillation_period) or the impulse model) in numpy, against the oracle's own functions fed
    the scaled input under ``consts.light`` patched to the variation: bit for bit"""
    inc = _small_case(model)
    light = consts.light
    assert LU.conv_ticks() == 40
    nominal = LU.nominal()
    knobs = [dict(), dict(photon_scale=0.5), dict(photon_scale=50.0), dict(singlet_fraction=0.2), dict(tau_s=nominal["tau_s"] * 2),
             dict(tau_t=nominal["tau_t"] * 0.8), dict(gain_scale=1.1), dict(gain_scale=-1.0)]
    if model == 0:
        knobs += [dict(response_time=nominal["response_time"] * 1.2), dict(oscillation_period=nominal["oscillation_period"] * 0.9)]
    gain0 = np.asarray(light.LIGHT_GAIN, dtype=np.float64)
    for kn in knobs:
        H.load_cfg("module0")
        light.LIGHT_WINDOW, light.SIPM_RESPONSE_MODEL = (0.01, 0.05), model
        v = dict(nominal, **kn)
        LU.validate([v], reference=nominal)
        x = LU.scaled_input(inc, v["photon_scale"])
        if v["photon_scale"] == 1.0:
            assert np.array_equal(x, inc)
        gain = gain0[:3] * v["gain_scale"]
        sc = LU.convolve(x, LU.scintillation_table(v), skip_zero=True)
        rp = LU.convolve(sc, LU.response_table(v), gain=gain)
        # the oracle under the patched constants
        light.SINGLET_FRACTION, light.TAU_S, light.TAU_T = v["singlet_fraction"], v["tau_s"], v["tau_t"]
        light.LIGHT_RESPONSE_TIME, light.LIGHT_OSCILLATION_PERIOD = v["response_time"], v["oscillation_period"]
        o_sc = O.scintillation_effect(x)[0]
        o_rp = O.light_detector_response(o_sc, gain, light.IMPULSE_MODEL)[0]
        assert np.array_equal(sc, o_sc), kn
        assert np.array_equal(rp, o_rp) and np.abs(o_rp).max() > 0, kn
    H.load_cfg("module0")


def test_poisson_rule_on_the_oracles_scintillation_stays_inside_the_bar():
    """``poisson_counts`` (numpy's exp) on the oracle's scint_k of the photon_scale 50 universe against the rule restated element
    by element with libm's exp: fewer than 1e-3 of the values differ, each by exactly one count -- the bar the GPU test holds the
    device's counts to; both branches (mean < 30, mean >= 30) occur"""
    inc = _small_case(1)
    light = consts.light
    tick = light.LIGHT_TICK_SIZE
    sc = O.scintillation_effect(LU.scaled_input(inc, 50.0))[0]
    rs = np.random.default_rng(5)
    u = rs.random(sc.shape, dtype=np.float32)
    z = rs.standard_normal(sc.shape, dtype=np.float32)
    got = LU.poisson_counts(sc, u, z)
    mean = sc.astype(np.float64) * tick
    assert ((mean > 0) & (mean < 30)).sum() > 20 and (mean >= 30).sum() > 20
    want = np.zeros(sc.shape, dtype=np.float32)
    for idx in np.ndindex(sc.shape):
        m = float(mean[idx])
        if not sc[idx] > 0:
            continue
        if m < 30:
            k, p = 0, math.exp(-m)
            s = p
            while float(u[idx]) > s:
                k += 1
                p = p * m / k
                prev, s = s, s + p
                if s == prev:
                    break
        else:
            k = max(int(float(z[idx]) * math.sqrt(m) + m), 0)
        want[idx] = np.float32(1.0 / tick * float(k))
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bad = d != 0
    assert bad.mean() < 1e-3 and np.all(d[bad] == np.float32(1.0 / tick)), (bad.mean(), d[bad][:5])
    assert np.array_equal(got[sc <= 0], np.zeros((sc <= 0).sum(), dtype=np.float32)) and (got > 0).sum() > 100
    H.load_cfg("module0")
