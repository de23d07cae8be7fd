"""CPU: the track generator's host side (larndsim_amd/track_generator.py, cli/generate_segments.py) -- struct layouts against the
header text, the stopping power against a Bethe formula written out here, the deterministic range against a quadrature, energy
accounting, the scattering law, the keyed streams, the datasets through the driver's own readers, the refusals.  No GPU call.

Bounds.  Stopping power: the same f64 formula, only log / sqrt rounding differs: rtol 1e-12.  Its minimum: within 0.5 % of the
tabulated 1.508 MeV cm^2/g (these constants give 1.5069).  Range: sum(dx) against scipy's quadrature of 1 / S from t_min to T0;
measured at step 0.1 cm: +1.000e-3 cm (50 MeV), +8.22e-4 cm (100 MeV), +9.27e-4 cm (300 MeV) -- the last step's overshoot past
t_min dominates, the midpoint rule's own error is below 1e-4 cm --; the tolerance is twice each; at step 0.05 cm the deviations
are 6.63e-4, 6.08e-4 and 4.96e-4 cm and must be smaller.  Monte Carlo: 5 standard errors of the sample."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from larndsim_amd import abi, batching, consts, lib, rng, track_generator as TG

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "larnd-sim_amd", "cli", "generate_segments.py")
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
BIG = ([-1e4] * 3, [1e4] * 3)
CTYPE = {"double": C.c_double, "int32_t": C.c_int32}
RANGE_DEV_01 = {50.0: 1.000e-3, 100.0: 8.22e-4, 300.0: 9.27e-4}       # cm, measured at step 0.1 cm (module docstring)


@pytest.fixture(autouse=True)
def _cfg():
    H.load_cfg("module0")


def _struct_fields(name):
    hdr = open(os.path.join(REPO, "include", "ldsim.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for item in rest.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", item.strip())
            out.append((m.group(1), CTYPE[ctype] * int(m.group(2)) if m.group(2) else CTYPE[ctype]))
    return out


def test_struct_layouts_match_the_header():
    """1. sizes, offsets, entries, constants; the ABI version stays 8"""
    for name, cls, size in (("LdsimTrackGenParams", abi.LdsimTrackGenParams, 192), ("LdsimTrackGenPrimary", abi.LdsimTrackGenPrimary, 80)):
        fields = _struct_fields(name)
        assert [f for f, _ in fields] == [f for f, _ in cls._fields_], name
        for (f, t), (_, mine) in zip(fields, cls._fields_):
            if hasattr(t, "_length_"):
                assert (t._length_, t._type_) == (mine._length_, mine._type_), (name, f)
            else:
                assert t is mine, (name, f)
        assert C.sizeof(cls) == size
    p = abi.LdsimTrackGenParams
    assert [getattr(p, f).offset for f, _ in p._fields_] == [0, 24, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120, 128, 176, 180, 184, 188]
    q = abi.LdsimTrackGenPrimary
    assert [getattr(q, f).offset for f, _ in q._fields_] == [0, 24, 48, 56, 64, 68, 72, 76]
    assert TG.primary_dtype.itemsize == 80
    assert [TG.primary_dtype.fields[f][1] for f, _ in q._fields_] == [getattr(q, f).offset for f, _ in q._fields_]
    hdr = open(os.path.join(REPO, "include", "ldsim.h")).read()
    for entry in ("ldsim_track_gen_count", "ldsim_track_gen", "ldsim_track_gen_ms"):
        assert re.search(r"\bint " + entry + r"\(ldsim_ctx\* ctx", hdr), entry
        assert entry in lib.EXPORTS and hasattr(lib.load(), entry)
    for name, value in (("ME", TG.ELECTRON_MASS), ("M_MUON", TG.MASSES[13]), ("M_PION", TG.MASSES[211]),
                        ("M_PROTON", TG.MASSES[2212]), ("HARD_CAP", TG.HARD_CAP), ("HARD_TRIES", TG.HARD_TRIES),
                        ("STEP_BLOCKS", TG.STEP_BLOCKS), ("MAX_STEPS", TG.MAX_STEPS_LIMIT), ("NF64", len(TG.F64_COLUMNS)),
                        ("NI32", len(TG.I32_COLUMNS))):
        m = re.search(r"#define LDSIM_TRACK_GEN_" + name + r" (\S+)", hdr)
        assert m and float(m.group(1)) == value, name
    assert rng.TAG_GEN == TG.TAG_GEN == 7 and "RNG_TAG_GEN = 7" in open(os.path.join(REPO, "larnd-sim_amd", "csrc", "rng.h")).read()
    assert lib.load().ldsim_abi_version() == abi.ABI_VERSION == 8
    assert "#define LDSIM_ABI_VERSION 8" in hdr


def _bethe(T, M, rho):
    """PDG's mean stopping power with Sternheimer's density effect, written out independently (MeV cm^2 / g)"""
    me, K, ZA, I = 0.51099895, 0.307075, 18.0 / 39.948, 188e-6
    E = T + M
    gamma = E / M
    beta2 = 1.0 - 1.0 / gamma ** 2
    bg = math.sqrt(gamma ** 2 - 1.0)
    tmax = 2 * me * bg ** 2 / (1 + 2 * gamma * me / M + (me / M) ** 2)
    x = math.log10(bg)
    if x >= 3.0:
        delta = 2 * math.log(10) * x - 5.2146
    elif x >= 0.2:
        delta = 2 * math.log(10) * x - 5.2146 + 0.19559 * (3.0 - x) ** 3.0
    else:
        delta = 0.0
    return K * ZA / beta2 * (0.5 * math.log(2 * me * bg ** 2 * tmax / I ** 2) - beta2 - delta / 2)


def test_stopping_power_against_bethe_written_out_here():
    """2. 20 energies from 5 MeV to 100 GeV for each particle, rtol 1e-12 (the formula here forms beta^2 and beta gamma from
    gamma, the module from T / M; 1 - 1 / gamma^2 cancels at low T, 1e-16 / beta^2 = 1e-14 for 5 MeV protons: inside 1e-12)"""
    p = TG.params(world=BIG)
    for pdg in (13, -13, 211, -211, 2212):
        for T in np.geomspace(5.0, 1e5, 20):
            want = _bethe(float(T), TG.MASSES[abs(pdg)], p["density"])
            got = float(TG.stopping_power(T, pdg, p))
            assert abs(got - want) <= 1e-12 * want, (pdg, T, got, want)
            assert float(TG.restricted_stopping_power(T, pdg, p, t_cut=1e9)) == got        # Tc' = Tmax: the same number
            assert float(TG.restricted_stopping_power(T, pdg, p)) <= got
    T = np.geomspace(100.0, 1000.0, 4001)
    s = TG.stopping_power(T, 13, p)
    print(f"minimum of the muon stopping power: {s.min():.5f} MeV cm^2/g at T = {T[s.argmin()]:.1f} MeV")
    assert abs(s.min() - 1.508) <= 0.005 * 1.508
    assert 200 < T[s.argmin()] < 350
    tm = TG.tmax(1000.0, 13)
    g = 1000.0 / TG.MASSES[13] + 1
    assert abs(tm - 2 * 0.51099895 * (g * g - 1) / (1 + 2 * g * 0.51099895 / TG.MASSES[13] + (0.51099895 / TG.MASSES[13]) ** 2)) < 1e-10


@pytest.mark.parametrize("T0", [50.0, 100.0, 300.0])
def test_deterministic_range_against_quadrature(T0):
    """3. straggling and scattering off: a straight track whose length is the integral of 1 / S from t_min to T0.  Measured
    deviations at step 0.1 cm: +1.000e-3 (50 MeV), +8.22e-4 (100 MeV), +9.27e-4 cm (300 MeV); tolerance twice that; at step
    0.05 cm (6.63e-4, 6.08e-4, 4.96e-4 cm) the deviation must be smaller"""
    from scipy.integrate import quad
    dev = {}
    for step in (0.1, 0.05):
        p = TG.params(world=BIG, step=step, straggling=False, mcs=False)
        g = TG.generate_twin(TG.primaries(13, [0, 0, 0], [0, 0, 1], T0), p, 1)
        want = quad(lambda T: 1.0 / (float(TG.stopping_power(T, 13, p)) * p["density"]), p["t_min"], T0, epsabs=1e-12, epsrel=1e-12)[0]
        assert g["end_state"][0] == TG.STOPPED
        assert np.all(g["x_start"] == 0) and np.all(g["y_end"] == 0) and np.all(np.diff(g["z_end"]) > 0)      # exactly straight
        assert abs(g["z_end"][-1] - g["dx"].sum()) < 1e-9 and abs(g["path"][0] - g["dx"].sum()) < 1e-9
        dev[step] = g["dx"].sum() - want
        print(f"T0 {T0} MeV, step {step} cm: {g['counts'][0]} segments, range {g['dx'].sum():.6f} cm, quadrature {want:.6f} cm, "
              f"deviation {dev[step]:+.3e} cm")
    assert abs(dev[0.1]) <= 2 * RANGE_DEV_01[T0]
    assert abs(dev[0.05]) < abs(dev[0.1])


@pytest.mark.parametrize("straggling", [False, True])
def test_energy_accounting_of_stopped_walks(straggling):
    """4a. sum(dE) of every stopped walk equals T0 to rounding (some hundred additions of values <= T0: 1e-12 relative)"""
    p = TG.params(world=BIG, straggling=straggling)
    n = 64
    T0 = np.geomspace(30.0, 100.0, n)
    prim = TG.primaries(np.where(np.arange(n) % 2, 2212, 13), [0, 0, 0], [0, 0, 1], T0, event_id=np.arange(n) // 8,
                        track_in_event=np.arange(n) % 8)
    g = TG.generate_twin(prim, p, 5)
    assert (g["end_state"] == TG.STOPPED).all() and (g["end_energy"] == 0).all()
    tot = np.bincount(g["primary"], weights=g["dE"], minlength=n)
    assert np.all(np.abs(tot - T0) <= 1e-12 * T0)
    assert (g["dE"] >= 0).all() and (g["dx"] > 0).all() and (g["counts"] == np.bincount(g["primary"], minlength=n)).all()


def test_mean_deposit_of_single_steps():
    """4b. 2e5 single steps of 0.1 cm at 1 GeV, straggling on: soft + hard deposits average to the unrestricted Bethe mean"""
    n, h = 200_000, 0.1
    p = TG.params(world=BIG, step=h, max_steps=1, mcs=False)
    g = TG.generate_twin(TG.primaries(13, [0, 0, 0], [0, 0, 1], 1000.0, event_id=np.arange(n)), p, 11)
    assert (g["counts"] == 1).all() and (g["end_state"] == TG.TRUNCATED).all() and np.all(g["dx"] == h)
    want = float(TG.stopping_power(1000.0, 13, p)) * p["density"] * h
    se = g["dE"].std(ddof=1) / math.sqrt(n)
    print(f"mean deposit {g['dE'].mean():.6f} MeV, Bethe {want:.6f} MeV, standard error {se:.6f} MeV, "
          f"{int((g['dE'] > 0.1 + want).sum())} steps with a hard collision or more")
    assert abs(g["dE"].mean() - want) <= 5 * se
    assert g["dE"].max() > 1.0                     # hard collisions are there


def test_scattering_angle_after_100_steps():
    """5. energy loss off: after 100 steps of 0.1 cm the space angle's RMS is sqrt(2 100) theta0(h); 2e4 muons of 1 GeV.  The
    direction after 100 scatterings is that of segment 100 (max_steps 101)."""
    n, h = 20_000, 0.1
    p = TG.params(world=BIG, step=h, max_steps=101, energy_loss=False)
    g = TG.generate_twin(TG.primaries(13, [0, 0, 0], [0, 0, 1], 1000.0, event_id=np.arange(n)), p, 3)
    assert (g["counts"] == 101).all() and np.all(g["dE"] == 0)
    d = np.stack([(g[a + "_end"] - g[a + "_start"]) / g["dx"] for a in "xyz"], axis=1)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 1e-12
    last = d[g["step"] == 100]
    assert len(last) == n
    theta = np.arccos(np.clip(last[:, 2], -1, 1))
    rms, want = math.sqrt((theta ** 2).mean()), math.sqrt(200.0) * float(TG.highland_theta0(h, 1000.0, 13, p))
    print(f"space angle RMS {rms:.6e} rad, expected {want:.6e} rad ({rms / want - 1:+.3%}; bound {5 / math.sqrt(2 * n):.3%})")
    assert abs(rms / want - 1.0) <= 5.0 / math.sqrt(2 * n)
    for k in range(2):
        assert abs(last[:, k].mean()) <= 5 * last[:, k].std(ddof=1) / math.sqrt(n)
    assert abs(float(TG.highland_theta0(h, 1000.0, 13, p)) -
               13.6 / (1000.0 * (1000.0 + 2 * TG.MASSES[13]) / (1000.0 + TG.MASSES[13])) * math.sqrt(h / (19.55 / p["density"]))
               * (1 + 0.038 * math.log(h / (19.55 / p["density"]) / (1 - (TG.MASSES[13] / (1000.0 + TG.MASSES[13])) ** 2)))) < 1e-12


def _same_walk(a, ia, b, ib):
    ma, mb = a["primary"] == ia, b["primary"] == ib
    return all(np.array_equal(a[k][ma], b[k][mb]) for k in TG.F64_COLUMNS + ("step", "pdg_id", "event_id"))


def test_keyed_streams():
    """6. a primary's walk does not depend on what else is in the call; seeds differ; the sources are pure functions of the seed"""
    p = TG.params(world=BIG)
    mine = TG.primaries(13, [1, 2, 3], [0.3, -0.5, 0.8], 60.0, event_id=7, track_in_event=3)
    others = TG.primaries([2212, -211, 13], [0, 0, 0], [[1, 0, 0], [0, 1, 0], [1, 1, 1]], [40.0, 80.0, 35.0], event_id=[7, 8, 9],
                          track_in_event=[0, 3, 3])
    alone = TG.generate_twin(mine, p, 21)
    first = TG.generate_twin(np.concatenate([mine, others]), p, 21)
    last = TG.generate_twin(np.concatenate([others, mine]), p, 21)
    assert _same_walk(alone, 0, first, 0) and _same_walk(alone, 0, last, 3)
    assert not _same_walk(alone, 0, TG.generate_twin(mine, p, 22), 0)
    assert not _same_walk(first, 0, first, 3)                              # (event 9, track 3) is another stream
    w = TG.default_world()
    for make in (lambda s: TG.gun_primaries(13, [0, 0, 0], None, (30.0, 100.0), 4, 3, s),
                 lambda s: TG.cosmic_primaries(w, (1e3, 1e5), 4, 3, s)):
        a, b, c = make(5), make(5), make(6)
        assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
        assert len(a) == 12 and list(a["event_id"]) == [0] * 4 + [1] * 4 + [2] * 4 and list(a["track_in_event"]) == [0, 1, 2, 3] * 3
        assert np.allclose(np.sqrt((a["dir"] ** 2).sum(axis=1)), 1.0, atol=1e-12)
    cos = TG.cosmic_primaries(w, (1e3, 1e5), 1000, 1, 5)
    assert np.all(cos["pos"][:, 1] == w[1][1]) and (cos["dir"][:, 1] < 0).all()
    assert (cos["kinetic_energy"] >= 1e3).all() and (cos["kinetic_energy"] <= 1e5).all()
    # cos^2 zenith law: <cos theta> = 3/4, variance 3/5 - 9/16
    assert abs(-cos["dir"][:, 1].mean() - 0.75) <= 5 * math.sqrt((0.6 - 0.5625) / 1000)
    more = TG.gun_primaries(13, [0, 0, 0], None, (30.0, 100.0), 4, 1, 5, event_id0=1)
    assert more.tobytes() == TG.gun_primaries(13, [0, 0, 0], None, (30.0, 100.0), 4, 3, 5)[4:8].tobytes()


def _sp_cli():
    spec = importlib.util.spec_from_file_location("sp_cli_track_generator", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_tool_output_through_the_drivers_readers(tmp_path):
    """7. --twin writes an .npz that load_input / prepare_tracks / attach_event_times accept; ids, times and the frame"""
    out = str(tmp_path / "gen.npz")
    b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)
    c = b[0].mean(axis=1)
    r = subprocess.run([sys.executable, TOOL, "--config", "module0", "--source", "gun", "--pdg", "13", "--energy", "40", "--position",
                        str(c[2]), str(c[1]), str(c[0]), "--isotropic", "--tracks_per_event", "3", "--n_events", "2", "--seed", "4",
                        "--twin", "--output", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "6 primaries in 2 events" in r.stdout and "6 stopped, 0 left the world box, 0 truncated" in r.stdout
    cli = _sp_cli()
    H.load_cfg("module0")
    seg, truth = cli.load_input(out)
    assert seg.dtype == TG.to_datasets(TG.primaries(13, [0, 0, 0], [0, 0, 1], 1.0)[:0], TG.generate_twin(
        TG.primaries(13, [0, 0, 0], [0, 0, 1], 1.0)[:0], TG.params(world=BIG)))[0].dtype
    assert set(truth) == {"trajectories", "vertices"}
    traj, vert = truth["trajectories"], truth["vertices"]
    assert len(traj) == 6 and len(vert) == 2 and list(vert["event_id"]) == [0, 1] and list(vert["n_primaries"]) == [3, 3]
    assert np.array_equal(seg["segment_id"], np.arange(len(seg)))
    assert np.array_equal(traj["traj_id"], np.arange(6)) and seg["traj_id"].max() == 5
    assert np.array_equal(traj["event_id"][seg["traj_id"]], seg["event_id"])
    assert np.array_equal(seg["traj_id"], seg["file_traj_id"]) and np.array_equal(vert["event_id"][seg["vertex_id"]], seg["event_id"])
    assert np.array_equal(np.bincount(seg["traj_id"], minlength=6), traj["n_segments"])
    assert (seg["pdg_id"] == 13).all() and (seg["n_electrons"] == 0).all() and (seg["n_photons"] == 0).all()
    assert (seg["pixel_plane"] == 0).all() and (seg["long_diff"] == 0).all() and (seg["tran_diff"] == 0).all()
    for i in range(6):
        m = seg["traj_id"] == i
        assert np.all(np.diff(seg["t"][m].astype(np.float64)) > 0) and np.all(seg["t_end"][m] >= seg["t_start"][m])
        assert abs(float(seg["dE"][m].astype(np.float64).sum()) - 40.0) < 1e-3             # f4 columns
    np.testing.assert_allclose(seg["dEdx"], seg["dE"] / seg["dx"], rtol=1e-5)
    tracks = cli.prepare_tracks(seg.copy())
    lo, hi = np.sort(b[0], axis=-1)[:, 0], np.sort(b[0], axis=-1)[:, 1]
    for k, a in enumerate("xyz"):
        assert (tracks[a] >= lo[k]).all() and (tracks[a] <= hi[k]).all(), a
    cli.attach_event_times(truth, np.array([10.0, 20.0]), consts.sim)
    assert list(truth["vertices"]["t_event"]) == [10.0, 20.0]
    again = str(tmp_path / "again.npz")
    r2 = subprocess.run([sys.executable, TOOL, "--source", "gun", "--energy", "40", "--position", str(c[2]), str(c[1]), str(c[0]),
                         "--isotropic", "--tracks_per_event", "3", "--n_events", "2", "--seed", "4", "--twin", "--output", again],
                        capture_output=True, text=True)
    assert r2.returncode == 0
    seg2 = np.load(again)["segments"]                   # (field by field: the padding bytes of an aligned record are not data)
    assert seg2.dtype == seg.dtype and all(np.array_equal(seg2[f], seg[f]) for f in seg.dtype.names)
    bad = subprocess.run([sys.executable, TOOL, "--source", "gun", "--pdg", "11", "--twin", "--output", again], capture_output=True,
                         text=True)
    assert bad.returncode == 2 and "unknown pdg 11" in bad.stderr


def test_refusals_name_what_is_wrong():
    """8. the Python layer refuses what the C-ABI refuses"""
    for kw, what in (({"step": 0.0}, "step"), ({"step": math.nan}, "step"), ({"min_step": -1.0}, "min_step"),
                     ({"min_step": 1.0}, "exceeds step"), ({"max_loss_fraction": 0.0}, "max_loss_fraction"),
                     ({"max_loss_fraction": 2.0}, "max_loss_fraction"), ({"t_cut": math.inf}, "t_cut"), ({"t_min": 0.0}, "t_min"),
                     ({"t_cut": 188e-6}, "mean excitation"), ({"t_cut": 1e-4}, "mean excitation"), ({"density": 0.0}, "density"),
                     ({"t_min": 0.01}, "stopping power"), ({"max_steps": 0}, "max_steps"), ({"max_steps": TG.MAX_STEPS_LIMIT + 1}, "max_steps"),
                     ({"world": ([0, 0, 0], [1, 0, 1])}, "empty or inverted"), ({"world": ([0, 0, 2], [1, 1, 1])}, "empty or inverted")):
        with pytest.raises(TG.TrackGenError, match=what):
            TG.params(**dict({"world": BIG}, **kw))
    p = TG.params(world=([0, 0, 0], [10, 10, 10]))
    ok = dict(pdg=13, pos=[5, 5, 5], direction=[0, 0, 1], kinetic_energy=50.0)
    for kw, what in (({"pdg": 11}, "unknown pdg 11"), ({"pdg": -2212}, "unknown pdg"), ({"pos": [5, 5, 11]}, "outside the world box"),
                     ({"pos": [math.nan, 5, 5]}, "outside the world box"), ({"direction": [0, 0, 0]}, "zero direction"),
                     ({"kinetic_energy": 0.0}, "kinetic energy"), ({"kinetic_energy": math.inf}, "kinetic energy")):
        with pytest.raises(TG.TrackGenError, match=what):
            TG.generate_twin(TG.primaries(**dict(ok, **kw)), p, 0)
    with pytest.raises(TG.TrackGenError, match="primary 1"):
        TG.generate_twin(TG.primaries([13, 11], [5, 5, 5], [0, 0, 1], 50.0), p, 0)
    g = TG.generate_twin(TG.primaries(13, [5, 5, 10], [0, 0, 1], 50.0), p, 0)      # on the wall, heading out: one empty segment
    assert g["counts"][0] == 1 and g["end_state"][0] == TG.EXITED and g["dx"][0] == 0 and g["dEdx"][0] == 0
