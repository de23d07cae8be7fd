"""GPU: the track generator (csrc/kernels_trackgen.hip: gen_kernel) against its numpy twin (larndsim_amd/track_generator.py
generate_twin), against analytic values, at its limits and through the chain that reads its file.

Bounds.  Kernel and twin do the same f64 operations in the same order on the same keyed draws; they differ in the last bit of
log / log10 / pow / exp / sqrt / cos / sin.  Some hundred steps of a few ulp on magnitudes <= 1e3 give 1e-10, the columns are held
to 1e-6 cm / MeV (times: relative to their magnitude).  A comparison decided by that last bit can change a walk's length: such
primaries are counted, the cap is 1 in 10^4 -- none of 2048 --, the seed is one for which the twin in f64 and in longdouble agree on
every walk (track_gen_cases.SEED1), and the number found is printed.  Monte Carlo: 5 standard errors, as on the host.
Shapes: 2048 primaries (eight workgroups of 256 at group 256, partial groups at 1000, one group at 4096), odd counts for the
halves (1000 + 1048), walks of 100 to 400 steps."""
import ctypes as C
import functools
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import track_gen_cases as TC
from larndsim_amd import abi, consts, lib, synth, track_generator as TG

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "larnd-sim_amd", "cli", "generate_segments.py")
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
BIG = ([-1e4] * 3, [1e4] * 3)
COLUMNS = TG.F64_COLUMNS + TG.I32_COLUMNS + ("counts", "end_state", "end_pos", "end_time", "path", "end_energy")


@pytest.fixture(autouse=True)
def _cfg():
    H.load_cfg("module0")
    lib.context()
    yield
    lib.set_option("track_gen_group_primaries", 0)


@functools.lru_cache(maxsize=None)
def _twin1():
    H.load_cfg("module0")
    return TG.generate_twin(TC.mixed_primaries(), TC.params1(), TC.SEED1)


@functools.lru_cache(maxsize=None)
def _gpu1():
    H.load_cfg("module0")
    return TG.generate(TC.mixed_primaries(), TC.params1(), TC.SEED1)


@functools.lru_cache(maxsize=None)
def _differing():
    return TC.compare(_gpu1(), _twin1(), "kernel against twin")


def _same_bytes(a, b, what, keys=COLUMNS):
    for k in keys:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def test_kernel_against_twin():
    """1. 2048 mixed primaries, straggling and scattering on: counts and end states equal, every column within 1e-6"""
    got, exp = _gpu1(), _twin1()
    differ = _differing()
    assert differ <= TC.N1 // 10_000
    assert set(np.unique(exp["end_state"])) == {TG.STOPPED, TG.EXITED}           # both ends occur
    assert got["counts"].min() >= 50 and got["counts"].max() <= 500
    assert np.array_equal(got["primary"], np.repeat(np.arange(TC.N1), got["counts"]))
    assert np.array_equal(got["step"], np.concatenate([np.arange(c) for c in got["counts"]]))
    stopped = got["end_state"] == TG.STOPPED
    tot = np.bincount(got["primary"], weights=got["dE"], minlength=TC.N1)
    T0 = TC.mixed_primaries()["kinetic_energy"]
    assert np.all(np.abs(tot - T0)[stopped] <= 1e-12 * T0[stopped])
    assert np.allclose(tot + got["end_energy"], T0, rtol=1e-12, atol=0)


def test_determinism():
    """2. byte-identical arrays at three group sizes, in one call and in two halves, on two contexts, in two calls in a row"""
    prim, p, ref = TC.mixed_primaries(), TC.params1(), _gpu1()
    _same_bytes(TG.generate(prim, p, TC.SEED1), ref, "second call")
    for group in (64, 256, 1000, 4096):
        lib.set_option("track_gen_group_primaries", group)
        _same_bytes(TG.generate(prim[::-1].copy(), p, TC.SEED1), TG.generate(prim[::-1].copy(), p, TC.SEED1), f"group {group}, reversed")
        _same_bytes(TG.generate(prim, p, TC.SEED1), ref, f"group {group}")
    lib.set_option("track_gen_group_primaries", 0)
    a, b = TG.generate(prim[:1000], p, TC.SEED1), TG.generate(prim[1000:], p, TC.SEED1)
    for k in COLUMNS:
        joined = np.concatenate([a[k], b[k] + 1000 if k == "primary" else b[k]])
        assert joined.tobytes() == np.asarray(ref[k]).tobytes(), ("two halves", k)
    h = C.c_void_p()
    c = abi.pack_consts()
    lib.check(lib.load().ldsim_ctx_create(C.c_int(0), C.byref(c), C.byref(h)))
    try:
        _same_bytes(TG.generate(prim, p, TC.SEED1, ctx=h), ref, "second context")
    finally:
        lib.check(lib.load().ldsim_ctx_destroy(h))
    assert not np.array_equal(TG.generate(prim, p, TC.SEED1 + 1)["counts"], ref["counts"])
    for name, value in (("track_gen_group_primaries", 32), ("track_gen_group_primaries", 100.5)):
        with pytest.raises(lib.LdsimError, match=name):
            lib.set_option(name, value)


def _raw(ctx, prim, p, seed=1, capacity=None, count_only=False, **override):
    """the entries straight through ctypes: (status, message, n_segments, f64 columns, i32 columns)"""
    P = TG._pack(p)
    for k, v in override.items():
        if k in ("world_lo", "world_hi", "sternheimer"):
            getattr(P, k)[:] = v
        else:
            setattr(P, k, v)
    prim = np.ascontiguousarray(prim, dtype=TG.primary_dtype)
    n = len(prim)
    if count_only:
        counts, state, end = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, 6))
        rc = lib.load().ldsim_track_gen_count(ctx, C.byref(P), lib.ptr(prim), C.c_int64(n), C.c_uint64(seed), lib.ptr(counts),
                                              lib.ptr(state), lib.ptr(end))
        return rc, lib.load().ldsim_last_error().decode(), counts, state, end
    cap = 0 if capacity is None else int(capacity)
    f, i = np.zeros((len(TG.F64_COLUMNS), max(cap, 1))), np.zeros((len(TG.I32_COLUMNS), max(cap, 1)), dtype=np.int32)
    nseg = C.c_int64(-1)
    rc = lib.load().ldsim_track_gen(ctx, C.byref(P), lib.ptr(prim), C.c_int64(n), C.c_uint64(seed), C.c_int64(cap), lib.ptr(f),
                                    lib.ptr(i), C.byref(nseg))
    return rc, lib.load().ldsim_last_error().decode(), nseg.value, f, i


def test_two_passes_and_capacity():
    """3. the count pass's counts are the write pass's segments per primary; a capacity one too small is refused with the number
    needed and the context works afterwards; exactly enough succeeds"""
    ctx = lib.context()
    prim, p = TC.mixed_primaries(300), TC.params1()
    cnt = TG.count(prim, p, 9)
    total = int(cnt["counts"].sum())
    rc, err, nseg, f, i = _raw(ctx, prim, p, 9, capacity=total - 1)
    assert rc == -1 and "ldsim_track_gen" in err and f"{total} segments are needed" in err and "too small" in err and nseg == 0
    rc, err, nseg, f, i = _raw(ctx, prim, p, 9, capacity=total)
    assert rc == 0 and nseg == total
    assert np.array_equal(np.bincount(i[0], minlength=300), cnt["counts"])
    rc, err, nseg, f2, i2 = _raw(ctx, prim, p, 9, capacity=total + 77)             # a wider stride, the same columns
    assert rc == 0 and nseg == total and np.array_equal(f2[:, :total], f) and np.array_equal(i2[:, :total], i)
    assert not f2[:, total:].any()
    # without a count pass before it (another seed: the context's counts are not this input's)
    g = TG.generate(prim, p, 10)
    rc, err, nseg, f3, i3 = _raw(ctx, prim, p, 11, capacity=int(TG.count(prim, p, 11)["counts"].sum()) + 5)
    rc2, _, nseg2, f4, i4 = _raw(ctx, prim[:7], p, 10, capacity=int(g["counts"][:7].sum()))
    assert rc == 0 and rc2 == 0 and nseg2 == int(g["counts"][:7].sum())
    assert np.array_equal(f4[9], g["dx"][:nseg2])
    empty = TG.generate(prim[:0], p, 9)
    assert len(empty["dx"]) == 0 and len(empty["counts"]) == 0
    assert TG.generate_ms() == 0.0 and TG.generate(prim, p, 9)["dx"].shape == (total,) and TG.generate_ms() > 0


def test_physics_on_the_device():
    """4. the kernel's own output against the analytic values of the host tests 4 and 5, same sizes, same 5-standard-error bounds"""
    n, h = 200_000, 0.1
    p = TG.params(world=BIG, step=h, max_steps=1, mcs=False)
    g = TG.generate(TG.primaries(13, [0, 0, 0], [0, 0, 1], 1000.0, event_id=np.arange(n)), p, 11)
    assert (g["counts"] == 1).all() and (g["end_state"] == TG.TRUNCATED).all() and np.all(g["dx"] == h)
    want = float(TG.stopping_power(1000.0, 13, p)) * p["density"] * h
    se = g["dE"].std(ddof=1) / math.sqrt(n)
    print(f"mean deposit {g['dE'].mean():.6f} MeV, Bethe {want:.6f} MeV, standard error {se:.6f} MeV")
    assert abs(g["dE"].mean() - want) <= 5 * se and g["dE"].max() > 1.0
    n = 20_000
    p = TG.params(world=BIG, step=h, max_steps=101, energy_loss=False)
    g = TG.generate(TG.primaries(13, [0, 0, 0], [0, 0, 1], 1000.0, event_id=np.arange(n)), p, 3)
    assert (g["counts"] == 101).all() and np.all(g["dE"] == 0)
    d = np.stack([(g[a + "_end"] - g[a + "_start"]) / g["dx"] for a in "xyz"], axis=1)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 1e-12
    last = d[g["step"] == 100]
    theta = np.arccos(np.clip(last[:, 2], -1, 1))
    rms, want = math.sqrt((theta ** 2).mean()), math.sqrt(200.0) * float(TG.highland_theta0(h, 1000.0, 13, p))
    print(f"space angle RMS {rms:.6e} rad, expected {want:.6e} rad ({rms / want - 1:+.3%}; bound {5 / math.sqrt(2 * n):.3%})")
    assert abs(rms / want - 1.0) <= 5.0 / math.sqrt(2 * n)
    for k in range(2):
        assert abs(last[:, k].mean()) <= 5 * last[:, k].std(ddof=1) / math.sqrt(n)
    # stopped walks account for their energy, with straggling on and off
    for straggling in (False, True):
        p = TG.params(world=BIG, straggling=straggling)
        T0 = np.geomspace(30.0, 100.0, 64)
        g = TG.generate(TG.primaries(np.where(np.arange(64) % 2, 2212, 13), [0, 0, 0], [0, 0, 1], T0, event_id=np.arange(64)), p, 5)
        assert (g["end_state"] == TG.STOPPED).all()
        assert np.all(np.abs(np.bincount(g["primary"], weights=g["dE"], minlength=64) - T0) <= 1e-12 * T0)


def test_world_box_and_truncation():
    """5. primaries aimed out of a small box end on the wall, on its coordinate exactly; no point lies outside; a walk that needs
    more than max_steps keeps max_steps segments and is flagged"""
    lo, hi = np.array([-5.0, -4.0, -3.0]), np.array([5.0, 4.0, 6.0])
    p = TG.params(world=(lo, hi))
    prim = TG.gun_primaries(13, [0.5, 0.25, 1.0], None, 100.0, 8, 64, 17)
    g = TG.generate(prim, p, 17)
    assert (g["end_state"] == TG.EXITED).all()
    end = g["end_pos"]
    on_wall = (end == lo) | (end == hi)
    assert (on_wall.sum(axis=1) >= 1).all()
    assert set(np.nonzero(on_wall)[1]) == {0, 1, 2}                   # every axis's walls are reached
    for k, a in enumerate("xyz"):
        for which in ("_start", "_end", ""):
            assert (g[a + which] >= lo[k]).all() and (g[a + which] <= hi[k]).all(), a + which
    lastseg = np.cumsum(g["counts"]) - 1
    assert np.array_equal(np.stack([g[a + "_end"][lastseg] for a in "xyz"], axis=1), end)
    p = TG.params(world=BIG, max_steps=10)
    g = TG.generate(TG.primaries(13, [0, 0, 0], [0, 0, 1], [100.0, 0.6]), p, 1)
    # (0.6 MeV: four steps of at most 5 % loss each down to t_min = 0.5 MeV)
    assert list(g["counts"]) == [10, 4] and list(g["end_state"]) == [TG.TRUNCATED, TG.STOPPED] and len(g["dx"]) == 14
    assert g["end_energy"][0] > 90 and g["end_energy"][1] == 0
    TC.compare(g, TG.generate_twin(TG.primaries(13, [0, 0, 0], [0, 0, 1], [100.0, 0.6]), p, 1), "truncated")


def test_refusals_straight_through_ctypes():
    """6. every refusal of the C-ABI, with the entry's name in the message"""
    ctx = lib.context()
    p = TG.params(world=([0, 0, 0], [10, 10, 10]))
    ok = dict(pdg=13, pos=[5, 5, 5], direction=[0, 0, 1], kinetic_energy=50.0)
    one = TG.primaries(**ok)
    rc, err, nseg, _, _ = _raw(ctx, one, p, capacity=1000)
    assert rc == 0 and nseg > 10
    nan, inf = math.nan, math.inf
    cases = [(dict(step=0.0), "step"), (dict(step=nan), "step"), (dict(step=inf), "step"), (dict(min_step=-1.0), "min_step"),
             (dict(min_step=1.0), "exceeds step"), (dict(max_loss_fraction=0.0), "max_loss_fraction"),
             (dict(max_loss_fraction=1.5), "max_loss_fraction"), (dict(t_cut=-1.0), "t_cut"), (dict(t_cut=inf), "t_cut"),
             (dict(t_min=0.0), "t_min"), (dict(t_min=nan), "t_min"), (dict(t_cut=188e-6), "mean excitation"),
             (dict(t_cut=1e-4), "mean excitation"), (dict(t_min=0.01), "stopping power"), (dict(density=0.0), "density"),
             (dict(rad_length=-1.0), "rad_length"), (dict(sternheimer=[nan, 3, 0.2, 3, 5.2, 0]), "sternheimer"),
             (dict(world_hi=[10, 0, 10]), "empty or inverted"), (dict(world_lo=[0, 0, 20]), "empty or inverted"),
             (dict(world_hi=[10, inf, 10]), "empty or inverted"), (dict(max_steps=0), "max_steps"),
             (dict(max_steps=TG.MAX_STEPS_LIMIT + 1), "max_steps")]
    for kw, msg in cases:
        for count_only in (False, True):
            r = _raw(ctx, one, p, capacity=1000, count_only=count_only, **kw)
            assert r[0] == -1 and msg in r[1] and ("ldsim_track_gen_count" if count_only else "ldsim_track_gen:") in r[1], (kw, r[:2])
    for kw, msg in ((dict(pdg=11), "unknown pdg 11"), (dict(pdg=-2212), "unknown pdg -2212"), (dict(pos=[5, 5, 10.5]), "outside the world box"),
                    (dict(pos=[nan, 5, 5]), "outside the world box"), (dict(direction=[0, 0, 0]), "zero direction"),
                    (dict(kinetic_energy=0.0), "kinetic energy"), (dict(kinetic_energy=inf), "kinetic energy"),
                    (dict(kinetic_energy=nan), "kinetic energy"), (dict(time=inf), "time")):
        bad = np.concatenate([one, TG.primaries(**dict(ok, **kw))])
        for count_only in (False, True):
            r = _raw(ctx, bad, p, capacity=1000, count_only=count_only)
            assert r[0] == -1 and msg in r[1] and "primary 1" in r[1] and "ldsim_track_gen" in r[1], (kw, r[:2])
    assert _raw(ctx, one, p, capacity=-1)[0] == -1 and "negative capacity" in lib.load().ldsim_last_error().decode()
    # more than 2^31 - 1 segments: 2048 walks of 2^20 steps (energy loss, fluctuations and scattering off: steps of 0.1 cm for ever)
    far = TG.params(world=([-1e9] * 3, [1e9] * 3), max_steps=1 << 20, energy_loss=False, straggling=False, mcs=False)
    many = TG.primaries(13, [0, 0, 0], [0, 0, 1], np.full(2048, 1000.0), event_id=np.arange(2048))
    rc, err, counts, state, _ = _raw(ctx, many, far, count_only=True)
    assert rc == 0 and (counts == 1 << 20).all() and (state == TG.TRUNCATED).all()
    rc, err, nseg, _, _ = _raw(ctx, many, far, capacity=1)
    assert rc == -1 and "2147483648 segments, more than 2^31 - 1" in err and "ldsim_track_gen:" in err and nseg == 0
    with pytest.raises(lib.LdsimError, match="more than 2\\^31 - 1"):
        TG.generate(many, far, 1)
    # the context still walks, and the same segments
    again = _raw(ctx, one, p, capacity=1000)
    assert again[0] == 0 and again[2] == nseg_ok(ctx, one, p)


def nseg_ok(ctx, one, p):
    return int(TG.count(one, p, 1, ctx)["counts"].sum())


def _sp_cli():
    spec = importlib.util.spec_from_file_location("sp_cli_track_generator_gpu", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_through_the_chain(tmp_path, capsys):
    """7. the tool's file for 2 events of 8 stopping muons in module0 goes through simulate_pixels.py and yields packets; the
    output's segments keep the generator's truth and its summed dE; the --twin file gives the same packets when test 1 found no
    differing primary"""
    b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)
    c = b[0].mean(axis=1)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONHOME"}
    args = ["--config", "module0", "--source", "gun", "--pdg", "13", "--energy", "40", "--position", str(c[2]), str(c[1]), str(c[0]),
            "--isotropic", "--tracks_per_event", "8", "--n_events", "2", "--seed", "12"]
    for name, extra in (("gpu.npz", []), ("twin.npz", ["--twin"])):
        r = subprocess.run([sys.executable, TOOL, *args, *extra, "--output", str(tmp_path / name)], capture_output=True, text=True,
                           env=env, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "16 primaries in 2 events" in r.stdout and "16 stopped, 0 left the world box, 0 truncated" in r.stdout
    with np.load(tmp_path / "gpu.npz") as f:
        seg, traj, vert = f["segments"], f["trajectories"], f["vertices"]
    with np.load(tmp_path / "twin.npz") as f:
        seg_t = f["segments"]
    assert len(traj) == 16 and len(vert) == 2 and len(seg) == int(traj["n_segments"].sum()) > 1000
    assert len(seg_t) == len(seg)
    for k in TG.F64_COLUMNS:
        np.testing.assert_allclose(seg[k], seg_t[k], rtol=1e-6, atol=1e-6, err_msg=k)
    cli = _sp_cli()
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    common = dict(config="module0", rand_seed=7, rng="keyed", light_simulated=False, response_file=str(tmp_path / "resp.npy"))
    out = {}
    try:
        for name in ("gpu", "twin"):
            cli.run_simulation(str(tmp_path / (name + ".npz")), str(tmp_path / (name + "_out.npz")), **common)
            with np.load(tmp_path / (name + "_out.npz")) as f:
                out[name] = {k: f[k] for k in f.files}
    finally:
        H.load_cfg("module0")
    capsys.readouterr()
    o = out["gpu"]
    assert len(o["packets"]) > 100 and (o["packets"]["packet_type"] == 0).sum() > 50
    oseg = o["segments"]
    assert len(oseg) == len(seg) and np.array_equal(np.sort(oseg["segment_id"]), seg["segment_id"])
    back = seg[oseg["segment_id"]]
    for k in ("dE", "dx", "dEdx", "traj_id", "file_traj_id", "event_id", "vertex_id", "pdg_id", "x", "y", "z", "x_start", "z_end"):
        # (the driver swaps x <-> z for itself and back for the file; t, t_start and t_end it fills with the arrival times)
        assert np.array_equal(oseg[k], back[k]), k
    assert float(np.sort(oseg["dE"].astype(np.float64)).sum()) == float(np.sort(seg["dE"].astype(np.float64)).sum())
    assert abs(float(seg["dE"].astype(np.float64).sum()) - 16 * 40.0) < 1e-2
    assert (oseg["n_electrons"] > 0).any()
    assert len(o["trajectories"]) == 16 and len(o["vertices"]) == 2 and "t_event" in o["vertices"].dtype.names
    print(f"fields of the twin's file that differ from the kernel's in some f4's last bit: "
          f"{[k for k in seg.dtype.names if not np.array_equal(seg[k], seg_t[k])]}")
    assert len(out["twin"]["packets"]) > 100
    if _differing() == 0:
        assert o["packets"].tobytes() == out["twin"]["packets"].tobytes()
