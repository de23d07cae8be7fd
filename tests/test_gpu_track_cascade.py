"""GPU: the track cascade (csrc/kernels_trackgen.hip: gen_step<true>, cas_kernel) against its numpy twin
(larndsim_amd/track_cascade.py), against itself under regrouping, against the track generator with emission off, at its limits
and through the chain that reads its file.

Bounds.  Kernel and twin do the same f64 operations in the same order on the same keyed draws; they differ in the last bit of
log / log10 / pow / exp / sqrt / cos / sin / cbrt.  Segments: the bounds of test_gpu_track_generator.py (1e-6 cm / MeV, times
relative to their magnitude).  Counts of segments and of secondaries, end states and the secondaries' integer fields and keys:
equal for every particle of every generation -- the cap on differing families is 1 in 10^4, none of 512 --, at the seed for which
the twin in f64 and in longdouble agree on all of them and on the secondaries' floats (track_cascade_cases.SEED1, test 8 of
test_cpu_track_cascade.py).  The secondaries' pos, dir, kinetic_energy and time: 1e-12 cm, MeV and us, absolute.
Shapes: 512 generation-0 particles (two workgroups at group 256, partial groups at 1000, one group at 4096 and at the default),
some 1000 and 200 particles in generations 1 and 2, halves of 250 + 262."""
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
import track_cascade_cases as CC
import track_gen_cases as GC
from larndsim_amd import abi, consts, lib, synth, track_cascade as TC, track_generator as TG

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "larnd-sim_amd", "cli", "generate_segments.py")
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
COLUMNS = TG.F64_COLUMNS + TG.I32_COLUMNS + ("counts", "secondary_counts", "end_state", "end_pos", "end_time", "path", "end_energy",
                                             "secondaries")
ME = TG.ELECTRON_MASS


@pytest.fixture(autouse=True)
def _cfg():
    H.load_cfg("module0")
    lib.context()
    yield
    lib.set_option("track_gen_group_primaries", 0)


@functools.lru_cache(maxsize=None)
def _twin1():
    H.load_cfg("module0")
    return TC.cascade_twin(CC.mixed_particles(), CC.params1(), CC.cascade1(), CC.SEED1)


@functools.lru_cache(maxsize=None)
def _gpu1():
    H.load_cfg("module0")
    return TC.cascade(CC.mixed_particles(), CC.params1(), CC.cascade1(), CC.SEED1)


def _same_bytes(a, b, what, keys=COLUMNS):
    for k in keys:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def test_cascade_against_twin():
    """1. 512 mixed generation-0 particles, three generations, decays on: counts, end states, integer fields and keys equal for
    every particle of every generation; segments within the track generator's bounds; the secondaries' floats within 1e-12"""
    got, exp = _gpu1(), _twin1()
    print(f"particles per generation: kernel {[len(g['particles']) for g in got]}, twin {[len(g['particles']) for g in exp]}")
    bad = CC.same_counts(got, exp)
    print(f"{int(bad.sum())} of {CC.N1} families differ in a count, an end state or an integer field")
    assert bad.sum() <= CC.N1 // 10_000
    assert len(got) == 3 and len(got[2]["secondaries"]) == 0 and len(got[1]["secondaries"]) > 50
    for k, (g, e) in enumerate(zip(got, exp)):
        assert GC.compare(g, e, f"generation {k}") == 0
        a, b = g["secondaries"], e["secondaries"]
        assert np.array_equal(a["key"], b["key"])
        worst = CC.secondary_deviation(got, exp)[k]
        print(f"generation {k}: {len(a)} secondaries, largest deviations " + ", ".join(f"{f} {v:.1e}" for f, v in worst.items()))
        assert max(worst.values()) <= 1e-12, (k, worst)
        assert np.array_equal(g["primary"], np.repeat(np.arange(len(g["counts"])), g["counts"]))
    proc = got[1]["particles"]["process"]
    assert (proc == TC.DECAY).sum() > 20 and (proc == TC.DELTA_RAY).sum() > 500
    assert set(np.unique(got[0]["end_state"])) == {TG.STOPPED, TG.EXITED}
    # what the families deposit: T0 + the decay electrons' energy - what left the box with a particle
    n = CC.N1
    dE, dec, left = np.zeros(n), np.zeros(n), np.zeros(n)
    for g, r in zip(got, TC.ancestors(got)):
        dE += np.bincount(r[g["primary"]], weights=g["dE"], minlength=n)
        d = g["particles"]["process"] == TC.DECAY
        dec += np.bincount(r[d], weights=g["particles"]["kinetic_energy"][d], minlength=n)
        left += np.bincount(r, weights=g["end_energy"], minlength=n)
    assert np.abs(dE + left - dec - got[0]["particles"]["kinetic_energy"]).max() <= 1e-9


def test_determinism():
    """2. byte-identical segments and secondary records at four group sizes and the default, in one call and in two halves, on two
    contexts, in two calls in a row; the count pass's two count arrays are what the write pass stored"""
    part, p, cp, ref = CC.mixed_particles(), CC.params1(), CC.cascade1(), _gpu1()[0]
    _same_bytes(TC.walk_generation(part, p, cp, CC.SEED1), ref, "second call")
    for group in (64, 256, 1000, 4096):
        lib.set_option("track_gen_group_primaries", group)
        _same_bytes(TC.walk_generation(part, p, cp, CC.SEED1), ref, f"group {group}")
    lib.set_option("track_gen_group_primaries", 0)
    assert np.array_equal(np.bincount(ref["primary"], minlength=CC.N1), ref["counts"])
    assert np.array_equal(np.bincount(ref["secondaries"]["parent"], minlength=CC.N1), ref["secondary_counts"])
    cnt = TC.count_generation(part, p, cp, CC.SEED1)
    assert np.array_equal(cnt["counts"], ref["counts"]) and np.array_equal(cnt["secondary_counts"], ref["secondary_counts"])
    a, b = TC.walk_generation(part[:250], p, cp, CC.SEED1), TC.walk_generation(part[250:], p, cp, CC.SEED1)
    b["secondaries"]["parent"] += 250
    for k in COLUMNS:
        joined = np.concatenate([a[k], b[k] + 250 if k == "primary" else b[k]])
        assert joined.tobytes() == np.asarray(ref[k]).tobytes(), ("two halves", k)
    h = C.c_void_p()
    c = abi.pack_consts()
    lib.check(lib.load().ldsim_ctx_create(C.c_int(0), C.byref(c), C.byref(h)))
    try:
        _same_bytes(TC.walk_generation(part, p, cp, CC.SEED1, ctx=h), ref, "second context")
    finally:
        lib.check(lib.load().ldsim_ctx_destroy(h))
    # the second generation too (about 1000 electrons), at a group size that splits it unevenly
    sec = ref["secondaries"]
    lib.set_option("track_gen_group_primaries", 64)
    _same_bytes(TC.walk_generation(sec, p, cp, CC.SEED1), _gpu1()[1], "generation 1, group 64")
    lib.set_option("track_gen_group_primaries", 0)
    assert not np.array_equal(TC.walk_generation(part, p, cp, CC.SEED1 + 1)["counts"], ref["counts"])


def test_emission_off_is_the_track_generator():
    """3. with emit = 0 the cascade entry writes, for heavy particles, the bytes ldsim_track_gen writes for the same primaries"""
    prim, p = GC.mixed_primaries(512), GC.params1()
    ref = TG.generate(prim, p, GC.SEED1)
    for cp in (TC.cascade_params(t_track=0.5, decays=True), TC.cascade_params(delta_tracks=False)):
        got = TC.walk_generation(TC.particles(prim), p, cp, GC.SEED1, emit=False)
        _same_bytes(got, ref, "emit = 0", TG.F64_COLUMNS + TG.I32_COLUMNS + ("counts", "end_state", "end_pos", "end_time", "path",
                                                                              "end_energy"))
        assert len(got["secondaries"]) == 0 and not got["secondary_counts"].any()
    on = TC.walk_generation(TC.particles(prim), p, TC.cascade_params(t_track=0.5), GC.SEED1)
    assert len(on["secondaries"]) > 100 and on["dE"].sum() < ref["dE"].sum()


def _raw(ctx, part, p, cp, seed=1, capacity=None, secondary_capacity=None, count_only=False, emit=1, **override):
    """the entries straight through ctypes: (status, message, n_segments, n_secondaries, i32 columns, secondaries)"""
    P, CP = TG._pack(p), TC._pack(cp, emit)
    for k, v in override.items():
        target = CP if hasattr(CP, k) else P
        if k in ("world_lo", "world_hi", "sternheimer"):
            getattr(target, k)[:] = v
        else:
            setattr(target, k, v)
    part = np.ascontiguousarray(part, dtype=TC.particle_dtype)
    n = len(part)
    L = lib.load()
    if count_only:
        counts, sc, state, end = (np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32),
                                  np.zeros((n, 6)))
        rc = L.ldsim_track_cascade_count(ctx, C.byref(P), C.byref(CP), lib.ptr(part), C.c_int64(n), C.c_uint64(seed), lib.ptr(counts),
                                         lib.ptr(sc), lib.ptr(state), lib.ptr(end))
        return rc, L.ldsim_last_error().decode(), counts, sc, state, end
    cap = 0 if capacity is None else int(capacity)
    scap = 0 if secondary_capacity is None else int(secondary_capacity)
    f, i = np.zeros((len(TG.F64_COLUMNS), max(cap, 1))), np.zeros((len(TG.I32_COLUMNS), max(cap, 1)), dtype=np.int32)
    sec = np.zeros(max(scap, 1), dtype=TC.particle_dtype)
    nseg, nsec = C.c_int64(-1), C.c_int64(-1)
    rc = L.ldsim_track_cascade(ctx, C.byref(P), C.byref(CP), lib.ptr(part), C.c_int64(n), C.c_uint64(seed), C.c_int64(cap), lib.ptr(f),
                               lib.ptr(i), C.byref(nseg), C.c_int64(scap), lib.ptr(sec), C.byref(nsec))
    return rc, L.ldsim_last_error().decode(), nseg.value, nsec.value, i, sec


def test_capacities():
    """4. a segment or a secondary capacity one too small is refused with the number needed, exactly enough is accepted, and the
    context works afterwards"""
    ctx = lib.context()
    part, p, cp = CC.mixed_particles(300), CC.params1(), CC.cascade1()
    cnt = TC.count_generation(part, p, cp, 9)
    total, stotal = int(cnt["counts"].sum()), int(cnt["secondary_counts"].sum())
    assert stotal > 100
    rc, err, nseg, nsec, _, _ = _raw(ctx, part, p, cp, 9, total - 1, stotal)
    assert rc == -1 and "ldsim_track_cascade:" in err and f"{total} segments are needed" in err and "too small" in err
    assert nseg == 0 and nsec == 0
    rc, err, nseg, nsec, _, _ = _raw(ctx, part, p, cp, 9, total, stotal - 1)
    assert rc == -1 and "ldsim_track_cascade:" in err and f"{stotal} secondaries are needed" in err and "too small" in err
    rc, err, nseg, nsec, i, sec = _raw(ctx, part, p, cp, 9, total, stotal)
    assert rc == 0 and nseg == total and nsec == stotal
    assert np.array_equal(np.bincount(i[0], minlength=300), cnt["counts"])
    assert np.array_equal(np.bincount(sec["parent"], minlength=300), cnt["secondary_counts"])
    rc, err, nseg, nsec, i2, sec2 = _raw(ctx, part, p, cp, 9, total + 77, stotal + 5)          # wider strides, the same output
    assert rc == 0 and np.array_equal(i2[:, :total], i) and not i2[:, total:].any()
    assert sec2[:stotal].tobytes() == sec.tobytes() and not sec2[stotal:].view(np.uint8).any()
    # without a count pass before it (another seed: the context's counts are not this input's), and an empty list
    want = TC.count_generation(part, p, cp, 11)
    rc, err, nseg, nsec, _, _ = _raw(ctx, part, p, cp, 10, 10 ** 6, 10 ** 5)
    rc2, _, nseg2, nsec2, _, _ = _raw(ctx, part, p, cp, 11, int(want["counts"].sum()), int(want["secondary_counts"].sum()))
    assert rc == 0 and rc2 == 0 and nseg2 == int(want["counts"].sum()) and nsec2 == int(want["secondary_counts"].sum())
    empty = TC.walk_generation(part[:0], p, cp, 9)
    assert len(empty["dx"]) == 0 and len(empty["secondaries"]) == 0
    assert TC.walk_generation_ms() == 0.0 and len(TC.walk_generation(part, p, cp, 9)["dx"]) == total and TC.walk_generation_ms() > 0


def test_refusals_straight_through_ctypes():
    """5. every refusal of the C-ABI, with the entry's name in the message"""
    ctx = lib.context()
    p, cp = TG.params(world=([0, 0, 0], [10, 10, 10])), TC.cascade_params()
    ok = dict(pdg=11, pos=[5, 5, 5], direction=[0, 0, 1], kinetic_energy=5.0)
    one = TC.particles(TG.primaries(**ok))
    rc, err, nseg, nsec, _, _ = _raw(ctx, one, p, cp, capacity=1000, secondary_capacity=100)
    assert rc == 0 and nseg > 10
    nan, inf = math.nan, math.inf
    cases = [(dict(step=0.0), "step"), (dict(step=nan), "step"), (dict(min_step=-1.0), "min_step"), (dict(min_step=1.0), "exceeds step"),
             (dict(max_loss_fraction=0.0), "max_loss_fraction"), (dict(max_loss_fraction=1.5), "max_loss_fraction"),
             (dict(t_cut=-1.0), "t_cut"), (dict(t_cut=inf), "t_cut"), (dict(t_min=0.0), "t_min"), (dict(t_min=nan), "t_min"),
             (dict(t_cut=1e-4), "mean excitation"), (dict(t_min=0.01), "stopping power"), (dict(density=0.0), "density"),
             (dict(rad_length=-1.0), "rad_length"), (dict(sternheimer=[nan, 3, 0.2, 3, 5.2, 0]), "sternheimer"),
             (dict(world_hi=[10, 0, 10]), "empty or inverted"), (dict(world_lo=[0, 0, 20]), "empty or inverted"),
             (dict(max_steps=0), "max_steps"), (dict(max_steps=TG.MAX_STEPS_LIMIT + 1), "max_steps"),
             (dict(t_track=0.05), "t_track"), (dict(t_track=0.3), "t_track"), (dict(t_track=nan), "t_track"),
             (dict(t_track=inf), "t_track"), (dict(t_cut=2.0), "t_track"), (dict(capture_fraction=-0.1), "capture_fraction"),
             (dict(capture_fraction=1.5), "capture_fraction"), (dict(capture_fraction=nan), "capture_fraction"),
             (dict(mu_plus_lifetime=0.0), "mu_plus_lifetime"), (dict(mu_plus_lifetime=nan), "mu_plus_lifetime"),
             (dict(mu_minus_lifetime=-1.0), "mu_minus_lifetime"), (dict(mu_minus_lifetime=inf), "mu_minus_lifetime")]
    for kw, msg in cases:
        for count_only in (False, True):
            r = _raw(ctx, one, p, cp, capacity=1000, secondary_capacity=100, count_only=count_only, **kw)
            assert r[0] == -1 and msg in r[1] and ("ldsim_track_cascade_count" if count_only else "ldsim_track_cascade:") in r[1], (kw, r[:2])
    for kw, msg in ((dict(pdg=22), "unknown pdg 22"), (dict(pdg=-2212), "unknown pdg -2212"), (dict(pos=[5, 5, 10.5]), "outside the world box"),
                    (dict(pos=[nan, 5, 5]), "outside the world box"), (dict(direction=[0, 0, 0]), "zero direction"),
                    (dict(kinetic_energy=0.0), "kinetic energy"), (dict(kinetic_energy=inf), "kinetic energy"),
                    (dict(kinetic_energy=nan), "kinetic energy"), (dict(time=inf), "time")):
        bad = np.concatenate([one, TC.particles(TG.primaries(**dict(ok, **kw)))])
        for count_only in (False, True):
            r = _raw(ctx, bad, p, cp, capacity=1000, secondary_capacity=100, count_only=count_only)
            assert r[0] == -1 and msg in r[1] and "particle 1" in r[1] and "ldsim_track_cascade" in r[1], (kw, r[:2])
    assert _raw(ctx, one, p, cp, capacity=-1)[0] == -1 and "negative capacity" in lib.load().ldsim_last_error().decode()
    assert _raw(ctx, one, p, cp, capacity=1000, secondary_capacity=-1)[0] == -1
    # the old entries still refuse an electron, by their own names
    P = TG._pack(p)
    prim = TG.primaries(**ok)
    counts, state, end = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros((1, 6))
    rc = lib.load().ldsim_track_gen_count(ctx, C.byref(P), lib.ptr(prim), C.c_int64(1), C.c_uint64(1), lib.ptr(counts), lib.ptr(state),
                                          lib.ptr(end))
    assert rc == -1 and "ldsim_track_gen_count: primary 0 has unknown pdg 11" in lib.load().ldsim_last_error().decode()
    # more than 2^31 - 1 segments: 2048 walks of 2^20 steps (energy loss, fluctuations and scattering off), as in the track
    # generator's test
    far = TG.params(world=([-1e9] * 3, [1e9] * 3), max_steps=1 << 20, energy_loss=False, straggling=False, mcs=False)
    many = TC.particles(TG.primaries(13, [0, 0, 0], [0, 0, 1], np.full(2048, 1000.0), event_id=np.arange(2048)))
    rc, err, nseg, nsec, _, _ = _raw(ctx, many, far, cp, capacity=1, secondary_capacity=1)
    assert rc == -1 and "2147483648 segments, more than 2^31 - 1" in err and "ldsim_track_cascade:" in err and nseg == 0
    # more than 2^31 - 1 secondaries from 2^28 segments, which are accepted: steps of 512 cm of muons of 10^16 MeV with t_track =
    # t_cut = t_min = 0.5 MeV have a Poisson mean of 98 hard collisions, so every step emits the cap of 8 (fewer with probability
    # 10^-32; a collision's energy is at least t_cut exactly, 1 / (2 - u ..) >= 0.5); 2048 walks of 2^17 steps lose 4x10^8 MeV each
    dense = TG.params(world=([-1e9] * 3, [1e9] * 3), step=512.0, max_loss_fraction=1.0, t_cut=0.5, t_min=0.5, max_steps=1 << 17, mcs=False)
    hot = TC.particles(TG.primaries(13, [0, 0, 0], [0, 0, 1], np.full(2048, 1e16), event_id=np.arange(2048)))
    tt = TC.cascade_params(t_track=0.5)
    rc, err, counts, scounts, state, _ = _raw(ctx, hot, dense, tt, count_only=True)
    assert rc == 0 and (counts == 1 << 17).all() and (scounts == 1 << 20).all() and (state == TG.TRUNCATED).all(), err
    rc, err, nseg, nsec, _, _ = _raw(ctx, hot, dense, tt, capacity=1, secondary_capacity=1)
    assert rc == -1 and "2147483648 secondaries, more than 2^31 - 1" in err and "ldsim_track_cascade:" in err and nseg == 0 and nsec == 0
    with pytest.raises(lib.LdsimError, match="secondaries, more than 2\\^31 - 1"):
        TC.walk_generation(hot, dense, tt, 1)
    # the context still walks, and the same segments
    again = _raw(ctx, one, p, cp, capacity=1000, secondary_capacity=100)
    assert again[0] == 0 and again[2] == nseg0(ctx, one, p, cp)


def nseg0(ctx, one, p, cp):
    return int(TC.count_generation(one, p, cp, 1, ctx=ctx)["counts"].sum())


def _sp_cli():
    spec = importlib.util.spec_from_file_location("sp_cli_track_cascade_gpu", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_through_the_chain(tmp_path, capsys):
    """6. the tool's file for 2 events of 4 stopping mu+ of 100 MeV with --secondaries --decays goes through simulate_pixels.py:
    packets exist, the output's trajectories keep the parent links, the segments' summed dE is the primaries' T0 plus the decay
    electrons' T within f4 rounding, and the --twin file gives the same packets"""
    b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)
    c = b[0].mean(axis=1)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONHOME"}
    args = ["--config", "module0", "--source", "gun", "--pdg", "-13", "--energy", "100", "--position", str(c[2]), str(c[1]), str(c[0]),
            "--isotropic", "--tracks_per_event", "4", "--n_events", "2", "--seed", "12", "--secondaries", "--decays", "--margin", "60"]
    for name, extra in (("gpu.npz", []), ("twin.npz", ["--twin"])):
        r = subprocess.run([sys.executable, TOOL, *args, *extra, "--output", str(tmp_path / name)], capture_output=True, text=True,
                           env=env, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "8 primaries in 2 events" in r.stdout and "8 decay electrons" in r.stdout and "0 left the world box, 0 truncated" in r.stdout
    with np.load(tmp_path / "gpu.npz") as f:
        seg, traj, vert = f["segments"], f["trajectories"], f["vertices"]
    with np.load(tmp_path / "twin.npz") as f:
        seg_t, traj_t = f["segments"], f["trajectories"]
    assert len(vert) == 2 and traj["primary"].sum() == 8 and len(traj) > 16 and len(seg) == int(traj["n_segments"].sum()) > 1000
    assert len(seg_t) == len(seg) and np.array_equal(traj["parent_id"], traj_t["parent_id"]) and np.array_equal(traj["pdg_id"], traj_t["pdg_id"])
    for k in TG.F64_COLUMNS:
        np.testing.assert_allclose(seg[k], seg_t[k], rtol=1e-6, atol=1e-6, err_msg=k)
    dec = traj[(traj["pdg_id"] == -11) & (traj["parent_id"] >= 0) & (traj["parent_id"] < 8)]
    assert len(dec) == 8
    want = 8 * 100.0 + float((dec["E_start"].astype(np.float64) - ME).sum())
    print(f"summed dE {float(seg['dE'].astype(np.float64).sum()):.4f} MeV, T0 + decay electrons {want:.4f} MeV")
    assert abs(float(seg["dE"].astype(np.float64).sum()) - want) < 2e-2      # (some 1e4 f4 values of 1e-8 relative rounding each, E_start f4)
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
    otraj = o["trajectories"]
    assert len(otraj) == len(traj) and np.array_equal(otraj["parent_id"], traj["parent_id"]) and np.array_equal(otraj["traj_id"], traj["traj_id"])
    assert np.array_equal(otraj["primary"], traj["primary"]) and len(o["vertices"]) == 2
    assert len(o["segments"]) > 1000 and (o["segments"]["n_electrons"] > 0).any()      # (the driver keeps the active volume's)
    assert o["packets"].tobytes() == out["twin"]["packets"].tobytes()
