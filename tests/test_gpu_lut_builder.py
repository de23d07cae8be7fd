"""GPU: the light LUT builder (csrc/kernels_lutbuild.hip: lut_build_kernel, lut_trace_kernel) against its numpy twin
(larndsim_amd/lut_builder.py trace_twin), against closed forms, and through the light leg that reads its table.

Bounds.  Kernel and twin do the same f64 operations in the same order on the same keyed draws; they can differ only in the last
bit of log / cos / sin / cbrt, so a different fate or step count needs a comparison decided by that bit: the cap of 1 photon in
10^4 is the issue's, the expected number is 0, and the number found is printed.  Where the fates agree, times agree to rtol 1e-12
and end points to 1e-12 of the end point's norm (a walk of tens of steps accumulates a few 1e-16 per step of a 30 cm scale; a
single coordinate may pass through 0, a position vector in this box does not).  Tables against their own trace are integers and
must be equal.  Monte Carlo against closed forms: 5 binomial standard errors of the expected share, every cell with at least 1000
expected photons (asserted).
Shapes: the smallest that take every path -- six detectors with two on one wall, a grid with an axis of one voxel, photon counts
that are no multiple of the group (20 000 at groups of 256, 4096, 8192: one partial group, several groups, a group larger than
the count), both tally paths."""
import ctypes as C
import functools
import importlib.util
import json
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import helpers as H
import light_interp_cases as LC
from larndsim_amd import abi, consts, lib, lightLUT, lut_builder as LB, synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "larnd-sim_amd", "cli", "build_light_lut.py")
BOX = [30.0, 60.0, 30.0]
VG = LB.GROUP_VELOCITY_CM_NS
SEED = 20241016
# test 1's case: six detectors, two of them on u0; a wall without one (w0)
SIX = {"box": BOX, "detectors": [LB.detector("u0", (20, 0), (40, 15)), LB.detector("u0", (40, 15), (60, 30)),
                                 LB.detector("u1", (5, 5), (55, 25)), LB.detector("v0", (0, 0), (30, 30)),
                                 LB.detector("v1", (10, 0), (30, 20)), LB.detector("w1", (0, 10), (30, 50))]}
GRID1, VOXELS1, N1 = (2, 1, 3), (0, 2, 5), 20_000
INC_DTYPE = [('segment_id', 'u4'), ('n_photons_det', 'f4'), ('t0_det', 'f4')]


def _p1(emit_mode, **kw):
    return LB.params(rayleigh_cm=20, absorption_cm=80, wall_reflectivity=[0.5, 0.5, 0.3, 0.3, 0, 0], emit_mode=emit_mode, **kw)


@functools.lru_cache(maxsize=None)
def _twin1(voxel, emit_mode, max_steps=1000):
    return LB.trace_twin(SIX, GRID1, voxel, (0, N1), SEED, _p1(emit_mode, max_steps=max_steps))


@functools.lru_cache(maxsize=None)
def _trace1(voxel, emit_mode, max_steps=1000):
    H.load_cfg("module0")
    return LB.trace(SIX, GRID1, voxel, (0, N1), SEED, _p1(emit_mode, max_steps=max_steps))


def _compare(got, exp, what):
    n = len(exp["fate"])
    differ = (got["fate"] != exp["fate"]) | (got["steps"] != exp["steps"])
    print(f"{what}: {int(differ.sum())} of {n} photons differ from the twin in fate or step count")
    assert differ.sum() <= n // 10_000, what
    same = ~differ
    np.testing.assert_allclose(got["time"][same], exp["time"][same], rtol=1e-12, atol=0, err_msg=what)
    err = np.linalg.norm(got["end"][same] - exp["end"][same], axis=1)
    assert (err <= 1e-12 * np.linalg.norm(exp["end"][same], axis=1)).all(), (what, err.max())


@pytest.mark.parametrize("emit_mode", [0, 1], ids=["volume", "centre"])
def test_trajectories_against_the_twin(emit_mode):
    """1. fate, step count, arrival time and end point of 20 000 photons from each of 3 voxels, both emit modes"""
    fates = []
    for v in VOXELS1:
        got, exp = _trace1(v, emit_mode), _twin1(v, emit_mode)
        _compare(got, exp, f"voxel {v}, emit_mode {emit_mode}")
        fates.append(got["fate"])
        assert got["steps"].min() >= 1 and (got["time"] > 0).all()
        assert (got["end"] >= 0).all() and (got["end"] <= np.array(BOX)).all()
    fates = np.concatenate(fates)
    assert (fates == LB.FATE_BULK).any() and (fates == LB.FATE_WALL).any() and (fates != LB.FATE_TRUNCATED).all()
    assert set(range(6)) <= set(np.unique(fates))                 # every detector, the second one of u0 included
    cut, exp = _trace1(VOXELS1[1], emit_mode, 3), _twin1(VOXELS1[1], emit_mode, 3)
    _compare(cut, exp, f"max_steps 3, emit_mode {emit_mode}")
    assert (cut["fate"] == LB.FATE_TRUNCATED).any() and (cut["steps"][cut["fate"] == LB.FATE_TRUNCATED] == 3).all()
    if emit_mode:                                                 # centre emission: the voxel's centre is where every walk starts
        one = LB.trace({"box": BOX, "detectors": [LB.detector("u0", (0, 0), (60, 30))]}, GRID1, 0, (0, 64), SEED,
                       LB.params(emit_mode=1))
        hit = one["fate"] == 0
        r = np.linalg.norm(one["end"][hit] - np.array([7.5, 30.0, 5.0]), axis=1)
        np.testing.assert_allclose(one["time"][hit], r / VG, rtol=1e-12)


@pytest.fixture
def tally_path():
    """sets the build's tally path and puts the default back"""
    H.load_cfg("module0")
    lib.context()

    def choose(lds_tile, group=4096):
        lib.set_option("lut_build_lds_tile", lds_tile)
        lib.set_option("lut_build_group_photons", group)
    yield choose
    lib.set_option("lut_build_lds_tile", 1)
    lib.set_option("lut_build_group_photons", 4096)


def _assert_same_tallies(a, b, what):
    for k in ("count", "hist", "tsum", "fates"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert np.asarray(a["tmin"], dtype="f4").tobytes() == np.asarray(b["tmin"], dtype="f4").tobytes(), (what, "tmin")


@pytest.mark.parametrize("lds_tile", [1, 0], ids=["lds_tile", "global_atomics"])
@pytest.mark.parametrize("emit_mode", [0, 1], ids=["volume", "centre"])
def test_tables_are_the_tallies_of_the_kernels_own_walk(emit_mode, lds_tile, tally_path):
    """2. count, hist, tmin (bit-equal), tsum and the fate counters of a build == numpy tallies of the trace of the same photons"""
    tally_path(lds_tile)
    p = _p1(emit_mode)
    for v in VOXELS1:
        got = LB.build(SIX, GRID1, N1, SEED, p, (v, v + 1))
        exp = LB.tally(_trace1(v, emit_mode), 6, p["nprof"])
        _assert_same_tallies({k: got[k][0] for k in exp}, exp, (v, emit_mode, lds_tile))
        assert int(got["count"].sum() + got["fates"].sum()) == N1
        assert (got["hist"].sum(axis=-1) == got["count"]).all()
    # a tile too big for LDS takes the global path by itself: 6 detectors x 512 bins fit, 40 x 512 do not
    many = {"box": BOX, "detectors": LB.tile_wall("u0", 8, 5, BOX) + SIX["detectors"][2:]}
    pw = _p1(emit_mode, nprof=512)
    big = LB.build(many, GRID1, 3000, SEED, pw, (5, 6))
    exp = LB.tally(LB.trace(many, GRID1, 5, (0, 3000), SEED, pw), len(many["detectors"]), 512)
    _assert_same_tallies({k: big[k][0] for k in exp}, exp, "nprof 512")


# ---- closed forms -------------------------------------------------------------------------------------------------------
GRID3, N3 = (2, 1, 2), 200_000
EXTRA = [LB.detector("v0", (0, 0), (30, 30)), LB.detector("w1", (0, 0), (30, 60))]
LAYOUTS = {"two_on_u0": [LB.detector("u0", (20, 0), (40, 15)), LB.detector("u0", (40, 15), (60, 30))] + EXTRA,
           "full_u0": [LB.detector("u0", (0, 0), (60, 30))] + EXTRA}


def _centre(voxel, grid):
    i, j, k = voxel // grid[2] // grid[1], voxel // grid[2] % grid[1], voxel % grid[2]
    return np.array([(i + 0.5) * BOX[0] / grid[0], (j + 0.5) * BOX[1] / grid[1], (k + 0.5) * BOX[2] / grid[2]])


def _rect_frame(point, det):
    """(h, pa, pb): height of the point over the detector's wall and its foot in the wall's in-plane coordinates"""
    w = LB.wall_index(det["wall"])
    axis = w // 2
    h = BOX[axis] - point[axis] if w % 2 else point[axis]
    return h, point[(axis + 1) % 3], point[(axis + 2) % 3]


def _distance_range(point, det):
    h, pa, pb = _rect_frame(point, det)
    near = math.hypot(min(max(pa, det["lo"][0]), det["hi"][0]) - pa, min(max(pb, det["lo"][1]), det["hi"][1]) - pb)
    far = math.hypot(max(abs(det["lo"][0] - pa), abs(det["hi"][0] - pa)), max(abs(det["lo"][1] - pb), abs(det["hi"][1] - pb)))
    return math.hypot(h, near), math.hypot(h, far)


def _absorbed_share(point, det, lam, m=400):
    """m x m midpoint quadrature of exp(-r / lambda) h / (4 pi r^3) over the rectangle"""
    h, pa, pb = _rect_frame(point, det)
    a = det["lo"][0] + (np.arange(m) + 0.5) * (det["hi"][0] - det["lo"][0]) / m - pa
    b = det["lo"][1] + (np.arange(m) + 0.5) * (det["hi"][1] - det["lo"][1]) / m - pb
    r = np.sqrt(h * h + a[:, None] ** 2 + b[None, :] ** 2)
    cell = (det["hi"][0] - det["lo"][0]) * (det["hi"][1] - det["lo"][1]) / (m * m)
    return float((np.exp(-r / lam) * h / (4 * math.pi * r ** 3)).sum() * cell)


@functools.lru_cache(maxsize=None)
def _build3(layout, absorption):
    H.load_cfg("module0")
    return LB.build({"box": BOX, "detectors": LAYOUTS[layout]}, GRID3, N3, SEED, LB.params(absorption_cm=absorption, emit_mode=1))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_pure_geometry_against_the_solid_angle(layout):
    """3. vis within 5 binomial standard errors of Omega / 4 pi in every (voxel, detector) cell; tmin and the histogram's support
    from the nearest and the farthest point of the rectangle"""
    dets = LAYOUTS[layout]
    t = _build3(layout, math.inf)
    lut = LB.to_lut(t, GRID3)
    assert (t["fates"][:, 0] == 0).all() and (t["fates"][:, 2] == 0).all()
    assert (t["count"].sum(axis=1) + t["fates"][:, 1] == N3).all()
    for v in range(4):
        pt = _centre(v, GRID3)
        for k, d in enumerate(dets):
            share = LB.solid_angle_visibility(pt, d, BOX)
            assert N3 * share >= 1000, (v, k, share)
            vis = t["count"][v, k] / N3
            assert abs(vis - share) <= 5 * math.sqrt(share * (1 - share) / N3), (v, k, vis, share)
            assert lut["vis"].reshape(4, -1)[v, k] == np.float32(vis)
            d_min, d_max = _distance_range(pt, d)
            assert t["tmin"][v, k] >= np.float32(d_min / VG), (v, k)
            support = np.flatnonzero(t["hist"][v, k])
            assert support.min() >= math.floor(d_min / VG) and support.max() <= math.floor(d_max / VG), (v, k, support)
            assert lut["t0_avg"].reshape(4, -1)[v, k] >= lut["t0"].reshape(4, -1)[v, k]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_absorption_against_the_quadrature(layout):
    """4. absorption length 40 cm: vis within 5 standard errors of the attenuated solid-angle integral"""
    dets = LAYOUTS[layout]
    t = _build3(layout, 40.0)
    free = _build3(layout, math.inf)
    assert (t["fates"][:, 0] > 0).all() and (t["fates"][:, 2] == 0).all()
    assert (t["count"].sum(axis=1) + t["fates"].sum(axis=1) == N3).all()
    for v in range(4):
        pt = _centre(v, GRID3)
        for k, d in enumerate(dets):
            share = _absorbed_share(pt, d, 40.0)
            assert share < LB.solid_angle_visibility(pt, d, BOX)
            vis = t["count"][v, k] / N3
            assert abs(vis - share) <= 5 * math.sqrt(share * (1 - share) / N3), (v, k, vis, share)
            assert t["count"][v, k] < free["count"][v, k]


def test_conservation_under_scattering():
    """5. a 30 cm cube whose six walls are detectors, Rayleigh 6 cm, no absorption: every photon arrives, a sixth on each wall,
    later than the straight path; a reflecting box gives one detector more light than an absorbing one"""
    H.load_cfg("module0")
    cube = [30.0, 30.0, 30.0]
    walls = {"box": cube, "detectors": [LB.detector(w, (0, 0), (30, 30)) for w in LB.WALLS]}
    n = 200_000
    t = LB.build(walls, (1, 1, 1), n, SEED, LB.params(rayleigh_cm=6, emit_mode=1, max_steps=100_000))
    assert int(t["count"].sum()) == n and (t["fates"] == 0).all()
    for k in range(6):
        assert abs(t["count"][0, k] / n - 1 / 6) <= 5 * math.sqrt((1 / 6) * (5 / 6) / n), (k, t["count"][0, k] / n)
    lut = LB.to_lut(t, (1, 1, 1))
    assert (lut["t0_avg"] > 15 / VG).all() and (lut["t0"] >= np.float32(15 / VG)).all()
    np.testing.assert_allclose(lut["time_dist"].sum(axis=-1), 1.0, rtol=1e-6)
    one = {"box": cube, "detectors": [LB.detector("u0", (0, 0), (30, 30))]}
    dark = LB.build(one, (1, 1, 1), n, SEED, LB.params(rayleigh_cm=6, emit_mode=1, max_steps=100_000))
    lit = LB.build(one, (1, 1, 1), n, SEED, LB.params(rayleigh_cm=6, emit_mode=1, max_steps=100_000, wall_reflectivity=0.5))
    assert lit["count"][0, 0] > dark["count"][0, 0]
    for r in (dark, lit):
        assert int(r["count"].sum() + r["fates"].sum()) == n and r["fates"][0, 0] == 0 and r["fates"][0, 2] == 0
    assert lit["fates"][0, 1] < dark["fates"][0, 1]


def _second_context():
    h = C.c_void_p()
    c = abi.pack_consts()
    lib.check(lib.load().ldsim_ctx_create(C.c_int(0), C.byref(c), C.byref(h)))
    return h


def test_partition_independence(tally_path):
    """6. byte-identical arrays at group sizes 256 and 8192, with the voxel range in one call and in three, on two contexts;
    another seed gives other counts"""
    p = _p1(0)
    tally_path(1, 4096)
    ref = LB.build(SIX, GRID1, N1, SEED, p)
    assert ref["count"].shape == (6, 6) and (ref["count"].sum(axis=1) + ref["fates"].sum(axis=1) == N1).all()
    for v in VOXELS1:                                             # (and the table is the one test 2 pins to the trace)
        _assert_same_tallies({k: ref[k][v] for k in ("count", "hist", "tmin", "tsum", "fates")},
                             LB.tally(_trace1(v, 0), 6, p["nprof"]), v)
    for group in (256, 8192):
        tally_path(1, group)
        _assert_same_tallies(LB.build(SIX, GRID1, N1, SEED, p), ref, f"group {group}")
    tally_path(1, 4096)
    parts = [LB.build(SIX, GRID1, N1, SEED, p, r) for r in ((4, 6), (0, 1), (1, 4))]
    _assert_same_tallies(LB.concatenate(parts), ref, "three calls")
    empty = LB.build(SIX, GRID1, N1, SEED, p, (3, 3))
    assert empty["count"].shape == (0, 6)
    other = _second_context()
    try:
        _assert_same_tallies(LB.build(SIX, GRID1, N1, SEED, p, ctx=other), ref, "second context")
    finally:
        lib.check(lib.load().ldsim_ctx_destroy(other))
    assert not np.array_equal(LB.build(SIX, GRID1, N1, SEED + 1, p)["count"], ref["count"])


# ---- downstream ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _module0_lut(emit_mode):
    """(3, 4, 2) voxels x 8 detectors in module0's padded TPC box (kept alive: lib.set_light tells tables apart by address)"""
    H.load_cfg("module0")
    box = LB.box_from_consts(0)
    assert np.allclose(box, LB.box_from_consts(1), rtol=0, atol=1e-9)
    geo = {"box": box, "detectors": LB.tile_wall("v0", 2, 2, box, gap=0.5) + LB.tile_wall("v1", 2, 2, box, gap=0.5)}
    t = LB.build(geo, (3, 4, 2), 20_000, SEED, LB.params(rayleigh_cm=60, wall_reflectivity=0.2, emit_mode=emit_mode, nprof=8))
    return LB.to_lut(t, (3, 4, 2))


def _centre_segments(vox_div):
    """a segment at every voxel centre of an even and an odd TPC (x mirrored in the odd one, y flipped in both)"""
    H.load_cfg("module0")
    b = np.asarray(consts.detector.TPC_BORDERS)
    assert b[0][2][1] > b[0][2][0] and b[1][2][1] < b[1][2][0]
    idx = np.array([(i, j, k) for i in range(vox_div[0]) for j in range(vox_div[1]) for k in range(vox_div[2])])
    xs, ys, zs, tp = [], [], [], []
    for itpc in (0, 1):
        for i, j, k in idx:
            x, y, z = LC.position(i + 0.5, j + 0.5, k + 0.5, itpc, vox_div)
            xs.append(x), ys.append(y), zs.append(z), tp.append(itpc)
    return LC.records(np.array(xs), np.array(ys), np.array(zs), np.array(tp, dtype=np.int32), 31), np.concatenate([idx, idx])


def _incidence(r, lut):
    n_out = consts.light.N_OP_CHANNEL
    inc = np.zeros((len(r), n_out), dtype=INC_DTYPE)
    vox = np.full((len(r), 3), -1, dtype='i4')
    lightLUT.calculate_light_incidence[1, 256](r, lut, inc, vox)
    return inc['n_photons_det'].copy(), vox


def _expected_incidence(r, lut, idx):
    n_out = consts.light.N_OP_CHANNEL
    li = np.arange(n_out) % lut.shape[-1]
    vis = lut["vis"][idx[:, 0], idx[:, 1], idx[:, 2]][:, li].astype(np.float64)
    own = np.asarray(consts.light.OP_CHANNEL_TO_TPC)[None, :] == r["pixel_plane"][:, None]
    eff = np.asarray(consts.light.OP_CHANNEL_EFFICIENCY, dtype=np.float64)[None, :]
    return (eff * (vis * own) * r["n_photons"].astype(np.float64)[:, None]).astype(np.float32)


def test_built_table_through_the_light_incidence():
    """7. to_lut of a build goes through lib.set_light and calculate_light_incidence: n_photons_det is f4(eff * vis[voxel] *
    (ch2tpc == itpc) * n_photons) with the voxel computed in numpy; under light_lut_interp 1 a centre-emission table returns the
    voxel's own value at a voxel centre within 1 f4 ulp"""
    vox_div = (3, 4, 2)
    r, idx = _centre_segments(vox_div)
    lut = _module0_lut(0)
    assert lut.shape == (3, 4, 2, 8) and lut.dtype == synth.lut_dtype(8) and (lut["vis"] > 0).all()
    nph, vox = _incidence(r, lut)
    assert np.array_equal(vox, idx)
    exp = _expected_incidence(r, lut, idx)
    assert np.array_equal(nph, exp) and (nph > 0).any(axis=1).all()
    own = np.asarray(consts.light.OP_CHANNEL_TO_TPC)[None, :] == r["pixel_plane"][:, None]
    assert (nph[~own] == 0).all()
    centre = _module0_lut(1)
    assert not np.array_equal(centre["vis"], lut["vis"])
    try:
        lib.set_option("light_lut_interp", 1)
        got, vox = _incidence(r, centre)
    finally:
        lib.set_option("light_lut_interp", 0)
    assert np.array_equal(vox, idx)
    assert LC.ulp_close(got, _expected_incidence(r, centre, idx))


def test_tool_and_driver_files(tmp_path, capsys):
    """8. build_light_lut.py writes an .npz whose `arr` is to_lut of a direct build; simulate_pixels.py --light_lut_filename
    takes it and writes non-empty light_dat"""
    H.load_cfg("module0")
    box = LB.box_from_consts(0)
    geo = {"box": box, "detectors": LB.tile_wall("v0", 6, 4, box, gap=0.3) + LB.tile_wall("v1", 6, 4, box, gap=0.3)}
    LB.dump(tmp_path / "geo.json", geo)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONHOME"}
    args = ["--geometry", str(tmp_path / "geo.json"), "--vox_div", "3", "4", "2", "--photons", "5000", "--seed", "9",
            "--rayleigh_cm", "60", "--wall_reflectivity", "0.3", "--nprof", "20", "--max_steps", "4"]
    r = subprocess.run([sys.executable, TOOL, *args, "--output", str(tmp_path / "lut.npz")], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "truncated share" in r.stdout and "WARNING" in r.stderr and "--max_steps" in r.stderr      # 4 steps cut walks off
    p = LB.params(rayleigh_cm=60, wall_reflectivity=0.3, nprof=20, max_steps=4)
    direct = LB.build(geo, (3, 4, 2), 5000, 9, p)
    with np.load(tmp_path / "lut.npz") as f:
        arr, fates, run = f["arr"], f["fates"], json.loads(str(f["params"]))
    exp = LB.to_lut(direct, (3, 4, 2))
    assert arr.dtype == exp.dtype == synth.lut_dtype(20) and arr.shape == (3, 4, 2, 48) and arr.tobytes() == exp.tobytes()
    assert np.array_equal(fates, direct["fates"]) and fates[:, 2].sum() > 1e-3 * 24 * 5000
    assert run["photons"] == 5000 and run["seed"] == 9 and run["vox_div"] == [3, 4, 2] and run["rayleigh_cm"] == 60
    r = subprocess.run([sys.executable, TOOL, *args, "--voxel_range", "5", "11", "--output", str(tmp_path / "part.npz")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(tmp_path / "part.npz") as f:
        assert f["arr"].tobytes() == exp.reshape(24, 48)[5:11].tobytes()
    # the driver
    spec = importlib.util.spec_from_file_location("sp_cli_lut_builder", os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    seg = synth.make_segments(60, seed=10, segs_per_event=30)
    np.save(tmp_path / "in.npy", seg)
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    try:
        cli.run_simulation(str(tmp_path / "in.npy"), str(tmp_path / "out.npz"), config="module0", rand_seed=1,
                           response_file=str(tmp_path / "resp.npy"), light_lut_filename=str(tmp_path / "lut.npz"))
    finally:
        H.load_cfg("module0")
    capsys.readouterr()
    with np.load(tmp_path / "out.npz") as out:
        dat = out["light_dat__light_dat_allmodules"]
        assert dat.shape == (out["segments"].shape[0], consts.light.N_OP_CHANNEL) and len(dat) > 0
        assert (dat["n_photons_det"] > 0).any()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _raw_build(ctx, box=BOX, dets=((0, (20, 0), (40, 15)),), grid=(2, 1, 3), vrange=(0, 1), n_photons=100, nprof=10, rho=0.0,
               rayleigh=math.inf, max_steps=10):
    """ldsim_light_lut_build straight through ctypes (the Python layer would refuse most of these itself): (status, message)"""
    P = abi.LdsimLutBuildParams()
    P.box[:] = box
    P.rayleigh_cm, P.absorption_cm, P.group_velocity_cm_ns = rayleigh, math.inf, VG
    P.wall_reflectivity[:] = [rho] * 6
    P.emit_mode, P.max_steps, P.nprof = 0, max_steps, nprof
    D = (abi.LdsimLutDetector * len(dets))()
    for k, (w, lo, hi) in enumerate(dets):
        D[k].wall = w
        D[k].lo[:] = lo
        D[k].hi[:] = hi
    nv, nd, npf = max(vrange[1] - vrange[0], 1), len(dets), min(max(nprof, 1), 512)
    out = [np.zeros((nv, nd), dtype="u4"), np.zeros((nv, nd, npf), dtype="u4"), np.zeros((nv, nd), dtype="f4"),
           np.zeros((nv, nd), dtype="u8"), np.zeros((nv, 3), dtype="u8")]
    rc = lib.load().ldsim_light_lut_build(ctx, C.byref(P), D, C.c_int32(nd), *(C.c_int32(v) for v in grid), C.c_int64(vrange[0]),
                                          C.c_int64(vrange[1]), C.c_int64(n_photons), C.c_uint64(1), *(lib.ptr(a) for a in out))
    return rc, lib.load().ldsim_last_error().decode(), out


def test_refusals():
    """9. every limit returns LDSIM_EINVAL with a message; a build on a context another thread is inside returns LDSIM_ESTATE"""
    H.load_cfg("module0")
    ctx = lib.context()
    EINVAL, ESTATE = -1, -4
    rc, _, out = _raw_build(ctx)
    assert rc == 0 and int(out[0].sum() + out[4].sum()) == 100
    strip = [(2, (0.0, k * 0.02), (30.0, k * 0.02 + 0.01)) for k in range(1025)]             # 1025 disjoint strips on v0
    assert _raw_build(ctx, dets=strip[:1024], n_photons=64)[0] == 0
    cases = {
        "1025 detectors": (dict(dets=strip), "1025 detectors"),
        "no detector": (dict(dets=()), "0 detectors"),
        "nprof": (dict(nprof=513), "nprof 513"),
        "nprof 0": (dict(nprof=0), "nprof 0"),
        "photons": (dict(n_photons=2 ** 31), "n_photons 2147483648"),
        "no photons": (dict(n_photons=0), "n_photons 0"),
        "box": (dict(box=[30.0, 0.0, 30.0]), "zero-sized box"),
        "grid": (dict(grid=(2, 0, 3)), "zero-sized grid"),
        "rectangle": (dict(dets=((0, (20, 5), (40, 5)),)), "zero-sized rectangle"),
        "outside": (dict(dets=((0, (20, 0), (60.5, 15)),)), "outside wall u0"),
        "wall": (dict(dets=((6, (20, 0), (40, 15)),)), "unknown wall 6"),
        "overlap": (dict(dets=((0, (20, 0), (40, 15)), (0, (39, 14), (45, 20)))), "detectors 0 and 1 overlap on wall u0"),
        "reflectivity": (dict(rho=1.0), "wall_reflectivity[u0] = 1"),
        "rayleigh": (dict(rayleigh=0.0), "must be > 0"),
        "max_steps": (dict(max_steps=0), "max_steps"),
        "range": (dict(vrange=(5, 7)), "voxel range [5, 7)"),
    }
    for name, (kw, msg) in cases.items():
        rc, err, _ = _raw_build(ctx, **kw)
        assert rc == EINVAL and msg in err and "ldsim_light_lut_build" in err, (name, rc, err)
    with pytest.raises(lib.LdsimError, match="unknown wall 6|photon range"):
        LB.trace(SIX, GRID1, 0, (5, 2), 1)
    with pytest.raises(lib.LdsimError, match="voxel 6 outside the grid"):
        LB.trace(SIX, GRID1, 6, (0, 10), 1)
    for name, value in (("lut_build_group_photons", 32), ("lut_build_group_photons", 100.5), ("lut_build_lds_tile", 2)):
        with pytest.raises(lib.LdsimError, match=name):
            lib.set_option(name, value)
    # the context still builds, and the same table
    good = LB.build(SIX, GRID1, 2000, 3, _p1(0))
    # busy: a second thread enters while this one is inside a build (the guard is symmetric: whichever is second is refused, has
    # touched nothing, and its call is simply made again)
    refused, other, done = [], [], threading.Event()

    def intruder():
        while not done.is_set():
            rc, err, _ = _raw_build(ctx, n_photons=64)
            if rc == ESTATE:
                refused.append(err)
            elif rc != 0:
                other.append((rc, err))

    th = threading.Thread(target=intruder)
    th.start()
    mine = 0
    try:
        for _ in range(400):
            try:
                again = LB.build(SIX, GRID1, 2000, 3, _p1(0), ctx=ctx)
            except lib.LdsimError as e:
                assert "error -4" in str(e) and "in use by another thread" in str(e)
                mine += 1
                continue
            _assert_same_tallies(again, good, "beside the intruder")
            if refused:
                break
    finally:
        done.set()
        th.join(timeout=60)
    assert not th.is_alive() and not other, other[:3]
    assert refused and all("in use by another thread" in m for m in refused)
