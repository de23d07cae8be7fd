"""CPU: the light LUT builder's host side (larndsim_amd/lut_builder.py, cli/build_light_lut.py) -- struct layouts against the
header text, geometry validation, the numpy twin's sampling laws and its pure-geometry visibility against the closed form, the
table made from tallies, the tool's argument handling.  No GPU call."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from larndsim_amd import abi, lib, lut_builder as LB, rng, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "larnd-sim_amd", "cli", "build_light_lut.py")
BOX = [30.0, 60.0, 30.0]
# the three rectangles on u0 (in-plane coordinates (v, w)) seen from (7.5, 30, 5), the centre of voxel 0 of a (2, 1, 3) grid
RECTS = [LB.detector("u0", (20, 0), (40, 15)), LB.detector("u0", (40, 15), (60, 30))]
FULL = [LB.detector("u0", (0, 0), (60, 30))]
POINT = (7.5, 30.0, 5.0)

CTYPE = {"double": C.c_double, "int32_t": C.c_int32}


def _struct_fields(name):
    """[(field, ctypes type)] of `typedef struct <name> { ... }` as include/ldsim.h spells it"""
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
    for name, cls, size in (("LdsimLutBuildParams", abi.LdsimLutBuildParams, 112), ("LdsimLutDetector", abi.LdsimLutDetector, 40)):
        fields = _struct_fields(name)
        assert [f for f, _ in fields] == [f for f, _ in cls._fields_], name
        for (f, t), (_, mine) in zip(fields, cls._fields_):
            if hasattr(t, "_length_"):
                assert (t._length_, t._type_) == (mine._length_, mine._type_), (name, f)
            else:
                assert t is mine, (name, f)
        assert C.sizeof(cls) == size
    p = abi.LdsimLutBuildParams
    assert (p.box.offset, p.rayleigh_cm.offset, p.absorption_cm.offset, p.group_velocity_cm_ns.offset) == (0, 24, 32, 40)
    assert (p.wall_reflectivity.offset, p.emit_mode.offset, p.max_steps.offset, p.nprof.offset) == (48, 96, 100, 104)
    d = abi.LdsimLutDetector
    assert (d.wall.offset, d.lo.offset, d.hi.offset) == (0, 8, 24)
    hdr = open(os.path.join(REPO, "include", "ldsim.h")).read()
    for entry in ("ldsim_light_lut_build", "ldsim_light_lut_trace", "ldsim_light_lut_build_ms"):
        assert re.search(r"\bint " + entry + r"\(ldsim_ctx\* ctx", hdr), entry
        assert entry in lib.EXPORTS and hasattr(lib.load(), entry)
    assert "#define LDSIM_LUT_MAX_DETECTORS 1024" in hdr and abi.LUT_MAX_DETECTORS == LB.MAX_DETECTORS == 1024
    assert "#define LDSIM_LUT_MAX_NPROF 512" in hdr and abi.LUT_MAX_NPROF == LB.MAX_NPROF == 512
    assert rng.TAG_LUT == 6 and "RNG_TAG_LUT = 6" in open(os.path.join(REPO, "larnd-sim_amd", "csrc", "rng.h")).read()
    assert lib.load().ldsim_abi_version() == abi.ABI_VERSION == 8


def test_geometry_validation_names_the_entry(tmp_path):
    good = {"box": BOX, "detectors": RECTS}
    box, dets = LB.validate(good)
    assert list(box) == BOX and [w for w, _, _ in dets] == [0, 0]
    LB.dump(tmp_path / "g.json", good)
    assert LB.read(tmp_path / "g.json") == good

    def bad(match, **kw):
        with pytest.raises(LB.GeometryError, match=match):
            LB.validate(dict(good, **kw))

    bad(r"detectors\[2\]: overlaps detectors\[0\] on wall u0", detectors=RECTS + [LB.detector("u0", (39.9, 14), (50, 15))])
    LB.validate(dict(good, detectors=RECTS + [LB.detector("u0", (40, 0), (50, 15))]))          # touching is no overlap
    LB.validate(dict(good, detectors=RECTS + [LB.detector("u1", (20, 0), (40, 15))]))          # nor the same rectangle on another wall
    bad(r"detectors\[1\]: .*lies off wall v0", detectors=[RECTS[0], LB.detector("v0", (0, 0), (30.5, 30))])
    bad(r"detectors\[0\]: .*lies off wall w1", detectors=[LB.detector("w1", (-0.1, 0), (30, 60))])
    bad(r"detectors\[1\]: unknown wall 'x0'", detectors=[RECTS[0], {"wall": "x0", "lo": [0, 0], "hi": [1, 1]}])
    bad(r"detectors\[0\]: zero-sized rectangle", detectors=[LB.detector("u0", (20, 5), (20, 15))])
    bad(r"box: three finite lengths > 0", box=[30, 0, 30])
    bad(r"box: three finite lengths > 0", box=[30, -60, 30])
    bad(r"detectors: a list of 1 .. 1024", detectors=[])
    with pytest.raises(LB.GeometryError, match=r"wall_reflectivity\[v1\] = 1.0"):
        LB.params(wall_reflectivity=[0, 0, 0, 1.0, 0, 0])
    with pytest.raises(LB.GeometryError, match="rayleigh_cm and absorption_cm"):
        LB.params(rayleigh_cm=0.0)
    with pytest.raises(LB.GeometryError, match="rayleigh_cm and absorption_cm"):
        LB.params(absorption_cm=-3.0)
    with pytest.raises(LB.GeometryError, match="group_velocity_cm_ns"):
        LB.params(group_velocity_cm_ns=0.0)
    with pytest.raises(LB.GeometryError, match="nprof"):
        LB.params(nprof=513)
    assert LB.params(rayleigh_cm=math.inf, wall_reflectivity=0.999)["wall_reflectivity"] == [0.999] * 6


def test_tile_wall_and_box_from_consts():
    tiles = LB.tile_wall("v1", 3, 2, BOX, gap=0.5)                  # v walls: in-plane (w, u) = 30 x 30
    assert len(tiles) == 6 and all(t["wall"] == "v1" for t in tiles)
    LB.validate({"box": BOX, "detectors": tiles})
    w = (30 - 4 * 0.5) / 3
    assert tiles[0]["lo"] == [0.5, 0.5] and tiles[0]["hi"][0] == pytest.approx(0.5 + w)
    assert tiles[-1]["hi"][0] == pytest.approx(29.5) and tiles[-1]["hi"][1] == pytest.approx(29.5)
    assert tiles[1]["lo"][0] == tiles[0]["lo"][0] and tiles[1]["lo"][1] > tiles[0]["hi"][1]      # second coordinate fastest
    LB.validate({"box": BOX, "detectors": LB.tile_wall("u0", 6, 4, BOX)})                        # gap 0: touching, no overlap
    with pytest.raises(LB.GeometryError, match="leaves no room"):
        LB.tile_wall("u0", 2, 2, BOX, gap=12.0)
    from larndsim_amd import consts
    consts.load_snapshot("module0")
    b = np.asarray(consts.detector.TPC_BORDERS)
    for itpc in (0, 1):
        assert LB.box_from_consts(itpc) == [abs(b[itpc, k, 1] - b[itpc, k, 0]) + 0.04 for k in range(3)]


def _numpy_uniforms(n, stream):
    """n keyed uniforms (f32 in (0, 1], widened) of one stream, made in numpy"""
    u = rng.keyed_block_uniforms(11, rng.TAG_LUT, np.full((n + 3) // 4, stream, dtype=np.uint64), np.arange((n + 3) // 4))
    return u.astype(np.float64).ravel()[:n]


def test_rayleigh_inverse_has_the_moments_of_the_law():
    """mu ~ (3/8)(1 + mu^2) on [-1, 1]: <mu> = 0, <mu^2> = 2/5; var(mu) = 2/5, var(mu^2) = <mu^4> - 4/25 = 9/35 - 4/25"""
    n = 2_000_000
    mu = LB.rayleigh_mu(_numpy_uniforms(n, 1))
    assert mu.min() >= -1.0 and mu.max() <= 1.0
    assert abs(mu.mean()) <= 5 * math.sqrt(0.4 / n), mu.mean()
    assert abs((mu * mu).mean() - 0.4) <= 5 * math.sqrt((9 / 35 - 4 / 25) / n), (mu * mu).mean()


def test_lambert_draw_has_mean_cosine_two_thirds():
    """cos theta = sqrt(u): density 2 cos theta, <cos> = 2/3, var = 1/2 - 4/9"""
    n = 200_000
    c = LB.lambert_cos(_numpy_uniforms(n, 2))
    assert abs(c.mean() - 2 / 3) <= 5 * math.sqrt((0.5 - 4 / 9) / n), c.mean()


@pytest.mark.parametrize("dets,expect", [(RECTS, ((0.1837, 5e-5), (0.00997, 5e-6))), (FULL, ((0.2802, 5e-5),))],
                         ids=["two", "full_wall"])
def test_twin_pure_geometry_matches_the_solid_angle(dets, expect):
    n = 200_000
    geo = {"box": BOX, "detectors": dets}
    omega = [LB.solid_angle_visibility(POINT, d, BOX) for d in dets]
    for o, (e, half_digit) in zip(omega, expect):
        assert abs(o - e) <= half_digit, (o, e)                    # the figures this case was set up with, as rounded there
        assert n * o >= 1000
    tr = LB.trace_twin(geo, (2, 1, 3), 0, (0, n), 5, LB.params(emit_mode=1))
    assert (tr["steps"] == 1).all() and set(np.unique(tr["fate"])) <= {LB.FATE_WALL, 0, 1}
    t = LB.tally(tr, len(dets), 100)
    assert int(t["count"].sum() + t["fates"].sum()) == n and t["fates"][0] == 0 and t["fates"][2] == 0
    for k, o in enumerate(omega):
        vis = t["count"][k] / n
        assert abs(vis - o) <= 5 * math.sqrt(o * (1 - o) / n), (k, vis, o)
    hit = tr["fate"] >= 0
    assert (tr["end"][hit, 0] == 0.0).all()                        # put on the wall exactly
    r = np.linalg.norm(tr["end"][hit] - np.array(POINT), axis=1)
    np.testing.assert_allclose(tr["time"][hit], r / LB.GROUP_VELOCITY_CM_NS, rtol=1e-12)


def test_twin_is_a_function_of_the_photon_not_of_the_range():
    geo = {"box": BOX, "detectors": RECTS + [LB.detector("v1", (0, 0), (30, 30))]}
    p = LB.params(rayleigh_cm=20, absorption_cm=80, wall_reflectivity=[0.5, 0.5, 0.3, 0.3, 0, 0], max_steps=50)
    whole = LB.trace_twin(geo, (2, 1, 3), 4, (0, 3000), 9, p)
    part = LB.trace_twin(geo, (2, 1, 3), 4, (1000, 2000), 9, p)
    for k in whole:
        assert np.array_equal(whole[k][1000:2000], part[k]), k
    assert {LB.FATE_BULK, LB.FATE_WALL} <= set(np.unique(whole["fate"])) and (whole["fate"] >= 0).any()
    other = LB.trace_twin(geo, (2, 1, 3), 4, (0, 3000), 10, p)
    assert not np.array_equal(other["fate"], whole["fate"])
    cut = LB.trace_twin(geo, (2, 1, 3), 4, (0, 3000), 9, dict(p, max_steps=3))
    assert (cut["fate"] == LB.FATE_TRUNCATED).any() and cut["steps"].max() == 3
    same = cut["fate"] != LB.FATE_TRUNCATED
    assert np.array_equal(cut["fate"][same], whole["fate"][same]) and (whole["steps"][~same] > 3).all()


def test_to_lut_from_tallies():
    nprof = 20
    geo = {"box": BOX, "detectors": RECTS + [LB.detector("u1", (0, 0), (1, 1))]}
    p = LB.params(rayleigh_cm=30, wall_reflectivity=0.4, nprof=nprof)
    rows = [LB.tally(LB.trace_twin(geo, (2, 1, 3), v, (0, 4000), 3, p), 3, nprof) for v in range(6)]
    t = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    t["n_photons"], t["voxel_range"] = 4000, (0, 6)
    t["count"][5, 2], t["hist"][5, 2], t["tsum"][5, 2], t["tmin"][5, 2] = 0, 0, 0, np.inf        # (an unlit cell for certain)
    lut = LB.to_lut(t, (2, 1, 3))
    assert lut.dtype == synth.lut_dtype(nprof) and lut.shape == (2, 1, 3, 3)
    lit = t["count"].reshape(2, 1, 3, 3) > 0
    assert lit.any() and (~lit).any()
    np.testing.assert_allclose(lut["time_dist"].sum(axis=-1)[lit], 1.0, rtol=1e-6)
    assert (lut["time_dist"][~lit] == 0).all() and (lut["t0"][~lit] == 0).all() and (lut["vis"][~lit] == 0).all()
    assert (lut["t0"][lit] <= lut["t0_avg"][lit] * (1 + 1e-6)).all() and (lut["t0"][lit] > 0).all()
    np.testing.assert_array_equal(lut["vis"], (t["count"] / 4000).astype("f4").reshape(2, 1, 3, 3))
    with pytest.raises(ValueError, match="do not fill"):
        LB.to_lut(t, (2, 2, 3))
    assert LB.to_lut(t).shape == (6, 3)


def _tool(*args):
    env = {k: v for k, v in os.environ.items() if k != "PYTHONHOME"}
    return subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True, env=env, timeout=120)


def test_tool_help_and_argument_errors(tmp_path):
    r = _tool("--help")
    assert r.returncode == 0
    for flag in ("--geometry", "--vox_div", "--photons", "--seed", "--rayleigh_cm", "--absorption_cm", "--group_velocity_cm_ns",
                 "--wall_reflectivity", "--emit", "--max_steps", "--nprof", "--voxel_range", "--output"):
        assert flag in r.stdout, flag
    geo = tmp_path / "g.json"
    geo.write_text(json.dumps({"box": BOX, "detectors": RECTS}))
    base = ["--geometry", str(geo), "--vox_div", "2", "1", "3", "--photons", "100", "--output", str(tmp_path / "o.npz")]
    for extra, msg in ((["--emit", "corner"], "invalid choice"), (["--wall_reflectivity", "1.0"], r"wall_reflectivity\[u0\] = 1.0"),
                       (["--rayleigh_cm", "0"], "a length > 0"), (["--voxel_range", "2", "9"], "--voxel_range"),
                       (["--wall_reflectivity", "0.1", "0.2"], "one value or six"), (["--nprof", "600"], "nprof")):
        r = _tool(*base, *extra)
        assert r.returncode == 2 and re.search(msg, r.stderr), (extra, r.stderr)
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"box": BOX, "detectors": RECTS + [LB.detector("u0", (30, 10), (45, 20))]}))
    r = _tool(*(base[:1] + [str(bad)] + base[2:]))
    assert r.returncode == 2 and "overlaps detectors[0]" in r.stderr
    r = _tool(*base[2:])
    assert r.returncode == 2 and "--geometry" in r.stderr
    assert not (tmp_path / "o.npz").exists()
