"""GPU: the drift-field map builder (csrc/kernels_fmapbuild.hip) -- the conjugate-gradient solve against the direct numpy solve,
the field and trace kernels against the long-double numpy twin, the exact properties, the refusals, a built map through the
charge chain and through the driver.

Bounds.  Solve: with r = b - A psi_gpu formed here in numpy, |r|_2 <= tol |b|_2 (1 + 1e-3) (the stopping rule; 1e-3 for the other
order of the sums) and |psi_gpu - psi_twin|_2 <= (|r|_2 + |b - A psi_twin|_2) / lambda_min, lambda_min the analytic smallest
eigenvalue of the stencil: |A^-1|_2 = 1 / lambda_min, nothing in it comes from the kernel.  Field and trace: fed the twin's psi,
per channel and absolute, four times the largest difference between the f64 twin and the long-double twin of the same case (the
rule of tests/test_gpu_response_builder.py; the factor covers the device's sqrt and division against libm).  Through the chain:
helpers.assert_wave_close at its defaults.
Shapes: (5, 9, 17) at (0.7, 1.1, 0.4) cm -- unequal dimensions and pitches, 765 nodes = 3 chunks, the last one ragged, 45 columns
in a 64-lane wave; (3, 3, 3) -- one interior node; (2, 4, 3) -- none; (33, 20, 9) with n = -1 -- 24 chunks, 660 columns = 10.3
waves per plane; module0's (63, 125, 31), solved once and shared."""
import ctypes as C
import functools
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from larndsim_amd import abi, batching, consts, field_map, field_map_builder as FB, lib, synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "larnd-sim_amd", "cli", "build_field_map.py")


def _params(dims, spacing, n=1, origin=(0.0, 0.0, 0.0), **kw):
    H.load_cfg("module0")
    z_far = origin[2] + (dims[2] - 1) * spacing[2]
    za, zc = (origin[2], z_far) if n > 0 else (z_far, origin[2])
    return FB.params(origin, spacing, dims, za, zc, **kw)


def _grid(name):
    return {"odd": lambda: _params((5, 9, 17), (0.7, 1.1, 0.4), 1, (-1.4, 2.0, -3.0)),
            "one": lambda: _params((3, 3, 3), (1.0, 1.0, 1.0)),
            "none": lambda: _params((2, 4, 3), (1.0, 0.5, 2.0), -1),
            "wide": lambda: _params((33, 20, 9), (0.5, 0.8, 1.2), -1, (3.0, -8.0, 1.0)),
            "module0": lambda: (H.load_cfg("module0"), FB.params(**FB.box_from_consts(0, 1.0)))[1]}[name]()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(params, source, walls or None) of the named case; sources chosen on the CPU so that the twin shows offsets of 0.1 .. 1 cm and
    no reversal"""
    rng = np.random.default_rng(11)
    if name == "odd":
        p = _grid("odd")
        return p, 0.15 * rng.normal(size=p["dims"]), 0.02 * rng.normal(size=p["dims"])
    if name == "one":
        p = _grid("one")
        return p, np.full(p["dims"], 0.3), 0.05 * rng.normal(size=p["dims"])
    if name == "none":
        p = _grid("none")
        return p, np.ones(p["dims"]), 0.05 * rng.normal(size=p["dims"])
    if name in ("wide", "defect"):
        p = _grid("wide")
        if name == "defect":                              # a patch of the x = 0 wall at +0.5 kV: part of the charge ends on the wall
            walls = np.zeros(p["dims"])
            walls[0, 5:15, 2:7] = 0.5
            return p, np.zeros(p["dims"]), walls
        x, y, z = np.arange(33)[:, None, None], np.arange(20)[None, :, None], np.arange(9)[None, None, :]
        blob = 0.05 * np.exp(-((x - 20) ** 2 / 30 + (y - 8) ** 2 / 20 + (z - 4) ** 2 / 4))
        return p, blob + 0.01 * rng.normal(size=p["dims"]), None
    if name == "module0_random":
        p = _grid("module0")
        return p, rng.normal(size=p["dims"]), None
    if name == "module0_cosmic":
        p = _grid("module0")
        return p, FB.cosmic_source(p), None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _solved(name):
    p, s, walls = _case(name)
    psi, it, res = FB.solve(p, s, walls)
    psi.setflags(write=False)
    return psi, it, res, FB.build_ms()[0]


@functools.lru_cache(maxsize=None)
def _twin_psi(name):
    p, s, walls = _case(name)
    psi = FB.solve_twin(p, s, walls)
    psi.setflags(write=False)
    return psi


def _apply(p, v):
    hx, hy, hz = p["spacing"]
    c = v[1:-1, 1:-1, 1:-1]
    return ((2 * c - v[:-2, 1:-1, 1:-1] - v[2:, 1:-1, 1:-1]) / hx ** 2 + (2 * c - v[1:-1, :-2, 1:-1] - v[1:-1, 2:, 1:-1]) / hy ** 2
            + (2 * c - v[1:-1, 1:-1, :-2] - v[1:-1, 1:-1, 2:]) / hz ** 2)


@pytest.mark.parametrize("name", ["odd", "one", "wide", "defect", "module0_random", "module0_cosmic"])
def test_solve_against_the_direct_solve(name):
    p, s, walls = _case(name)
    psi, it, res, ms = _solved(name)
    twin = _twin_psi(name)
    face = np.ones(p["dims"], dtype=bool)
    face[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(psi[face], twin[face])                                 # the walls' values, untouched
    b = np.linalg.norm(FB.rhs(p, s, walls))
    r = np.linalg.norm(s[1:-1, 1:-1, 1:-1] - _apply(p, psi))
    r_twin = np.linalg.norm(s[1:-1, 1:-1, 1:-1] - _apply(p, twin))
    err = np.linalg.norm(psi - twin)
    bound = (r + r_twin) / FB.lambda_min(p)
    print(f"{name}: {it} iterations, {ms:.2f} ms; |r| / |b| {r / b:.3e} (reported {res:.3e}, twin {r_twin / b:.3e}), tol {p['tol']:.0e}; "
          f"|psi - twin| {err:.3e}, bound {bound:.3e}, |psi| {np.linalg.norm(twin):.3e}")
    assert b > 0 and 1 <= it <= p["max_iters"]
    assert r <= p["tol"] * b * (1 + 1e-3)
    assert 0 < res <= p["tol"] and abs(res - r / b) <= 0.1 * p["tol"]        # (near the rounding floor the two orders of summing differ)
    assert err <= bound


def test_no_interior_node_and_zero_right_hand_side():
    p, s, walls = _case("none")
    psi, it, res = FB.solve(p, s, walls)
    assert it == 0 and res == 0.0 and np.array_equal(psi, walls)                 # every node is a wall node
    for name in ("odd", "wide"):
        p = _grid(name)
        psi, it, res = FB.solve(p, np.zeros(p["dims"]))
        assert it == 0 and res == 0.0 and not psi.any()


def _channel_bounds(p, psi):
    """per channel 4 x max |f64 twin - long-double twin|; the f64 twin, the long-double twin"""
    f64 = FB.trace_twin(p, psi, on_reverse="mask")
    ld = FB.trace_twin(p, psi, np.longdouble, on_reverse="mask")
    assert not f64["reversed"].any() and not ld["reversed"].any()
    return {c: 4 * float(np.abs(f64[c] - ld[c]).max()) for c in ("E", "dx", "dy", "dz")}, f64, ld


@pytest.mark.parametrize("name", ["odd", "one", "none", "wide", "defect"])
def test_field_and_trace_against_the_long_double_twin(name):
    p = _case(name)[0]
    psi = _twin_psi(name)                                 # the twin's potential: the solver's tolerance does not enter
    tol, f64, ld = _channel_bounds(p, psi)
    got = FB.trace(p, psi)
    ms = FB.build_ms()
    assert ms[1] > 0 and ms[2] > 0
    for c in ("E", "dx", "dy", "dz"):
        worst = float(np.abs(got[c] - ld[c]).max())
        print(f"{name} {c}: worst |kernel - long-double twin| {worst:.3e}, bound {tol[c]:.3e}, largest value {float(np.abs(ld[c]).max()):.4f}")
        assert got[c].dtype == np.float64 and got[c].shape == p["dims"]
        assert 0 < tol[c] < 1e-9
        assert worst <= tol[c]
    assert 0.1 < max(float(np.abs(ld[c]).max()) for c in ("dx", "dy")) < 5.0
    # the flags: exactly the twin's end points outside the box; the nodes on the anode plane do not move
    assert got["flags"].dtype == np.uint8 and np.array_equal(got["flags"], f64["flags"])
    anode = 0 if FB.drift_sign(p) > 0 else p["dims"][2] - 1
    assert all(not got[c][:, :, anode].any() for c in ("dx", "dy", "dz", "flags"))
    if name == "defect":
        n_flag = int(got["flags"].sum())
        print(f"defect: {n_flag} of {got['flags'].size} nodes end on the field cage")
        assert 0 < n_flag < got["flags"].size and got["flags"][1, 10, 4] == 1 and got["flags"][-1, 10, 4] == 0


def test_exact_properties():
    for name in ("odd", "one", "none", "wide", "module0"):
        p = _grid(name)
        m = FB.build(p, np.zeros(p["dims"]))
        assert np.all(m["E"] == p["E0"]) and all(not m[c].any() for c in ("dx", "dy", "dz")), name      # the nominal map, bit for bit
    for name in ("odd", "wide"):
        p, s, walls = _case(name)
        info = [{}, {}]
        a, b = FB.build(p, s, walls, info=info[0]), FB.build(p, s, walls, info=info[1])
        for c in ("E", "dx", "dy", "dz"):
            assert a[c].tobytes() == b[c].tobytes(), (name, c)                                            # two builds, the same bytes
        assert info[0]["psi"].tobytes() == info[1]["psi"].tobytes() and info[0]["iterations"] == info[1]["iterations"]
        assert info[0]["flags"].tobytes() == info[1]["flags"].tobytes()


@pytest.mark.parametrize("name", ["odd", "wide", "module0_cosmic"])
def test_same_bytes_at_any_number_of_workgroups(name):
    p, s, walls = _case(name)
    ref, it, res, _ = _solved(name)
    try:
        for wgs in (1, 7):
            lib.set_option("fmap_build_wgs", wgs)
            psi, it_w, res_w = FB.solve(p, s, walls)
            assert psi.tobytes() == ref.tobytes() and it_w == it and res_w == res, wgs
    finally:
        lib.set_option("fmap_build_wgs", 0)
    with pytest.raises(lib.LdsimError, match="fmap_build_wgs"):
        lib.set_option("fmap_build_wgs", -1)


def test_errors_leave_the_context_usable():
    p, s, walls = _case("odd")
    good = _solved("odd")[0]
    # 1. one iteration is not enough for a random source
    with pytest.raises(lib.LdsimError) as e:
        FB.solve(dict(p, max_iters=1), s, walls)
    text = str(e.value)
    m = re.search(r"relative residual ([0-9.e+-]+) after 1 iterations", text)
    assert f"ldsim error {abi.LDSIM_ENOCONV}:" in text and "ldsim_field_map_solve" in text and m, text
    assert p["tol"] < float(m.group(1)) < 1.0
    assert FB.solve(p, s, walls)[0].tobytes() == good.tobytes()
    # 2. a space charge that outweighs the nominal field
    big = np.full(p["dims"], 2.0)
    psi = FB.solve_twin(p, big)
    twin = FB.trace_twin(p, psi, on_reverse="mask")["reversed"]
    assert 0 < twin.sum() < twin.size
    with pytest.raises(lib.LdsimError) as e:
        FB.trace(p, psi)
    text = str(e.value)
    m = re.search(r"field reverses on the path of node (\d+) \(i, j, k\) = \((\d+), (\d+), (\d+)\)", text)
    assert f"ldsim error {abi.LDSIM_EINVAL}:" in text and "ldsim_field_map_trace" in text and m, text
    node = int(m.group(1))
    assert np.unravel_index(node, p["dims"]) == tuple(int(v) for v in m.groups()[1:]) and twin.reshape(-1)[node]
    assert node == int(np.flatnonzero(twin.reshape(-1))[0])                       # the lowest one
    with pytest.raises(FB.FieldMapBuildError, match=f"field reverses on the path of node {node} "):
        FB.trace_twin(p, psi)
    got = FB.trace(p, _twin_psi("odd"))
    assert np.abs(got["dx"]).max() > 0.1


def _raw(ctx, which, null=None, source=None, walls=None, **kw):
    """ldsim_field_map_solve / _trace straight through ctypes (the Python layer refuses these itself): (status, message)"""
    d = dict(origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), z_anode=0.0, z_cathode=4.0, e0=0.5, temperature=87.17,
             mobility=(551.6, 7158.3, 4440.43, 4.29, 43.63, 0.2053), tol=1e-12, step=0.5, n=(4, 4, 5), max_iters=100, check_every=8)
    d.update(kw)
    P = abi.LdsimFieldMapBuildParams()
    for k, v in d.items():
        if k in ("origin", "spacing", "mobility", "n"):
            getattr(P, k)[:] = v
        else:
            setattr(P, k, v)
    shape = tuple(max(int(v), 2) for v in d["n"]) if np.prod([max(int(v), 1) for v in d["n"]]) < 1e6 else (2, 2, 2)
    arr = {k: np.zeros(shape) for k in ("source", "psi", "E", "dx", "dy", "dz")}
    arr["source"][...] = 0.01
    if source is not None:
        arr["source"].reshape(-1)[source[0]] = source[1]
    if walls is not None:
        arr["psi"].reshape(-1)[walls[0]] = walls[1]
    flags = np.zeros(shape, dtype=np.uint8)
    L = lib.load()
    a = {k: (None if k == null else lib.ptr(v)) for k, v in arr.items()}
    if which == "solve":
        it, res = C.c_int32(), C.c_double()
        rc = L.ldsim_field_map_solve(ctx, None if null == "params" else C.byref(P), a["source"], a["psi"],
                                     None if null == "iterations" else C.byref(it), None if null == "residual" else C.byref(res))
    else:
        rc = L.ldsim_field_map_trace(ctx, None if null == "params" else C.byref(P), a["psi"], a["E"], a["dx"], a["dy"], a["dz"],
                                     None if null == "flags" else lib.ptr(flags))
    return rc, L.ldsim_last_error().decode()


def test_library_refusals():
    ctx = lib.context()
    nan, inf = float("nan"), float("inf")
    for which, entry in (("solve", "ldsim_field_map_solve"), ("trace", "ldsim_field_map_trace")):
        assert _raw(ctx, which)[0] == 0
        cases = [(dict(spacing=(1.0, 0.0, 1.0)), "spacing[y]"), (dict(spacing=(nan, 1.0, 1.0)), "spacing[x]"),
                 (dict(spacing=(1.0, 1.0, -1.0)), "spacing[z]"), (dict(spacing=(1.0, inf, 1.0)), "spacing[y]"),
                 (dict(e0=0.0), "E0"), (dict(e0=nan), "E0"), (dict(temperature=-1.0), "temperature"), (dict(temperature=inf), "temperature"),
                 (dict(tol=0.0), "tol"), (dict(tol=nan), "tol"), (dict(step=0.0), "step"), (dict(step=inf), "step"),
                 (dict(step=1e-7), "steps on the longest path"),
                 (dict(n=(1, 4, 5)), "dimension nx = 1"), (dict(n=(4, 4, 1)), "dimension nz = 1"), (dict(n=(2048, 2048, 512)), "exceed 2^31 - 1"),
                 (dict(z_cathode=0.0), "z_anode == z_cathode"), (dict(z_anode=nan), "finite planes"),
                 (dict(mobility=(0.0, 1.0, 1.0, 1.0, 1.0, 1.0)), "mobility[0]"), (dict(mobility=(1.0, 1.0, nan, 1.0, 1.0, 1.0)), "mobility[2]"),
                 (dict(max_iters=0), "max_iters"), (dict(check_every=0), "check_every"), (dict(origin=(0.0, nan, 0.0)), "origin[y]")]
        for kw, msg in cases:
            rc, text = _raw(ctx, which, **kw)
            assert rc == abi.LDSIM_EINVAL and entry in text and msg in text, (which, kw, rc, text)
        nulls = ("params", "source", "psi", "iterations", "residual") if which == "solve" else ("params", "psi", "E", "dx", "dy", "dz", "flags")
        for null in nulls:
            rc, text = _raw(ctx, which, null=null)
            assert rc == abi.LDSIM_EINVAL and entry in text and "null argument" in text, (which, null, text)
        assert _raw(ctx, which)[0] == 0                                           # the context is still usable
    for v in (nan, inf):
        rc, text = _raw(ctx, "solve", source=(27, v))
        assert rc == abi.LDSIM_EINVAL and "ldsim_field_map_solve: source[27]" in text, text
        rc, text = _raw(ctx, "solve", walls=(3, v))                               # node (0, 0, 3): on a wall
        assert rc == abi.LDSIM_EINVAL and "boundary value psi[3]" in text, text
        rc, text = _raw(ctx, "trace", walls=(27, v))
        assert rc == abi.LDSIM_EINVAL and "ldsim_field_map_trace: psi[27]" in text, text
    assert _raw(ctx, "solve", walls=(27, nan))[0] == 0                            # node (1, 1, 2) is inside: not read
    assert _raw(ctx, "solve")[0] == 0 and _raw(ctx, "trace")[0] == 0
    ms = (C.c_double * 3)()
    assert lib.load().ldsim_field_map_build_ms(ctx, ms) == 0 and all(v > 0 for v in ms)
    assert lib.load().ldsim_field_map_build_ms(ctx, None) == abi.LDSIM_EINVAL


# ---- through the chain ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _module0_maps():
    """TPC 0 of module0 under the cosmic profile: the kernels' map, the twin's map"""
    p, s, _ = _case("module0_cosmic")
    info = {}
    gpu = FB.build(p, s, info=info)
    twin = FB.build_twin(p, s)
    return p, gpu, twin, info


def _launch(ch, seg, bid, maps):
    if maps:
        ch.set_field_map(maps)
    else:
        ch.clear_field_map()
    ch.upload(seg, bid)
    ch.quench_drift()
    ch.run(0, len(seg), want_fractions=True)
    return {k: np.array(v) for k, v in ch.download().items()}


def test_built_map_through_the_chain():
    from larndsim_amd.chain import ChargeChain
    p, gpu, twin, info = _module0_maps()
    for c in ("E", "dx", "dy", "dz"):
        print(f"module0 TPC 0, {c}: kernels {gpu[c].min():+.6f} .. {gpu[c].max():+.6f}, |kernels - twin| <= {np.abs(gpu[c] - twin[c]).max():.3e}")
    print(f"{info['iterations']} iterations, relative residual {info['residual']:.3e}, {int(info['flags'].sum())} flagged nodes")
    assert np.abs(gpu["dx"]).max() > 1e-3 and np.abs(gpu["dz"]).max() > 1e-3 and not info["flags"].any()
    H.load_cfg("module0")
    seg = synth.make_segments(320, seed=5, segs_per_event=40)
    batching.swap_coordinates(seg)
    bid, order, _ = batching.assign_batches(seg)
    seg, bid = np.ascontiguousarray(seg[order]), bid[order].astype(np.int32)
    ch = ChargeChain(synth.make_response("survey"))
    try:
        plain = _launch(ch, seg, bid, None)
        with_gpu = _launch(ch, seg, bid, {0: gpu})
        with_twin = _launch(ch, seg, bid, {0: twin})
        zero = FB.build(p, np.zeros(p["dims"]))
        with_zero = _launch(ch, seg, bid, {0: zero})
    finally:
        ch.clear_field_map()
    assert len(plain["unique_pix"]) > 50 and (plain["adc_list"] != 0).sum() > 50
    assert set(with_zero) == set(plain)
    for k in plain:                                                               # a zero source: the launch without a map, bit for bit
        assert np.array_equal(with_zero[k], plain[k], equal_nan=True), k
    assert np.array_equal(with_gpu["unique_pix"], with_twin["unique_pix"])
    assert np.array_equal(with_gpu["adc_ticks_list"], with_twin["adc_ticks_list"])
    H.assert_wave_close(with_gpu["adc_list"], with_twin["adc_list"], what="adc_list under the kernels' map and the twin's")
    changed = (not np.array_equal(with_gpu["unique_pix"], plain["unique_pix"])
               or not np.array_equal(with_gpu["adc_list"], plain["adc_list"]))
    assert changed                                                                # the cosmic map does move charge


def test_tool_file_through_the_driver(tmp_path, capsys):
    """build_field_map.py on the GPU writes a file; simulate_pixels.py --field_map takes it"""
    H.load_cfg("module0")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONHOME"}
    out = tmp_path / "field_map.npz"
    r = subprocess.run([sys.executable, TOOL, "--config", "module0", "--pitch", "2", "--output", str(out)], capture_output=True,
                       text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "on the GPU" in r.stdout and "TPC 0: 32 x 63 x 16 nodes, drift direction n = +1" in r.stdout and "TPC 1:" in r.stdout
    maps = field_map.load(out, 2)
    assert set(maps) == {0, 1} and maps[1]["E"].shape == (32, 63, 16)
    p = FB.params(**FB.box_from_consts(1, 2.0))
    want = FB.build(p, FB.cosmic_source(p))
    assert all(maps[1][c].tobytes() == want[c].tobytes() for c in ("E", "dx", "dy", "dz"))
    spec = importlib.util.spec_from_file_location("sp_cli_field_map_builder", os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    np.save(tmp_path / "in.npy", synth.make_segments(60, seed=10, segs_per_event=30))
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    try:
        cli.run_simulation(str(tmp_path / "in.npy"), str(tmp_path / "out.npz"), config="module0", rand_seed=1,
                           response_file=str(tmp_path / "resp.npy"), light_simulated=False, field_map=str(out))
    finally:
        H.load_cfg("module0")
        lib.check(lib.load().ldsim_clear_field_maps(lib.context()))
    log = capsys.readouterr().out
    assert f"Drift-field map: {out}" in log
    with np.load(tmp_path / "out.npz") as f:
        n_hits = int((f["packets"]["packet_type"] == 0).sum())
    print(f"{n_hits} data packets")
    assert n_hits > 0
