"""GPU: drift-field maps (ChargeChain.set_field_map, simulate_pixels.py --field_map).  A uniform map reproduces the run
without one bit for bit; a constant offset equals shifting the input; a smooth random map matches the numpy restatement
below; the light leg keeps the true positions; the C-ABI validates and refuses.  Every GPU run is a fresh process with a
time limit of its own; nothing is retried."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from larndsim_amd import abi, batching, consts, field_map, synth
from test_gpu_multirank import _assert_same, _inputs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "larnd-sim_amd")
CLI = os.path.join(PKG, "cli", "simulate_pixels.py")
TESTS = os.path.dirname(os.path.abspath(__file__))
POS = ["x_start", "y_start", "z_start", "x_end", "y_end", "z_end", "x", "y", "z"]
DRIFTED = ["n_electrons", "n_photons", "t", "t_start", "t_end", "long_diff", "tran_diff", "pixel_plane"]


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _run(cmd, timeout):
    r = subprocess.run(cmd, env=_env(), capture_output=True, timeout=timeout)
    assert r.returncode == 0, (cmd, r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    return r


def _segments(cfg, n=600, seed=5):
    """batch-sorted segments in the simulation frame, their batch ids"""
    H.load_cfg(cfg)
    seg = synth.make_segments(n, seed=seed, segs_per_event=40)
    batching.swap_coordinates(seg)
    bid, order, _ = batching.assign_batches(seg)
    return np.ascontiguousarray(seg[order]), bid[order].astype(np.int32)


def _box(t):
    b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[t]
    return b.min(axis=1), b.max(axis=1)


def _uniform_maps(shape=(3, 4, 5), **const):
    """a map per TPC over its box (1 cm margin), every channel given in `const` constant"""
    maps = {}
    for t in range(len(consts.detector.TPC_BORDERS)):
        lo, hi = _box(t)
        m = {"origin": lo - 1, "spacing": (hi - lo + 2) / (np.array(shape) - 1)}
        m.update({k: np.full(shape, float(v)) for k, v in const.items()})
        maps[t] = m
    return maps


def _smooth_maps(seed, with_e=True, with_offsets=True):
    rs = np.random.default_rng(seed)
    maps = {}
    for t in range(len(consts.detector.TPC_BORDERS)):
        lo, hi = _box(t)
        shape = tuple(int(v) for v in rs.integers(4, 9, 3))
        sp = (hi - lo) / (np.array(shape) - 3)              # the grid overhangs the box: clamped and interior nodes both used
        org = lo - sp
        g = np.meshgrid(*[np.linspace(0, np.pi, s) for s in shape], indexing="ij")
        ph = rs.uniform(0, np.pi, (4, 3))
        wave = [np.sin(g[0] + ph[c, 0]) * np.cos(g[1] + ph[c, 1]) * np.sin(2 * g[2] + ph[c, 2]) for c in range(4)]
        m = {"origin": org, "spacing": sp}
        if with_e:
            m["E"] = consts.detector.E_FIELD * (1 + 0.3 * wave[0])
        if with_offsets:
            m.update(dx=0.8 * wave[1], dy=-0.6 * wave[2], dz=1.5 * wave[3])
        maps[t] = m
    return maps


# ---- numpy restatement of quench_drift_map_kernel ----------------------------------------------------------------------------
def _tpc_of(c, x, y, z):
    plane = np.full(len(x), c.default_plane_index, dtype=np.int32)
    B = np.ctypeslib.as_array(c.tpc_borders)
    for ip in range(c.n_tpc - 1, -1, -1):                   # (the first TPC that holds the point wins)
        p = B[ip]
        zlo = min(p[2][1] - 2e-2, p[2][0] - 2e-2)
        zhi = max(p[2][1] + 2e-2, p[2][0] + 2e-2)
        inside = ((p[0][0] - 2e-2 <= x) & (x <= p[0][1] + 2e-2) & (p[1][0] - 2e-2 <= y) & (y <= p[1][1] + 2e-2) &
                  (zlo <= z) & (z <= zhi))
        plane[inside] = ip
    return plane


def _eval(m, p):
    """trilinear, edge-clamped, a + f * (b - a) along z, then y, then x: {channel: values at the points p [3][n]}"""
    shape = next(m[c] for c in field_map.CHANNELS if c in m).shape
    inv = 1.0 / np.asarray(m["spacing"], dtype=np.float64)
    i0, f = [], []
    for a in range(3):
        u = np.clip((p[a] - m["origin"][a]) * inv[a], 0.0, shape[a] - 1)
        k = np.minimum(u.astype(np.int64), shape[a] - 2)
        i0.append(k)
        f.append(u - k)
    lerp = lambda a0, a1, t: a0 + t * (a1 - a0)              # noqa: E731
    out = {}
    for ch in field_map.CHANNELS:
        if ch not in m:
            continue
        v = np.asarray(m[ch], dtype=np.float64)
        q = lambda di, dj, dk: v[i0[0] + di, i0[1] + dj, i0[2] + dk]   # noqa: E731
        c00, c01 = lerp(q(0, 0, 0), q(0, 0, 1), f[2]), lerp(q(0, 1, 0), q(0, 1, 1), f[2])
        c10, c11 = lerp(q(1, 0, 0), q(1, 0, 1), f[2]), lerp(q(1, 1, 0), q(1, 1, 1), f[2])
        out[ch] = lerp(lerp(c00, c01, f[1]), lerp(c10, c11, f[1]), f[0])
    return out


def _restate(seg, maps, mode):
    """(anode view [9][n], drifted records) of the segments `seg` (before quench_drift) under `maps`"""
    c = abi.pack_consts(noise_zero=True)
    B = np.ctypeslib.as_array(c.tpc_borders)
    out = seg.copy()
    pos = np.stack([seg[f].astype(np.float64) for f in POS])
    plane = _tpc_of(c, pos[6], pos[7], pos[8])
    view = pos.copy()
    E = np.full(len(seg), c.e_field)
    for t, m in maps.items():
        sel = np.flatnonzero(plane == t)
        if not len(sel):
            continue
        d = np.zeros((9, len(sel)))
        for k0 in (0, 3, 6):
            v = _eval(m, pos[k0:k0 + 3, sel])
            for a, ch in enumerate(("dx", "dy", "dz")):
                d[k0 + a] = v.get(ch, 0.0)
            if k0 == 6 and "E" in v:
                E[sel] = v["E"]
        for k in range(9):
            b = B[t][k % 3]
            lo, hi = np.minimum(min(b), pos[k, sel]), np.maximum(max(b), pos[k, sel])
            view[k, sel] = np.minimum(np.maximum(pos[k, sel] + d[k], lo), hi).astype(seg.dtype[POS[k]]).astype(np.float64)
    dEdx, dE = seg["dEdx"].astype(np.float64), seg["dE"].astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == consts.physics.BOX:
            csi = c.box_beta * dEdx / (E * c.lar_density)
            recomb = np.log(c.box_alpha + csi) / csi
            recomb = np.where(recomb > 0, recomb, 0)
        else:
            recomb = c.birks_ab / (1 + c.birks_kb * dEdx / (E * c.lar_density))
    dt = seg.dtype
    n_e = (recomb * dE / c.w_ion).astype(dt["n_electrons"]).astype(np.float64)
    out["n_electrons"] = n_e
    out["n_photons"] = ((dE / c.w_ph - n_e) * c.scint_prescale).astype(dt["n_photons"])
    out["pixel_plane"] = plane
    ok = plane != c.default_plane_index
    z_anode = B[np.where(ok, plane, 0), 2, 0]
    zs, ze, z = view[2], view[5], view[8]
    t0 = seg["t0"].astype(np.float64)
    drift_time = np.abs(z - z_anode) / c.v_drift
    ds, de = np.abs(np.minimum(zs, ze) - z_anode), np.abs(np.maximum(zs, ze) - z_anode)
    upd = {"n_electrons": n_e * np.exp(-drift_time / c.electron_lifetime),
           "long_diff": np.sqrt(drift_time * 2 * c.long_diff), "tran_diff": np.sqrt(drift_time * 2 * c.tran_diff),
           "t": seg["t"] + (drift_time + t0), "t_start": seg["t_start"] + (np.minimum(ds, de) / c.v_drift + t0),
           "t_end": seg["t_end"] + (np.maximum(ds, de) / c.v_drift + t0)}
    for k, v in upd.items():
        out[k] = np.where(ok, v.astype(dt[k]), out[k])
    return view, out


def _ulps(got, want):
    """|got - want| in units of the last place of the field's dtype (1 for integers)"""
    if np.issubdtype(want.dtype, np.integer):
        return np.abs(got.astype(np.int64) - want.astype(np.int64))
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# ---- chain runs in a fresh process ---------------------------------------------------------------------------------------
_CHAIN = r'''
import sys, pickle
sys.path[:0] = [{pkg!r}, {tests!r}]
import numpy as np
import helpers as H
from larndsim_amd import consts, lib, synth
from larndsim_amd.chain import ChargeChain
job = pickle.load(open({job!r}, "rb"))
H.load_cfg(job["cfg"])
ch = ChargeChain(synth.make_response("survey"))
lut = synth.make_lut((14, 26, 8), 48, 40, 3) if job.get("light") else None
res = []
for run in job["runs"]:
    seg, bid, maps = run["seg"], run["bid"], run.get("maps")
    if maps:
        ch.set_field_map(maps)
    elif run.get("clear", True):
        ch.clear_field_map()
    ch.upload(seg, bid)
    ch.quench_drift(run.get("mode", consts.physics.BIRKS))
    r = dict(segs=ch.download_segments(seg.copy()))
    if maps:
        r["view"] = ch.download_anode_view()
    if lut is not None:
        ch.light_incidence(lut)
        r["light"] = ch.download_light_incidence()[0]
    if run.get("chain", True):
        ch.run(0, len(seg), want_fractions=True)
        r["out"] = ch.download()
        r["compact"] = ch.download_compact()
    res.append(r)
ch.clear_field_map()
pickle.dump(res, open({res!r}, "wb"))
print("chain ok")
'''


def _chain(tmp_path, job, name, timeout=300):
    import pickle
    jp, rp, sp = tmp_path / f"{name}.job", tmp_path / f"{name}.res", tmp_path / f"{name}.py"
    pickle.dump(job, open(jp, "wb"))
    sp.write_text(_CHAIN.format(pkg=PKG, tests=TESTS, job=str(jp), res=str(rp)))
    _run([sys.executable, str(sp)], timeout)
    return pickle.load(open(rp, "rb"))


def _same_results(a, b):
    _assert_same(a["out"], b["out"])
    for k, v in a["compact"].items():
        w = b["compact"][k]
        if isinstance(v, np.ndarray) and v.dtype.names:
            for f in v.dtype.names:
                assert np.array_equal(v[f], w[f]), (k, f)
        else:
            assert np.array_equal(v, w), k


@pytest.mark.parametrize("cfg", ["module0", "2x2_no_modvar"])
def test_uniform_map_is_bit_identical(tmp_path, cfg):
    """E = e_field, zero offsets on every TPC: compact hits, ADC arrays, ticks, track map, fractions and downloaded segments
    equal the run without a map bit for bit; after clear_field_map the no-map outputs come back"""
    seg, bid = _segments(cfg)
    maps = _uniform_maps(E=consts.detector.E_FIELD, dx=0, dy=0, dz=0)
    plain, mapped, cleared = _chain(tmp_path, dict(cfg=cfg, runs=[dict(seg=seg, bid=bid), dict(seg=seg, bid=bid, maps=maps),
                                                                  dict(seg=seg, bid=bid)]), "uniform")
    assert len(plain["out"]["unique_pix"]) > 50 and (plain["out"]["adc_list"] != 0).sum() > 50
    for r in (mapped, cleared):
        _same_results(plain, r)
        _assert_same({"s": plain["segs"]}, {"s": r["segs"]})
    view = np.stack([seg[f].astype(np.float64) for f in POS])
    assert np.array_equal(mapped["view"], view)


def test_constant_offset_equals_shifted_input(tmp_path):
    """a constant (dx, dy, dz) with uniform E against the run without a map whose input positions were moved and rounded in
    numpy: pixel ids, ticks, ADC codes, charges and fractions identical; many points pushed past a border are clamped, and
    every pixel id stays inside the geometry"""
    seg, bid = _segments("module0", n=800)
    maps = {}
    for t in range(len(consts.detector.TPC_BORDERS)):
        lo, hi = _box(t)
        anode = consts.detector.TPC_BORDERS[t][2][0]
        toward = -1.0 if anode < np.mean([lo[2], hi[2]]) else 1.0
        m = _uniform_maps(E=consts.detector.E_FIELD, dx=0.3 * (hi[0] - lo[0]), dy=-0.25 * (hi[1] - lo[1]),
                          dz=toward * 0.2 * (hi[2] - lo[2]))[t]
        maps[t] = m
    view, _ = _restate(seg, maps, consts.physics.BIRKS)
    shifted = seg.copy()
    for k, f in enumerate(POS):
        shifted[f] = view[k]
    B = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)
    on_border = sum(np.isin(view[k], B[:, k % 3].astype(seg.dtype[f]).astype(np.float64)).sum() for k, f in enumerate(POS))
    assert on_border > 100                                  # points pushed past a border and clamped onto it
    a, b = _chain(tmp_path, dict(cfg="module0", runs=[dict(seg=seg, bid=bid, maps=maps), dict(seg=shifted, bid=bid)]), "shift")
    assert np.array_equal(a["view"], view)
    _same_results(a, b)
    for f in DRIFTED:
        assert np.array_equal(a["segs"][f], b["segs"][f]), f
    upix = a["out"]["unique_pix"]
    n_pix = consts.detector.N_PIXELS[0] * consts.detector.N_PIXELS[1] * len(consts.detector.TPC_BORDERS)
    assert len(upix) > 50 and upix.min() >= 0 and upix.max() < n_pix


@pytest.mark.parametrize("cfg", ["module0", "2x2_no_modvar"])
def test_smooth_map_matches_restatement(tmp_path, cfg):
    """a smooth random map on every TPC: the anode view and n_electrons, n_photons, t, t_start, t_end, long_diff, tran_diff
    within one unit in the last place of their stored dtype of the numpy restatement, Box and Birks"""
    seg, bid = _segments(cfg, n=1000, seed=9)
    maps = _smooth_maps(3)
    runs = [dict(seg=seg, bid=bid, maps=maps, mode=mode, chain=False) for mode in (consts.physics.BOX, consts.physics.BIRKS)]
    got = _chain(tmp_path, dict(cfg=cfg, runs=runs), "smooth")
    for r, run in zip(got, runs):
        view, want = _restate(seg, maps, run["mode"])
        g = r["view"]
        assert (g != np.stack([seg[f].astype(np.float64) for f in POS])).sum() > 1000      # the map moved points
        for k, f in enumerate(POS):
            assert _ulps(g[k].astype(seg.dtype[f]), view[k].astype(seg.dtype[f])).max() <= 1, f
        for f in DRIFTED:
            assert _ulps(r["segs"][f], want[f]).max() <= 1, (run["mode"], f)


def test_light_keeps_true_positions(tmp_path):
    """offsets only: light incidence equals the run without a map; E only: n_photons follows the local field (restatement)
    and so does the light"""
    seg, bid = _segments("module0")
    offs = _smooth_maps(4, with_e=False)
    field = _smooth_maps(5, with_offsets=False)
    plain, o, e = _chain(tmp_path, dict(cfg="module0", light=True, runs=[
        dict(seg=seg, bid=bid, chain=False), dict(seg=seg, bid=bid, maps=offs, chain=False),
        dict(seg=seg, bid=bid, maps=field, chain=False)]), "light")
    assert plain["light"]["n_photons_det"].sum() > 0
    _assert_same({"l": plain["light"]}, {"l": o["light"]})
    assert np.array_equal(plain["segs"]["n_photons"], o["segs"]["n_photons"])
    _, want = _restate(seg, field, consts.physics.BIRKS)
    assert _ulps(e["segs"]["n_photons"], want["n_photons"]).max() <= 1
    assert not np.array_equal(e["segs"]["n_photons"], plain["segs"]["n_photons"])
    assert not np.array_equal(e["light"]["n_photons_det"], plain["light"]["n_photons_det"])


_ABI = r'''
import sys
sys.path[:0] = [{pkg!r}, {tests!r}]
import ctypes as C
import numpy as np
import helpers as H
from larndsim_amd import consts, lib, quenching, synth, batching
from larndsim_amd.chain import ChargeChain
from larndsim_amd.layout import make_layout
H.load_cfg("module0")
ch = ChargeChain(synth.make_response("survey"))
L = lib.load()
n_tpc = len(consts.detector.TPC_BORDERS)
def call(tpc, shape, org, sp, E=None, dx=None):
    s = np.array(shape, dtype=np.int64)
    o, p = np.array(org, dtype=np.float64), np.array(sp, dtype=np.float64)
    return L.ldsim_set_field_map(ch.ctx, C.c_int32(tpc), lib.ptr(s), lib.ptr(o), lib.ptr(p), lib.ptr(E), lib.ptr(dx), None, None)
ok = np.ones((2, 3, 2))
bad = [(n_tpc, (2, 3, 2), 0, 1, ok, None, "outside"), (-1, (2, 3, 2), 0, 1, ok, None, "outside"),
       (0, (1, 3, 2), 0, 1, np.ones((1, 3, 2)), None, "dimension"), (0, (2, 3, 2), 0, [1, 0, 1], ok, None, "spacing"),
       (0, (2, 3, 2), 0, [1, np.nan, 1], ok, None, "spacing"), (0, (2, 3, 2), 0, 1, 0 * ok, None, "E["),
       (0, (2, 3, 2), 0, 1, ok.copy(), np.where(ok > 0, np.nan, 0), "dx[")]
for tpc, shape, org, sp, E, dx, msg in bad:
    org = np.broadcast_to(np.asarray(org, dtype=np.float64), (3,)).copy()
    sp = np.broadcast_to(np.asarray(sp, dtype=np.float64), (3,)).copy()
    rc = call(tpc, shape, org, sp, E, dx)
    err = L.ldsim_last_error().decode()
    assert rc == -1 and msg in err, (tpc, shape, rc, err)
seg = synth.make_segments(80, seed=3, segs_per_event=40)
batching.swap_coordinates(seg)
bid, order, _ = batching.assign_batches(seg)
seg, bid = np.ascontiguousarray(seg[order]), bid[order]
assert call(0, (2, 3, 2), [0, 0, 0], [1, 1, 1], ok) == 0
# host-array stage calls refuse while a map is set
lay = make_layout(seg.dtype)
t = seg.copy()
for name, args in [("ldsim_quench", (C.c_int32(2),)), ("ldsim_drift", ())]:
    rc = getattr(L, name)(ch.ctx, lib.ptr(t), C.c_int64(len(t)), C.byref(lay), *args)
    assert rc == -4 and "field map" in L.ldsim_last_error().decode(), (name, rc)
try:
    quenching.quench(t.copy(), consts.physics.BIRKS)
    raise SystemExit("stage quench accepted with a map set")
except lib.LdsimError as e:
    assert "field map" in str(e)
# the chain needs the anode view of the maps set now
ch.upload(seg, bid)
try:
    ch.run(0, len(seg))
    raise SystemExit("chain ran without a mapped quench_drift")
except lib.LdsimError as e:
    assert "changed since" in str(e), str(e)
ch.quench_drift()
ch.run(0, len(seg))
assert call(1, (2, 2, 2), [0, 0, 0], [1, 1, 1], np.ones((2, 2, 2))) == 0
try:
    ch.run(0, len(seg))
    raise SystemExit("chain ran on the view of other maps")
except lib.LdsimError as e:
    assert "changed since" in str(e)
ch.clear_field_map()
try:
    ch.run(0, len(seg))
    raise SystemExit("chain ran on a freed view")
except lib.LdsimError as e:
    assert "changed since" in str(e)
ch.reset()
ch.quench_drift()
ch.run(0, len(seg))
quenching.quench(t.copy(), consts.physics.BIRKS)      # stage calls work again
print("abi ok")
'''


def test_abi_validation_and_refusals(tmp_path):
    p = tmp_path / "abi.py"
    p.write_text(_ABI.format(pkg=PKG, tests=TESTS))
    _run([sys.executable, str(p)], 300)


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _cli(tmp_path, args, name, timeout=600):
    out = tmp_path / name
    r = _run([sys.executable, CLI] + args + ["--output_filename", str(out)], timeout)
    return dict(np.load(out)), r.stdout.decode()


def test_cli_field_map(tmp_path):
    """--field_map: a uniform map writes the datasets of no flag (module0, and 2x2 with module variation); with a smooth map
    --n_gpus 1 --force_dist writes the plain run's file; under --rng keyed --chunk_segments 40 and 100000 agree, also with
    --tracks_current_mc and --raw_arrays"""
    args = _inputs(tmp_path) + ["--chunk_segments", "40"]
    H.load_cfg("module0")
    field_map.save(tmp_path / "map_uni.npz", _uniform_maps(E=consts.detector.E_FIELD, dx=0, dy=0, dz=0))
    field_map.save(tmp_path / "map_smooth.npz", _smooth_maps(6))
    a, log = _cli(tmp_path, args, "plain.npz")
    assert "Drift-field map: none" in log
    b, log = _cli(tmp_path, args + ["--field_map", str(tmp_path / "map_uni.npz")], "uni.npz")
    assert f"Drift-field map: {tmp_path / 'map_uni.npz'}" in log
    _assert_same(a, b)
    c, _ = _cli(tmp_path, args + ["--field_map", str(tmp_path / "map_smooth.npz")], "smooth.npz")
    assert len(c["packets"]) > 100 and not np.array_equal(a["packets"], c["packets"])
    for f in POS:                                           # the file keeps the true positions
        assert np.array_equal(a["segments"][f], c["segments"][f]), f
    d, _ = _cli(tmp_path, args + ["--field_map", str(tmp_path / "map_smooth.npz"), "--n_gpus", "1", "--force_dist"], "dist.npz")
    _assert_same(c, d)
    keyed = args[:-2] + ["--rng", "keyed", "--field_map", str(tmp_path / "map_smooth.npz"), "--tracks_current_mc", "--raw_arrays"]
    e, _ = _cli(tmp_path, keyed + ["--chunk_segments", "40"], "k40.npz")
    f, _ = _cli(tmp_path, keyed + ["--chunk_segments", "100000"], "k1e5.npz")
    _assert_same(e, f)


def test_cli_uniform_map_module_variation(tmp_path):
    """2x2 with module variation: zero offsets and no E channel (E = each module's own e_field) on all of its TPCs write
    the file of no flag"""
    H.load_cfg("2x2_no_modvar")
    seg = synth.make_segments(400, seed=21, segs_per_event=40)
    np.save(tmp_path / "in.npy", seg)
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    field_map.save(tmp_path / "map_uni.npz", _uniform_maps(dx=0, dy=0, dz=0))
    args = ["--input_filename", str(tmp_path / "in.npy"), "--config", "2x2", "--rand_seed", "7", "--response_file",
            str(tmp_path / "resp.npy"), "--light_simulated", "0"]
    a, _ = _cli(tmp_path, args, "plain.npz")
    b, _ = _cli(tmp_path, args + ["--field_map", str(tmp_path / "map_uni.npz")], "uni.npz")
    assert len(a["packets"]) > 50
    _assert_same(a, b)
