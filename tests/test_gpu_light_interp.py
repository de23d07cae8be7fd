"""GPU: trilinear LUT visibility (context option light_lut_interp: light_incidence_interp_kernel and its four-channel form)
against the numpy twin larndsim_amd/lightLUT.py: interpolated_light_incidence.

The bound of the parity checks is derived, not measured: kernel and twin do the same f64 operations in the same order (the
library is built without contraction into fused multiply-adds; a compiler that contracted one would move a sum by ~1e-16
relative), so at most the final rounding to f4 can differ: 1 f4 ulp of the expected value, everywhere.
The shapes are the smallest at which each branch can go wrong -- partial tiles (n = 1, 33, 70 at 32 segments a tile), a LUT with
an axis of one voxel and a detector count that forces the one-channel form, one that takes the four-channel form -- not the
workload's."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import light_interp_cases as LC
from test_h5_io import h5_python
from larndsim_amd import consts, lib, light_sim, lightLUT
from larndsim_amd.chain import ChargeChain
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INC_DTYPE = [('segment_id', 'u4'), ('n_photons_det', 'f4'), ('t0_det', 'f4')]
LUTS = {"scalar_2x1x3": ((2, 1, 3), 6), "quad_3x4x2": ((3, 4, 2), 8), "full_14x26x8": ((14, 26, 8), 48)}
# (configuration, per-module channel slice): module0 -- threshold trigger, t0_det written; 2x2 -- beam trigger, 8 TPCs, and
# with the slice n_out < N_OP_CHANNEL (the channel tables' slice then follows the segment's TPC)
CONFIGS = {"module0": ("module0", False), "2x2": ("2x2_no_modvar", False), "2x2_slice": ("2x2_no_modvar", True)}


@functools.lru_cache(maxsize=None)
def _lut(name):
    vox_div, ndet = LUTS[name]
    return LC.small_lut(vox_div, ndet, 500 + len(name) + ndet)          # (kept alive: lib.set_light tells tables apart by address)


def _n_out(per_module):
    n_op = consts.light.N_OP_CHANNEL
    return 2 * n_op // len(consts.detector.TPC_BORDERS) if per_module else n_op


def _stage(r, lut, n_out):
    inc = np.zeros((len(r), n_out), dtype=INC_DTYPE)
    vox = np.full((len(r), 3), -1, dtype='i4')
    lightLUT.calculate_light_incidence[1, 256](r, lut, inc, vox)
    return inc['n_photons_det'].copy(), inc['t0_det'].copy(), vox


def _resident(r, lut, n_out):
    ch = ChargeChain()
    ch.upload(r, np.zeros(len(r), dtype=np.int32))
    ch.light_incidence(lut, n_out=n_out)
    inc, vox = ch.download_light_incidence()
    return inc['n_photons_det'].copy(), inc['t0_det'].copy(), vox


def _all_forms(r, lut, n_out, interp):
    """{(light_incidence_scalar, stage call | resident leg): (n_photons_det, t0_det, voxel)} under light_lut_interp = interp"""
    got = {}
    lib.context()
    try:
        lib.set_option("light_lut_interp", interp)
        for scalar in (0, 1):
            lib.set_option("light_incidence_scalar", scalar)
            got[(scalar, "stage")] = _stage(r, lut, n_out)
            got[(scalar, "resident")] = _resident(r, lut, n_out)
    finally:
        lib.set_option("light_incidence_scalar", 0)
        lib.set_option("light_lut_interp", 0)
    return got


@pytest.mark.parametrize("n", [1, 33, 70])
@pytest.mark.parametrize("lut_name", ["scalar_2x1x3", "quad_3x4x2"])
@pytest.mark.parametrize("cfg_name", list(CONFIGS))
def test_parity_with_the_twin_and_between_the_forms(cfg_name, lut_name, n):
    """n_photons_det and t0_det within 1 f4 ulp of the twin, voxel identical; four-channel form, one-channel form, stage call
    and resident leg bit-identical to one another.  Positions: uniform, within 1e-3 cm of every border, on voxel centres, on
    voxel faces; some rows outside every TPC."""
    cfg, per_module = CONFIGS[cfg_name]
    H.load_cfg(cfg)
    lut = _lut(lut_name)
    vox_div = LUTS[lut_name][0]
    r = LC.mixed_segments(n, vox_div, seed=1000 + n)
    if n == 1:
        assert r["pixel_plane"][0] != consts.detector.DEFAULT_PLANE_INDEX
    n_out = _n_out(per_module)
    exp = lightLUT.interpolated_light_incidence(r, lut, n_out)
    got = _all_forms(r, lut, n_out, 1)
    first = got[(0, "stage")]
    for key, g in got.items():
        for a, b, what in zip(g, first, ("n_photons_det", "t0_det", "voxel")):
            assert a.tobytes() == b.tobytes(), (key, what)
    nph, t0d, vox = first
    assert np.array_equal(vox, exp[2])
    assert LC.ulp_close(nph, exp[0]), np.abs(nph - exp[0]).max()
    assert LC.ulp_close(t0d, exp[1]), np.abs(t0d - exp[1]).max()
    inside = r["pixel_plane"] != consts.detector.DEFAULT_PLANE_INDEX
    assert (nph[inside] > 0).any(axis=1).all() and (nph[~inside] == 0).all()
    if consts.light.LIGHT_TRIG_MODE == 0:
        assert (t0d[inside] > 0).all()
    # the nearest-voxel result is another one (the option does something) wherever a segment is off its voxel's centre
    # (with the option off the stage call is the reference's: rows outside every TPC keep the -1 the voxel array was handed in with)
    near, _, near_vox = _stage(r, lut, n_out)
    assert np.array_equal(near_vox[inside], vox[inside]) and (near_vox[~inside] == -1).all()
    if n > 1:
        assert (near != nph).any()


def test_parity_on_the_production_lut_shape():
    """(14, 26, 8) voxels, 48 detectors, 300 segments of every kind over module0's two TPCs: the same checks, and some dark
    corners (visibility 0 in a tenth of the table): t0_det takes the lit corners only."""
    H.load_cfg("module0")
    lut = _lut("full_14x26x8").copy()
    rng = np.random.default_rng(77)
    lut["vis"][rng.random(lut["vis"].shape) < 0.1] = 0.0
    r = LC.mixed_segments(300, (14, 26, 8), seed=78, outside_every=97)
    exp = lightLUT.interpolated_light_incidence(r, lut)
    got = _all_forms(r, lut, consts.light.N_OP_CHANNEL, 1)
    first = got[(0, "stage")]
    for key, g in got.items():
        for a, b, what in zip(g, first, ("n_photons_det", "t0_det", "voxel")):
            assert a.tobytes() == b.tobytes(), (key, what)
    assert np.array_equal(first[2], exp[2])
    assert LC.ulp_close(first[0], exp[0]) and LC.ulp_close(first[1], exp[1])
    assert (first[0] > 0).sum() > 10_000


def test_continuity_across_a_voxel_face():
    """Two positions 1e-6 cm either side of an interior voxel face of the (14, 26, 8) LUT, for a face of each axis.  Nearest voxel:
    the light yield steps by the LUT's own voxel-to-voxel difference, more than 1e-3 relative on some channel.  Trilinear: the two
    differ by less than 1e-4 relative on every channel -- the step times 2e-6 cm over a voxel width of more than 1 cm is 1e-6
    of a value that is at least half the larger side, two orders below the bound."""
    H.load_cfg("module0")
    vox_div = (14, 26, 8)
    lut = _lut("full_14x26x8")
    b = np.sort(np.asarray(consts.detector.TPC_BORDERS)[0], axis=-1)
    assert ((b[:, 1] - b[:, 0]) / np.array(vox_div) > 1.0).all()              # voxel widths in cm
    xs, ys, zs = [], [], []
    for axis, f in ((0, [7.0, 10.3, 3.7]), (1, [4.6, 13.0, 2.2]), (2, [9.4, 20.7, 5.0])):
        x, y, z = LC.position(f[0], f[1], f[2], 0, vox_div)
        for d in (-1e-6, 1e-6):
            p = [x, y, z]
            p[axis] += d
            xs.append(p[0]); ys.append(p[1]); zs.append(p[2])
    r = LC.records(np.array(xs), np.array(ys), np.array(zs), np.zeros(6, dtype=np.int32), 5)
    r["n_photons"] = 1e5
    own = np.asarray(consts.light.OP_CHANNEL_TO_TPC) == 0
    lib.context()
    try:
        near, _, nvox = _stage(r, lut, 96)
        lib.set_option("light_lut_interp", 1)
        tri, _, tvox = _stage(r, lut, 96)
    finally:
        lib.set_option("light_lut_interp", 0)
    onph, _, ovox = O.light_incidence(r, lut)
    assert np.array_equal(near, onph) and np.array_equal(nvox, ovox) and np.array_equal(tvox, ovox)
    for k, axis in enumerate((0, 1, 2)):
        a, c = 2 * k, 2 * k + 1
        assert abs(int(nvox[a, axis]) - int(nvox[c, axis])) == 1              # the pair straddles the face
        rel = lambda u, v: np.abs(u[own].astype(np.float64) - v[own]) / np.maximum(u[own], v[own])       # noqa: E731
        step, smooth = rel(near[a], near[c]).max(), rel(tri[a], tri[c]).max()
        print(f"axis {axis}: nearest step {step:.3e}, trilinear {smooth:.3e}")
        assert step > 1e-3
        assert smooth < 1e-4


def test_off_means_off():
    """The option at 0, at 1 and at 0 again: the first and third results are byte-identical and equal the oracle's."""
    H.load_cfg("module0")
    lut = _lut("quad_3x4x2")
    r = LC.mixed_segments(70, (3, 4, 2), seed=91)
    n_out = consts.light.N_OP_CHANNEL
    runs = []
    lib.context()
    try:
        for v in (0, 1, 0):
            lib.set_option("light_lut_interp", v)
            runs.append(_stage(r, lut, n_out) + _resident(r, lut, n_out))
    finally:
        lib.set_option("light_lut_interp", 0)
    for a, b in zip(runs[0], runs[2]):
        assert a.tobytes() == b.tobytes()
    assert any(a.tobytes() != b.tobytes() for a, b in zip(runs[0], runs[1]))
    onph, ot0, ovox = O.light_incidence(r, lut)
    inside = r["pixel_plane"] != consts.detector.DEFAULT_PLANE_INDEX
    for nph, t0d, vox in (runs[0][:3], runs[0][3:]):
        assert np.array_equal(nph[inside], onph[inside]) and np.array_equal(t0d[inside], ot0[inside])
        assert np.array_equal(vox[inside], ovox[inside]) and (nph[~inside] == 0).all()


def test_downstream_stages_take_the_interpolated_incidence():
    """module0 resident leg with the option on: light_incidence -> light_nticks -> sum_light equals light_sim.sum_light_signals
    fed with the twin's incidence arrays and the same visiting order, to the tolerance test_resident_light_leg_golden holds the
    resident sum to against its oracle (photons rtol 3e-6, truth ids exact, truth photons rtol 1e-5): the stages after the incidence
    are untouched."""
    H.load_cfg("module0")
    g = H.gold("light_module0.npz")
    r = H.quench_drift(O, g["segments_in"])
    n = len(r)
    lut = LC.small_lut((14, 26, 8), 48, 600, n_prof=int(g["n_prof"]))
    opc = g["op_channel"]
    Mt = g["true_id"].shape[-1]
    nph, t0d, tvox = lightLUT.interpolated_light_incidence(r, lut)
    twin = np.zeros((n, consts.light.N_OP_CHANNEL), dtype=INC_DTYPE)
    twin['n_photons_det'], twin['t0_det'] = nph, t0d
    lib.context()
    try:
        lib.set_option("light_lut_interp", 1)
        ch = ChargeChain()
        ch.upload(r, np.zeros(n, dtype=np.int32))
        ch.light_incidence(lut)
        nt_dev, ts_dev = ch.light_nticks(0, n)
        n_ticks, t_start = ch.sum_light(0, n, opc, np.arange(n, dtype='i8'), max_truth=Mt, max_ticks=int(g["n_ticks"]))
        out, tid, tph = ch.download_light()
    finally:
        lib.set_option("light_lut_interp", 0)
    nt_twin, ts_twin = light_sim.get_nticks(twin)
    assert nt_dev == nt_twin and float(ts_dev) == pytest.approx(float(ts_twin), rel=1e-6)
    assert n_ticks == min(nt_twin, int(g["n_ticks"])) and float(t_start) == pytest.approx(float(ts_twin), rel=1e-6)
    order = np.ascontiguousarray(np.stack([np.argsort(nph[:, c], kind="stable")[::-1] for c in opc]), dtype=np.int32)
    out2 = np.zeros_like(out); tid2 = np.full_like(tid, -1); tph2 = np.zeros_like(tph)
    light_sim.sum_light_signals[1, 64](r, tvox, np.arange(n, dtype='i8'), twin, opc, lut, float(t_start), out2, tid2, tph2, order,
                                       int(g["n_prof"]))
    assert out2.sum() > 0
    np.testing.assert_allclose(out, out2, rtol=3e-6, atol=0)
    assert np.array_equal(tid, tid2)
    np.testing.assert_allclose(tph, tph2, rtol=1e-5)


def test_option_values_other_than_0_and_1_are_refused():
    lib.context()
    try:
        for bad in (2, -1, 0.5):
            with pytest.raises(lib.LdsimError, match="light_lut_interp must be 0 or 1"):
                lib.set_option("light_lut_interp", bad)
        lib.set_option("light_lut_interp", 1)
        lib.set_option("light_lut_interp", 0)
    finally:
        lib.set_option("light_lut_interp", 0)


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "sp_cli_light_interp_gpu", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "larnd-sim_amd", "cli",
                                                "simulate_pixels.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _same(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and all(
        np.ascontiguousarray(x if f is None else x[f]).tobytes() == np.ascontiguousarray(y if f is None else y[f]).tobytes()
        for f in (x.dtype.names or [None]))


def test_driver_flag(tmp_path, capsys):
    """simulate_pixels.py --light_lut_interpolation on a small synthetic input (.npz stream: the interpreter of the GPU tests has
    no h5py): trilinear and nearest give identical charge datasets and different light datasets; nearest is the file of a run
    without the flag, dataset for dataset; the choice is in the run's header; the context option is back at 0 afterwards."""
    from larndsim_amd import synth
    cli = _cli()
    H.load_cfg("module0")
    seg = synth.make_segments(120, seed=23, segs_per_event=40)
    np.save(tmp_path / "in.npy", seg)
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    np.savez(tmp_path / "lut.npz", arr=LC.small_lut((14, 26, 8), 48, 24, n_prof=20))
    common = dict(input_filename=str(tmp_path / "in.npy"), config="module0", rand_seed=7, rng="keyed", light_simulated=True,
                  response_file=str(tmp_path / "resp.npy"), light_lut_filename=str(tmp_path / "lut.npz"))

    def run(name, **kw):
        cli.run_simulation(output_filename=str(tmp_path / name), **common, **kw)
        with np.load(tmp_path / name) as f:
            return {k: f[k] for k in f.files}, capsys.readouterr().out

    try:
        plain, log0 = run("plain.npz")
        near, log1 = run("near.npz", light_lut_interpolation="nearest")
        tri, log2 = run("tri.npz", light_lut_interpolation="trilinear")
        with pytest.raises(ValueError, match="light_lut_interpolation"):
            run("bad.npz", light_lut_interpolation="cubic")
    finally:
        H.load_cfg("module0")
    assert "Light LUT interpolation: nearest" in log0 and "Light LUT interpolation: nearest" in log1
    assert "Light LUT interpolation: trilinear (--light_lut_interpolation trilinear)" in log2
    assert set(plain) == set(near) == set(tri)
    light = {k for k in plain if k.startswith("light")}
    dat = [k for k in light if k.startswith("light_dat")]            # (the .npz stream spells the group's "/" as "__")
    assert len(dat) == 1 and "light_wvfm" in light
    def charge(d):
        """the charge read-out: data packets with their truth rows (trigger packets in the stream follow the light)"""
        m = d["packets"]["packet_type"] == 0
        return d["packets"][m], d["mc_packets_assn"][m]

    for k in plain:
        assert _same(plain[k], near[k]), k
        if k not in light and k not in ("packets", "mc_packets_assn"):
            assert _same(plain[k], tri[k]), k
    for x, y in zip(charge(near), charge(tri)):
        assert len(x) > 100 and _same(x, y)
    assert not _same(near[dat[0]], tri[dat[0]]) and not _same(near["light_wvfm"], tri["light_wvfm"])
    # the driver left the process-wide context as it found it
    r = LC.mixed_segments(33, (3, 4, 2), seed=5)
    onph, _, _ = O.light_incidence(r, _lut("quad_3x4x2"))
    assert np.array_equal(_stage(r, _lut("quad_3x4x2"), consts.light.N_OP_CHANNEL)[0], onph)


def test_driver_flag_hdf5_files(tmp_path):
    """The same through real HDF5 files (tests/light_interp_h5_driver.py, a fresh process of an interpreter with h5py): identical
    charge datasets, different light datasets, `nearest` the file of a run without the flag."""
    exe = h5_python()
    if exe is None:
        pytest.skip("no interpreter with h5py in this environment")
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "PYTHONHOME")}
    r = subprocess.run([exe, os.path.join(os.path.dirname(os.path.abspath(__file__)), "light_interp_h5_driver.py"), str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("LIGHT_INTERP_H5 ")][0][16:])
    assert res["n_data_packets"] > 100 and "light_wvfm" in res["differ"] and "packets" in res["datasets"]
