"""GPU: the field-response builder (csrc/kernels_respbuild.hip: response_build_kernel) against the long-double numpy twin
(larndsim_amd/response_builder.py twin), its exact properties, charge conservation on the full module0 shape, and the built
table through tracks_current and the driver.

Bounds.  Per entry, absolute: four times the largest difference between the f64 numpy twin and the long-double twin of the same
case -- a measurement of f64 rounding against a more precise reference; the factor 4 covers the device's atan2 / sqrt being a
few ulp off libm.  Nothing here is taken from the kernel's output.  The closure of a row telescopes over K + 1 edges: (K + 1) dt
times the per-entry bound.  Through the chain: helpers.assert_wave_close at its defaults against the oracle with the same table,
the per-segment charge at rtol 1e-5, and the ratio to a collection-only table as in tests/test_cpu_response_builder.py.
Shapes: (7, 5, 300) with arrival tick 280 -- I != J, 301 edges (ragged over waves, two passes of a 256-lane workgroup), trailing
zero ticks; (3, 2, 3800) at 0.05 us for the long row; (45, 45, 1950) once, shared."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from larndsim_amd import abi, batching, consts, detsim, lib, response_builder as RB, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "larnd-sim_amd", "cli", "build_response.py")
F4_TOL = 1e-5                  # the project's tolerance for f4-stored currents

CASES = {"main": dict(shape=(7, 5, 300), arrival_tick=280, n_sub=3),
         "n_sub_1": dict(shape=(7, 5, 300), arrival_tick=280, n_sub=1),
         "pad_0p8": dict(shape=(7, 5, 300), arrival_tick=280, n_sub=3, pad_frac=0.8),
         "long_row": dict(shape=(3, 2, 3800), n_sub=3, sampling=0.05)}


def _params(shape, n_sub, arrival_tick=None, pad_frac=1.0, sampling=None):
    H.load_cfg("module0")
    return RB.params(pad_size=pad_frac * consts.detector.PIXEL_PITCH, n_sub=n_sub, shape=shape, arrival_tick=arrival_tick,
                     sampling=sampling)


@functools.lru_cache(maxsize=None)
def _built(name):
    p = _params(**CASES[name])
    t = RB.build(p)
    t.setflags(write=False)
    return p, t


def _entry_tolerance(p):
    """4 x max |f64 twin - long-double twin|, and the long-double twin"""
    ld = RB.twin(p, np.longdouble)
    return 4 * float(np.abs(RB.twin(p) - ld).max()), ld


@pytest.mark.parametrize("name", list(CASES))
def test_table_against_the_long_double_twin(name):
    p, got = _built(name)
    tol, ld = _entry_tolerance(p)
    assert got.shape == ld.shape and got.dtype == np.float64
    worst = float(np.abs(got - ld).max())
    print(f"{name}: worst |kernel - long-double twin| {worst:.3e}, bound {tol:.3e}, peak entry {np.abs(ld).max():.4f}")
    assert 0 < tol < 2e-12 and np.abs(ld).max() > 0.5
    assert worst <= tol
    assert (got[:, :, p["arrival_tick"] + 1:] == 0).all() and (got[:, :, p["arrival_tick"]] != 0).all()


def test_exact_properties():
    p, main = _built("main")
    assert main[:, :, 281:].size == 7 * 5 * 19 and (main[:, :, 281:] == 0).all()              # after the arrival: exactly 0
    assert RB.build(p).tobytes() == main.tobytes()                                             # two builds, the same bytes
    corner = RB.build(_params((4, 3, 300), 3, 280))
    assert corner.tobytes() == np.ascontiguousarray(main[:4, :3]).tobytes()                    # a row does not know the grid
    long_k = RB.build(_params((7, 5, 300), 3, 150))
    short_k = RB.build(_params((7, 5, 200), 3, 150))
    assert short_k.tobytes() == np.ascontiguousarray(long_k[:, :, :200]).tobytes()             # nor the table's length
    assert (long_k[:, :, 151:] == 0).all() and not np.array_equal(long_k[:, :, :151], main[:, :, :151])


@functools.lru_cache(maxsize=None)
def _module0_table():
    H.load_cfg("module0")
    p = RB.params(n_sub=2)
    t = RB.build(p)
    ms = RB.build_ms()
    t.setflags(write=False)
    return p, t, ms


def test_full_module0_shape():
    p, R, ms = _module0_table()
    assert R.shape == (45, 45, 1950) and ms > 0
    # the per-entry bound of the same parameters from the (7, 7) rows around the pad: the long-double twin of the whole shape
    # takes 6 s, and the largest difference over a part of the rows can only be smaller than over all of them, never larger
    tol = _entry_tolerance(dict(p, n_i=7, n_j=7))[0]
    dt, K = p["sampling"], p["n_k"]
    z_top = RB.edge_heights(p)[0]
    ends = RB.mean_potential(p, [0.0, z_top], np.longdouble)
    expect = (ends[:, :, 0] - ends[:, :, 1]).astype(np.float64)
    closure = R.sum(axis=-1) * dt
    worst = float(np.abs(closure - expect).max())
    print(f"build {ms:.3f} ms; closure over the pad {closure[:5, :5].min():.8f} .. {closure[:5, :5].max():.8f}, elsewhere "
          f"{closure[5:].min():.3e} .. {closure[5:].max():.3e}; worst |closure - telescoped| {worst:.3e}, bound {(K + 1) * dt * tol:.3e}; "
          f"worst |R[i, j] - R[j, i]| {np.abs(R - R.transpose(1, 0, 2)).max():.3e}, bound {tol:.3e}")
    assert worst <= (K + 1) * dt * tol
    top = float(RB.weighting_potential(0.0, 0.0, z_top, p["pad_size"]))
    assert np.abs(closure[:5, :5] - (1 - top)).max() < 1e-6 and np.abs(closure[5:] + top).max() < 1e-6
    assert np.abs(closure[:, 5:] + top).max() < 1e-6
    assert np.abs(R - R.transpose(1, 0, 2)).max() <= tol
    assert (R[:, :, 1891:] == 0).all() and 3.5 < R.max() < 4.5         # (the numpy twin's peak: 3.90 at n_sub 2, 4.03 at 4)


def _segments():
    H.load_cfg("module0")
    seg = synth.make_segments(12, seed=5, segs_per_event=12)
    batching.swap_coordinates(seg)
    r = H.quench_drift(O, seg)
    nmax = O.max_pixels(r)
    assert H.oracle_radius(seg) == 1
    _, neigh, _, _ = O.get_pixels(r, nmax, 3 * nmax + 6, 1)
    _, T = O.time_intervals(r)
    return r, np.ascontiguousarray(neigh), T


def _tracks_current(neigh, r, resp, T):
    lib.context()
    sig = np.zeros(neigh.shape + (T,), dtype=np.float32)
    detsim.tracks_current[(1, 1, 1), (1, 1, 64)](sig, neigh, r, np.ascontiguousarray(resp))
    return sig


def test_built_table_through_tracks_current():
    p, table, _ = _module0_table()
    r, neigh, T = _segments()
    det = consts.detector
    ref = O.tracks_current(r, neigh, T, table)
    sig = _tracks_current(neigh, r, table, T)
    coll = _tracks_current(neigh, r, RB.collection_only(p), T)
    q_ref = ref.astype(np.float64).sum(axis=(1, 2)) * det.TIME_SAMPLING
    q_sig = sig.astype(np.float64).sum(axis=(1, 2)) * det.TIME_SAMPLING
    q_coll = coll.astype(np.float64).sum(axis=(1, 2)) * det.TIME_SAMPLING
    z_anode = np.asarray(det.TPC_BORDERS)[r["pixel_plane"], 2, 0]
    z_min = float(np.abs(r["z"] - z_anode).min())
    n_listed = int((neigh >= 0).sum(axis=1).max())
    bound = n_listed * p["pad_size"] ** 2 / (2 * np.pi * z_min ** 2)
    ratio = q_sig / q_coll
    err = np.abs(sig.astype(np.float64) - ref)
    i = np.unravel_index(np.argmax(err), err.shape)
    print(f"worst sample at {i}: got {sig[i]!r} ref {ref[i]!r}, waveform peak {np.abs(ref[i[:2]]).max()!r}; charge per segment "
          f"against the oracle: max rel {np.abs(q_sig / q_ref - 1).max():.3e}; P {n_listed}, z_min {z_min:.2f} cm, ratio "
          f"{ratio.min():.6f} .. {ratio.max():.6f}, 1 - ratio <= {bound + F4_TOL:.3e}")
    assert (ref != 0).sum() > 10000 and ((ref < 0).any(axis=-1) & (ref > 0).any(axis=-1)).any()    # bipolar waveforms went in
    np.testing.assert_allclose(q_sig, q_ref, rtol=1e-5)
    assert (q_coll > 0).all()
    assert (1 - ratio >= -F4_TOL).all() and (1 - ratio <= bound + F4_TOL).all()
    H.assert_wave_close(sig, ref, what="tracks_current with the built table")


def test_tool_file_through_the_driver(tmp_path, capsys):
    """build_response.py writes the table a direct build gives; simulate_pixels.py --response_file takes it and writes hits"""
    H.load_cfg("module0")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONHOME"}
    out = tmp_path / "response.npy"
    r = subprocess.run([sys.executable, TOOL, "--config", "module0", "--n_sub", "1", "--output", str(out)], capture_output=True,
                       text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ms on the GPU" in r.stdout and "(45, 45, 1950) table" in r.stdout
    table = np.load(out)
    assert table.dtype == np.float64 and table.tobytes() == RB.build(RB.params(n_sub=1)).tobytes()
    spec = importlib.util.spec_from_file_location("sp_cli_response_builder", os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    np.save(tmp_path / "in.npy", synth.make_segments(60, seed=10, segs_per_event=30))
    try:
        cli.run_simulation(str(tmp_path / "in.npy"), str(tmp_path / "out.npz"), config="module0", rand_seed=1,
                           response_file=str(out), light_simulated=False)
    finally:
        H.load_cfg("module0")
    capsys.readouterr()
    with np.load(tmp_path / "out.npz") as f:
        n_hits = int((f["packets"]["packet_type"] == 0).sum())
    print(f"{n_hits} data packets")
    assert n_hits > 0


def _raw_build(ctx, table=True, **kw):
    """ldsim_response_build straight through ctypes (the Python layer refuses these itself): (status, message)"""
    d = dict(pad_size=0.4434, bin_size=0.04434, v_drift=0.16, sampling=0.1, n_i=2, n_j=2, n_k=20, n_sub=2, arrival_tick=10)
    d.update(kw)
    P = abi.LdsimResponseBuildParams(**d)
    out = np.zeros((max(d["n_i"], 1), max(d["n_j"], 1), max(min(d["n_k"], 8000), 1)))
    rc = lib.load().ldsim_response_build(ctx, C.byref(P), lib.ptr(out) if table else None)
    return rc, lib.load().ldsim_last_error().decode()


def test_library_refusals():
    ctx = lib.context()
    assert _raw_build(ctx)[0] == 0
    for kw, msg in ((dict(pad_size=0.0), "pad_size"), (dict(bin_size=-1.0), "bin_size"), (dict(v_drift=float("nan")), "v_drift"),
                    (dict(sampling=0.0), "sampling"), (dict(n_i=0), "zero-sized table"), (dict(n_k=0, arrival_tick=0), "zero-sized table"),
                    (dict(n_k=7680), "n_k 7680"), (dict(n_sub=0), "n_sub 0"), (dict(n_sub=17), "n_sub 17"),
                    (dict(arrival_tick=20), "arrival_tick 20"), (dict(arrival_tick=-1), "arrival_tick -1")):
        rc, text = _raw_build(ctx, **kw)
        assert rc != 0 and "ldsim_response_build" in text and msg in text, (kw, rc, text)
    rc, text = _raw_build(ctx, table=False)
    assert rc != 0 and "null argument" in text
    assert _raw_build(ctx, n_k=7679, n_i=1, n_j=1)[0] == 0                 # the longest row the kernel takes
