"""CPU: the drift-field map loader (larndsim_amd/field_map.py) and the CLI's --field_map on the self-launch path."""
import os
import subprocess
import sys

import numpy as np
import pytest

from larndsim_amd import field_map

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")


def _good(shape=(3, 4, 5)):
    rs = np.random.default_rng(1)
    return {"origin": [0.0, -1.0, 2.0], "spacing": [1.0, 0.5, 2.0], "E": 0.5 + rs.random(shape),
            "dx": rs.normal(size=shape), "dz": np.zeros(shape)}


def test_load_round_trip(tmp_path):
    maps = {0: _good(), 3: {"origin": [0, 0, 0], "spacing": [1, 1, 1], "dy": np.ones((2, 2, 2))}}
    field_map.save(tmp_path / "m.npz", maps)
    got = field_map.load(tmp_path / "m.npz", n_tpc=4)
    assert sorted(got) == [0, 3] and sorted(got[3]) == ["dy", "origin", "spacing"]
    for t in maps:
        for k, v in maps[t].items():
            assert got[t][k].dtype == np.float64 and got[t][k].flags["C_CONTIGUOUS"]
            np.testing.assert_array_equal(got[t][k], np.asarray(v, dtype=np.float64))


@pytest.mark.parametrize("change, msg", [
    (lambda m: m.pop("origin"), "no origin"),
    (lambda m: m.pop("spacing"), "no spacing"),
    (lambda m: m.update(origin=[0.0, 1.0]), "origin must be 3"),
    (lambda m: m.update(spacing=[[1.0, 1.0, 1.0]]), "spacing must be 3"),
    (lambda m: m.update(E=np.ones((3, 4))), "every dimension"),
    (lambda m: m.update(E=np.ones((3, 1, 5))), "every dimension"),
    (lambda m: m.update(dx=np.ones((3, 4, 6))), "another channel"),
    (lambda m: m.update(E=np.where(np.arange(60).reshape(3, 4, 5) == 7, 0.0, 1.0)), "E must be > 0"),
    (lambda m: m.update(E=-np.ones((3, 4, 5))), "E must be > 0"),
    (lambda m: m["dx"].__setitem__((1, 2, 3), np.nan), "non-finite"),
    (lambda m: m["E"].__setitem__((0, 0, 0), np.nan), "non-finite"),
    (lambda m: m.update(origin=[0.0, np.inf, 0.0]), "finite"),
    (lambda m: m.update(spacing=[1.0, 0.0, 1.0]), "spacing must be > 0"),
    (lambda m: m.update(spacing=[1.0, 1.0, -2.0]), "spacing must be > 0"),
    (lambda m: m.update(spacing=[1.0, np.nan, 1.0]), "finite"),
    (lambda m: [m.pop(k) for k in ("E", "dx", "dz")], "none of the channels"),
])
def test_load_rejects(tmp_path, change, msg):
    m = _good()
    change(m)
    field_map.save(tmp_path / "bad.npz", {1: m})
    with pytest.raises(ValueError, match=msg):
        field_map.load(tmp_path / "bad.npz", n_tpc=2)


@pytest.mark.parametrize("tpc", [2, 7])
def test_load_rejects_tpc_out_of_range(tmp_path, tpc):
    field_map.save(tmp_path / "m.npz", {tpc: _good()})
    with pytest.raises(ValueError, match=f"TPC {tpc} outside"):
        field_map.load(tmp_path / "m.npz", n_tpc=2)


def test_load_rejects_unknown_key(tmp_path):
    np.savez(tmp_path / "m.npz", tpc0_origin=np.zeros(3), tpc0_spacing=np.ones(3), tpc0_E=np.ones((2, 2, 2)),
             tpc0_Ex=np.ones((2, 2, 2)))
    with pytest.raises(ValueError, match="unexpected key"):
        field_map.load(tmp_path / "m.npz", n_tpc=1)


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_cli_field_map_reaches_every_rank(tmp_path):
    """`--n_gpus 2 --field_map PATH` without a launcher: both self-launched ranks get the flag (LDSIM_CLI_REHEARSAL stops them
    before any GPU call)."""
    path = str(tmp_path / "map.npz")
    args = ["--input_filename", str(tmp_path / "in.npy"), "--output_filename", str(tmp_path / "out.npz"), "--n_gpus", "2",
            "--field_map", path]
    r = subprocess.run([sys.executable, CLI] + args, env=_env(LDSIM_CLI_REHEARSAL="1"), capture_output=True, timeout=180)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = sorted(ln for ln in r.stdout.decode().splitlines() if " field_map " in ln)
    assert got == [f"rehearsal: rank 0 field_map {path}", f"rehearsal: rank 1 field_map {path}"]
