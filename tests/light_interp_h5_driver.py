"""
simulate_pixels.py --light_lut_interpolation through real HDF5 files.  Started by tests/test_gpu_light_interp.py as a subprocess
of an interpreter that has h5py (the one the GPU tests run on may have none), on the GPU:

  python tests/light_interp_h5_driver.py <work dir>

A small synthetic input (HDF5 `segments`) is simulated without the flag, with `nearest` and with `trilinear`; the three files
are compared dataset for dataset here, and a one-line JSON summary goes to stdout for the test to read.
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, REPO, os.path.join(REPO, "larnd-sim_amd")):
    sys.path.insert(0, p)

from h5_layout import read_all                       # noqa: E402
from larndsim_amd import consts, synth               # noqa: E402


def same(x, y):
    """equal field by field (padding bytes of an aligned record are not data)"""
    return x.shape == y.shape and x.dtype == y.dtype and all(
        np.ascontiguousarray(x if f is None else x[f]).tobytes() == np.ascontiguousarray(y if f is None else y[f]).tobytes()
        for f in (x.dtype.names or [None]))


def main(work):
    import h5py
    spec = importlib.util.spec_from_file_location("sp_cli_light_interp_h5", os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    consts.load_snapshot("module0")
    seg = synth.make_segments(120, seed=23, segs_per_event=40)
    inp = os.path.join(work, "in.h5")
    with h5py.File(inp, "w") as f:
        f.create_dataset("segments", data=seg)
    np.save(os.path.join(work, "resp.npy"), synth.make_response("survey"))
    np.savez(os.path.join(work, "lut.npz"), arr=synth.make_lut((14, 26, 8), 48, 20, 24))
    common = dict(input_filename=inp, config="module0", rand_seed=7, rng="keyed", light_simulated=True,
                  response_file=os.path.join(work, "resp.npy"), light_lut_filename=os.path.join(work, "lut.npz"))
    files = {}
    for name, kw in (("plain", {}), ("nearest", dict(light_lut_interpolation="nearest")),
                     ("trilinear", dict(light_lut_interpolation="trilinear"))):
        out = os.path.join(work, name + ".h5")
        cli.run_simulation(output_filename=out, **common, **kw)
        files[name] = read_all(out)
    plain, near, tri = files["plain"], files["nearest"], files["trilinear"]
    assert set(plain) == set(near) == set(tri), (sorted(plain), sorted(tri))
    light = sorted(k for k in plain if k.startswith("light"))
    assert "light_dat/light_dat_allmodules" in light and "light_wvfm" in light, light
    for k in plain:                                  # `nearest` is the run without the flag, dataset for dataset
        assert same(plain[k], near[k]), k

    def charge(d):
        """the charge read-out: data packets with their truth rows (trigger packets in the stream follow the light)"""
        m = d["packets"]["packet_type"] == 0
        return d["packets"][m], d["mc_packets_assn"][m]

    for k in plain:
        if k not in light and k not in ("packets", "mc_packets_assn"):
            assert same(near[k], tri[k]), k
    n_data = 0
    for x, y in zip(charge(near), charge(tri)):
        assert same(x, y)
        n_data = len(x)
    differ = [k for k in light if not same(near[k], tri[k])]
    assert "light_dat/light_dat_allmodules" in differ and "light_wvfm" in differ, differ
    print("LIGHT_INTERP_H5 " + json.dumps(dict(datasets=sorted(plain), light=light, differ=differ, n_data_packets=int(n_data))))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
