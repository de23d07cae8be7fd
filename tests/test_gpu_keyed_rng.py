"""GPU: keyed random streams (ChargeChain.seed_keyed, simulate_pixels.py --rng keyed).  The device generator against its numpy
restatement, the inline FEE draws against materialised ones, keyed against table statistics, and the CLI's files at another
chunking, rank count or event subset.  Every GPU run is a fresh process with a time limit of its own; nothing is retried."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from larndsim_amd import lib, rng
from test_cpu_keyed_rng import keyed_normals, keyed_uniforms
from test_gpu_multirank import _LOOPBACK, _assert_same, _inputs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "larnd-sim_amd")
CLI = os.path.join(PKG, "cli", "simulate_pixels.py")
TESTS = os.path.dirname(os.path.abspath(__file__))
HEAD = f"import sys\nsys.path[:0] = [{PKG!r}, {TESTS!r}]\n"


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _run(cmd, timeout, **env):
    r = subprocess.run(cmd, env=_env(**env), capture_output=True, timeout=timeout)
    assert r.returncode == 0, (cmd, r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    return r


def _script(tmp_path, name, body, timeout=300):
    p = tmp_path / name
    p.write_text(HEAD + body)
    return _run([sys.executable, str(p)], timeout)


_DRAWS = r'''
import numpy as np
from larndsim_amd import lib, rng
from larndsim_amd.chain import ChargeChain
ch = ChargeChain()
ch.seed_keyed(0x0123456789ABCDEF)
keys = np.random.default_rng(1).integers(0, 2 ** 63, 1000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
u = rng.keyed_draws(keys, 1000, first=13, tag=rng.TAG_LIGHT_FLUCT, normal=False)
z = rng.keyed_draws(keys[:100], 1000, first=7, tag=rng.TAG_FEE)
big = rng.keyed_draws(keys[:10], 1000000, tag=rng.TAG_MC)
np.savez({out!r}, keys=keys, u=u, z=z, mean=big.astype(np.float64).mean(), var=big.astype(np.float64).var(), n=big.size)
ch.seed_rng(1)
try:
    rng.keyed_draws(keys[:1], 4)
    raise SystemExit("keyed draws accepted in table mode")
except lib.LdsimError as e:
    assert "keyed mode" in str(e), str(e)
print("draws ok")
'''


def test_keyed_draws_equal_numpy_restatement(tmp_path):
    """10^6 uniforms bit-identical to the numpy restatement (mixed keys, offset 13); 10^5 normals within 4 ulp of the pair's
    radius; 10^7 normals with mean and variance within 5 standard errors of 0 and 1"""
    out = tmp_path / "draws.npz"
    _script(tmp_path, "draws.py", _DRAWS.format(out=str(out)))
    d = np.load(out)
    seed, keys = 0x0123456789ABCDEF, d["keys"]
    want_u = keyed_uniforms(seed, rng.TAG_LIGHT_FLUCT, keys[:, None], np.arange(13, 1013)[None, :])
    assert d["u"].shape == (1000, 1000) and np.array_equal(d["u"], want_u)
    want_z, r = keyed_normals(seed, rng.TAG_FEE, keys[:100, None], np.arange(7, 1007)[None, :])
    err = np.abs(d["z"].astype(np.float64) - want_z)
    assert (err <= 4 * np.spacing(r.astype(np.float32)).astype(np.float64)).all(), err.max()
    n = int(d["n"])
    assert n == 10 ** 7
    assert abs(float(d["mean"])) < 5 / np.sqrt(n)
    assert abs(float(d["var"]) - 1) < 5 * np.sqrt(2.0 / n)


_INLINE = r'''
import numpy as np
import helpers as H
from larndsim_amd import batching, consts, lib, synth
from larndsim_amd.chain import ChargeChain
cfg = {cfg!r}
H.load_cfg(cfg, noise_zero=False)
seg = synth.make_segments(600, seed=5, segs_per_event=60)
batching.swap_coordinates(seg)
bid, order, table = batching.assign_batches(seg)
seg, bid = seg[order], bid[order]
ch = ChargeChain(synth.make_response("survey"))
ch.upload(seg, bid)
ch.quench_drift()
if {tables!r}:
    keys = np.arange(0, 2 ** 20, 7, dtype=np.int32)
    thr = consts.detector.DISCRIMINATION_THRESHOLD * (0.8 + 0.4 * np.random.default_rng(3).random(len(keys)))
    ch.set_pixel_thresholds(keys, thr, consts.detector.DISCRIMINATION_THRESHOLD)
ch.seed_keyed(11)
try:
    ch.run(0, len(seg), want_fractions=True)
    raise SystemExit("a keyed launch without batch keys ran")
except lib.LdsimError as e:
    assert "no key for batch id" in str(e), str(e)
ch.set_batch_keys(table, 1)
res = []
for mat in (0, 1):
    lib.set_option("debug_rng_materialize", mat)
    ch.run(0, len(seg), want_fractions=True)
    res.append(ch.download(fractions=True))
lib.set_option("debug_rng_materialize", 0)
a, b = res
assert (a["adc_list"] != 0).sum() > 200, (a["adc_list"] != 0).sum()
for k in a:
    assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
print("inline ok", cfg, int((a["adc_list"] != 0).sum()))
'''


@pytest.mark.parametrize("cfg,tables", [("module0", False), ("2x2_no_modvar", True)])
def test_inline_keyed_noise_equals_materialised(tmp_path, cfg, tables):
    """the chain with FEE noise on, keyed, draws inline in the scan; with debug_rng_materialize the same keyed normals are
    written to the table layout and read by the table scan that the oracle pins: ADC values, ticks, codes, track map and
    fractions are bit-identical.  A keyed launch without batch keys is refused."""
    r = _script(tmp_path, "inline.py", _INLINE.format(cfg=cfg, tables=tables))
    assert b"inline ok" in r.stdout


_CLOSURE = r'''
import numpy as np
import helpers as H
from larndsim_amd import batching, consts, synth
from larndsim_amd.chain import ChargeChain
H.load_cfg("module0", noise_zero=False)
consts.detector.DISCRIMINATION_THRESHOLD = 2.0 * consts.detector.UNCORRELATED_NOISE_CHARGE    # noise-dominated
seg = synth.make_segments(1500, seed=8, segs_per_event=300)
batching.swap_coordinates(seg)
bid, order, table = batching.assign_batches(seg)
seg, bid = seg[order], bid[order]
ch = ChargeChain(synth.make_response("survey"))
ch.upload(seg, bid)
ch.quench_drift()
out = {{}}
for mode in ("table", "keyed"):
    if mode == "table":
        ch.seed_rng(3)
    else:
        ch.seed_keyed(3)
        ch.set_batch_keys(table, 1)
    ch.run(0, len(seg))
    d = ch.download()
    hit = d["adc_list"] != 0
    out[mode] = dict(nhit=hit.sum(axis=1), codes=d["adc_digit"][hit], U=len(d["unique_pix"]))
np.savez({path!r}, **{{f"{{m}}_{{k}}": v for m, d in out.items() for k, v in d.items()}})
'''


def test_keyed_statistics_match_table_mode(tmp_path):
    """a different stream, not different physics: on a noise-dominated input (threshold at twice the uncorrelated noise,
    more than 2000 pixels) hits per pixel and the ADC code mean and variance agree within 5 standard errors"""
    path = tmp_path / "closure.npz"
    _script(tmp_path, "closure.py", _CLOSURE.format(path=str(path)))
    d = np.load(path)
    assert int(d["table_U"]) == int(d["keyed_U"]) > 2000
    for k in ("nhit", "codes"):
        a, b = d[f"table_{k}"].astype(np.float64), d[f"keyed_{k}"].astype(np.float64)
        assert len(a) > 2000 and len(b) > 2000, k
        se = np.sqrt(a.var() / len(a) + b.var() / len(b))
        assert abs(a.mean() - b.mean()) < 5 * se, (k, a.mean(), b.mean(), se)
        va, vb = a.var(), b.var()
        se_v = np.sqrt(np.mean((a - a.mean()) ** 4) / len(a) + np.mean((b - b.mean()) ** 4) / len(b))
        assert abs(va - vb) < 5 * se_v, (k, va, vb, se_v)


def _cli(tmp_path, args, name, timeout=600):
    out = tmp_path / name
    _run([sys.executable, CLI] + args + ["--output_filename", str(out)], timeout)
    return dict(np.load(out))


def test_keyed_files_do_not_depend_on_chunking(tmp_path):
    """--rng keyed, FEE noise at the reference defaults, light leg on: --chunk_segments 40 and 100000 write the same file,
    every dataset; again with --tracks_current_mc.  Control: table mode with the noise constants 0 is already equal, so
    nothing but the random streams follows the launch boundaries."""
    args = _inputs(tmp_path)
    noiseless = tmp_path / "noiseless.py"
    noiseless.write_text(_LOOPBACK.split("import json")[0].format(pkg=PKG, cli=CLI) + "cli.main(sys.argv[1:])\n")
    a = dict(np.load(_run_noiseless(tmp_path, noiseless, args + ["--chunk_segments", "40"], "c40.npz")))
    b = dict(np.load(_run_noiseless(tmp_path, noiseless, args + ["--chunk_segments", "100000"], "c1e5.npz")))
    _assert_same(a, b)
    for extra in ([], ["--tracks_current_mc"]):
        tag = "mc" if extra else "tc"
        a = _cli(tmp_path, args + extra + ["--rng", "keyed", "--chunk_segments", "40"], f"k40{tag}.npz")
        b = _cli(tmp_path, args + extra + ["--rng", "keyed", "--chunk_segments", "100000"], f"k1e5{tag}.npz")
        assert len(a["packets"]) > 100 and len(a["light_wvfm"]) >= 2
        _assert_same(a, b)


def _run_noiseless(tmp_path, script, argv, name):
    out = tmp_path / name
    _run([sys.executable, str(script)] + argv + ["--output_filename", str(out)], 600)
    return out


def test_keyed_world_2_loopback_equals_one_rank(tmp_path):
    """both ranks of a world-2 keyed run played in one process (the RCCL transfer replaced by a hand-over in memory, as in
    test_gpu_multirank), FEE noise and light on: every dataset equals the one-rank keyed file"""
    script = tmp_path / "loopback.py"
    script.write_text(_LOOPBACK.format(pkg=PKG, cli=CLI).replace(
        "consts.load_snapshot = load_snapshot\n", "consts.load_snapshot = _load\n", 1))
    argv = _inputs(tmp_path) + ["--chunk_segments", "40"]
    one = _cli(tmp_path, argv + ["--rng", "keyed"], "one.npz")
    kw = dict(input_filename=argv[1], output_filename=str(tmp_path / "two.npz"), config="module0", rand_seed=7,
              response_file=argv[7], chunk_segments=40, n_gpus=2, rng="keyed", light_lut_filename=argv[9],
              light_det_noise_filename=argv[11])
    r = _run([sys.executable, str(script), json.dumps(kw)], 600)
    tot = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("LOOPBACK ")][0][9:])
    assert tot["n_ranks"] == 2 and min(tot["rows_per_rank"]) > 50
    _assert_same(one, dict(np.load(tmp_path / "two.npz")))


def test_keyed_event_subset_rows_equal_full_run(tmp_path):
    """a keyed run on an input without its first events (the largest event id kept, so the event times are unchanged) writes,
    for the events it keeps, the data packets, their association rows and the light rows of the full run"""
    args = _inputs(tmp_path)
    full = _cli(tmp_path, args + ["--rng", "keyed"], "full.npz")
    seg = np.load(tmp_path / "in.npy")
    ev = np.unique(seg["event_id"])
    keep = ev[3:]
    np.save(tmp_path / "sub.npy", seg[np.isin(seg["event_id"], keep)])
    sub_args = list(args)
    sub_args[1] = str(tmp_path / "sub.npy")
    sub = _cli(tmp_path, sub_args + ["--rng", "keyed"], "sub.npz")

    def data_rows(d):
        p, a = d["packets"], d["mc_packets_assn"]
        return p, a, (p["packet_type"] == 0) & np.isin(a["event_ids"][:, 0], keep)
    pf, af, sel_f = data_rows(full)
    ps, as_, sel_s = data_rows(sub)
    assert sel_f.sum() > 100 and sel_f.sum() == sel_s.sum()
    for f in pf.dtype.names:
        assert np.array_equal(pf[f][sel_f], ps[f][sel_s]), f
    for f in af.dtype.names:
        if f != "segment_ids":                  # (ids of the file's own segment rows)
            assert np.array_equal(af[f][sel_f], as_[f][sel_s]), f
    # light: the kept events come last in the full run's event loop, so their rows are its tail
    n = len(sub["light_wvfm"])
    assert n >= 2 and len(full["light_wvfm"]) > n
    assert np.array_equal(full["light_wvfm"][-n:], sub["light_wvfm"])
    _assert_same({"t": full["light_trig"][-n:]}, {"t": sub["light_trig"]})
    if "light_wvfm_mc_assn" in full:           # (light truth rows: only with MAX_MC_TRUTH_IDS > 0)
        tf, ts = full["light_wvfm_mc_assn"], sub["light_wvfm_mc_assn"]
        wf = np.isin(tf["event_id"], keep)
        assert wf.sum() == len(ts) > 0
        for f in tf.dtype.names:
            if f != "trigger_id":               # (a running count from the file's first trigger)
                assert np.array_equal(tf[f][wf], ts[f]), f


def _devices():
    try:
        return lib.device_count()
    except Exception:
        return 0


@pytest.mark.skipif(_devices() < 2, reason="two ranks need two GPUs (RCCL does not put two ranks on one device)")
def test_keyed_two_ranks_equal_one_rank(tmp_path):
    """--n_gpus 2 --rng keyed equals the one-rank keyed file, every dataset, FEE noise and light on"""
    args = _inputs(tmp_path) + ["--chunk_segments", "80", "--rng", "keyed"]
    one = _cli(tmp_path, args, "one.npz")
    two = _cli(tmp_path, args + ["--n_gpus", "2"], "two.npz")
    _assert_same(one, two)


_REFUSE = r'''
import numpy as np
import helpers as H
from larndsim_amd import consts, fee, lib, light_sim, synth
from larndsim_amd.chain import ChargeChain
H.load_cfg("module0", noise_zero=False)
ch = ChargeChain(synth.make_response("survey"))
ch.seed_keyed(4)
msg = "keyed mode and this stage call carries no identity"
L = lib.load()
U, NT = 3, 100
ps = np.zeros((U, NT))
tt = np.linspace(0, 1, NT + 1)
thr = np.full(U, 1.0)
adc = np.zeros((U, consts.sim.MAX_ADC_VALUES)); ticks = np.zeros_like(adc)
import ctypes as C
rc = L.ldsim_get_adc_values(lib.context(), lib.ptr(ps), None, C.c_int64(U), C.c_int32(NT), C.c_int32(5), lib.ptr(tt),
                            C.c_int32(NT + 1), C.c_double(0.0), lib.ptr(thr), lib.ptr(adc), lib.ptr(ticks), None)
assert rc != 0 and msg in L.ldsim_last_error().decode(), L.ldsim_last_error()
inc = np.ones((2, 10), dtype=np.float32); disc = np.zeros_like(inc)
rc = L.ldsim_stat_fluctuations(lib.context(), lib.ptr(inc), C.c_int32(2), C.c_int32(10), lib.ptr(disc))
assert rc != 0 and msg in L.ldsim_last_error().decode(), L.ldsim_last_error()
seg = synth.make_segments(4, seed=1, segs_per_event=4)
from larndsim_amd.layout import make_layout
lay = make_layout(seg.dtype)
pix = np.zeros((4, 2), dtype=np.int32); sig = np.zeros((4, 2, 8), dtype=np.float32)
rc = L.ldsim_tracks_current_mc(lib.context(), lib.ptr(seg), C.c_int64(4), C.byref(lay), lib.ptr(pix), C.c_int32(2),
                               lib.ptr(sig), C.c_int32(8))
assert rc != 0 and msg in L.ldsim_last_error().decode(), L.ldsim_last_error()
rc = L.ldsim_tracks_current(lib.context(), lib.ptr(seg), C.c_int64(4), C.byref(lay), lib.ptr(pix), C.c_int32(2),
                            lib.ptr(sig), C.c_int32(8))
assert rc == 0, L.ldsim_last_error()            # (the deterministic stage runs in keyed mode)
ch.seed_rng(4)
assert L.ldsim_rng_is_keyed(lib.context()) == 0
print("refuse ok")
'''


def test_keyed_without_noise_equals_table_and_stage_calls_refuse(tmp_path):
    """keyed mode with every noise constant 0 and the light leg off writes the table-mode file; the host-array stage calls
    that draw refuse in keyed mode with the documented message"""
    noiseless = tmp_path / "noiseless.py"
    noiseless.write_text(_LOOPBACK.split("import json")[0].format(pkg=PKG, cli=CLI) + "cli.main(sys.argv[1:])\n")
    args = _inputs(tmp_path, light=False) + ["--chunk_segments", "80"]
    a = dict(np.load(_run_noiseless(tmp_path, noiseless, args, "table.npz")))
    b = dict(np.load(_run_noiseless(tmp_path, noiseless, args + ["--rng", "keyed"], "keyed.npz")))
    assert len(a["packets"]) > 100
    _assert_same(a, b)
    r = _script(tmp_path, "refuse.py", _REFUSE)
    assert b"refuse ok" in r.stdout
