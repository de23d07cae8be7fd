"""GPU: the sharded drop-in driver (simulate_pixels.py --n_gpus) and its exchange (ldsim_compact_accumulate,
ldsim_comm_gather_compact, ldsim_comm_gathered_compact_download, ldsim_comm_gatherv_bytes).  Every run is a fresh process
with a time limit of its own; nothing is retried."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from larndsim_amd import consts, lib, synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "larnd-sim_amd")
CLI = os.path.join(PKG, "cli", "simulate_pixels.py")
TESTS = os.path.dirname(os.path.abspath(__file__))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _run(cmd, timeout, **env):
    r = subprocess.run(cmd, env=_env(**env), capture_output=True, timeout=timeout)
    assert r.returncode == 0, (cmd, r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    return r


def _inputs(tmp_path, n_seg=520, light=True):
    H.load_cfg("module0")
    seg = synth.make_segments(n_seg, seed=21, segs_per_event=40)          # 13 events
    seg = seg[np.random.default_rng(2).permutation(len(seg))]
    np.save(tmp_path / "in.npy", seg)
    np.save(tmp_path / "resp.npy", synth.make_response("survey"))
    args = ["--input_filename", str(tmp_path / "in.npy"), "--config", "module0", "--rand_seed", "7",
            "--response_file", str(tmp_path / "resp.npy")]
    if light:
        np.savez(tmp_path / "lut.npz", arr=synth.make_lut((14, 26, 8), 48, 40, 3))
        noise = np.abs(np.random.default_rng(3).normal(0, 4000.0, (consts.light.N_OP_CHANNEL, 65)))
        np.save(tmp_path / "noise.npy", noise)
        args += ["--light_lut_filename", str(tmp_path / "lut.npz"), "--light_det_noise_filename", str(tmp_path / "noise.npy")]
    else:
        args += ["--light_simulated", "0"]
    return args


def _assert_same(a, b, keys=None):
    assert set(a) == set(b)
    for k in (keys or a):
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, k
        if x.dtype.names:                          # field by field: padding bytes of an aligned record are not data
            for f in x.dtype.names:
                assert np.array_equal(x[f], y[f], equal_nan=True), (k, f)
        else:
            assert np.array_equal(x, y, equal_nan=True), k


def test_cli_force_dist_one_rank_writes_the_same_file(tmp_path):
    """--n_gpus 1 --force_dist (one self-launched rank on the RCCL path: communicator, gather-v of the light results, gather of
    the compact stream) writes the file a plain run writes, FEE noise and light fluctuations and noise on: rank 0 seeds with
    rand_seed itself and owns every event."""
    args = _inputs(tmp_path) + ["--chunk_segments", "40"]
    _run([sys.executable, CLI] + args + ["--output_filename", str(tmp_path / "plain.npz")], 600)
    r = _run([sys.executable, CLI] + args + ["--output_filename", str(tmp_path / "dist.npz"), "--n_gpus", "1", "--force_dist"], 600)
    assert b"simulated " in r.stdout
    a, b = dict(np.load(tmp_path / "plain.npz")), dict(np.load(tmp_path / "dist.npz"))
    assert len(a["packets"]) > 100 and len(a["light_wvfm"]) >= 2 and len(a["light_trig"]) == len(a["light_wvfm"])
    _assert_same(a, b)


_GATHER_SCRIPT = r'''
import sys
sys.path[:0] = [{pkg!r}, {tests!r}]
import numpy as np
import helpers as H
from larndsim_amd import batching, comm, lib, synth
from larndsim_amd.chain import ChargeChain

H.load_cfg("module0")
seg = synth.make_segments(480, seed=9, segs_per_event=40)
batching.swap_coordinates(seg)
bid, order, table = batching.assign_batches(seg)
seg, bid = seg[order], bid[order]
ch = ChargeChain(synth.make_response("survey"))
ch.upload(seg, bid)
ch.quench_drift()
cm = comm.Communicator(ch.ctx, 0, 1)
assert cm.count() == (1, 0)
try:
    cm.gathered_compact(0, np.zeros((1, 5), dtype=np.int64))   # nothing gathered yet
    raise SystemExit("a download without a gather accepted")
except lib.LdsimError as e:
    assert "holds no gathered" in str(e), str(e)
cm.accumulate_compact(reset=True)
local = []
ranges = batching.chunk_ranges(bid, 60)
assert len(ranges) >= 4
for b0, e0 in ranges:
    ch.run(b0, e0, want_fractions=True)
    local.append(ch.download_compact())
    cm.accumulate_compact()
try:
    cm.accumulate_compact()                         # the same launch twice: refused
    raise SystemExit("a launch was appended twice")
except lib.LdsimError:
    pass
sizes = cm.gather_compact(0)
got = cm.gathered_compact(0, sizes)
for k in ("hit_pixels", "track_segments", "hit_rows", "hit_charge", "fractions"):
    want = np.concatenate([c[k] for c in local])
    assert got[k].shape == want.shape and got[k].tobytes() == want.tobytes(), k
assert len(got["hit_rows"]) > 100 and len(got["fractions"]) > 100
assert list(sizes[0]) == [len(got["hit_pixels"]), len(got["track_segments"]), len(got["hit_rows"]), len(got["hit_charge"]),
                          len(got["fractions"])]
for bad, what in ((lambda: cm.gather_compact(0, root=1), "root out of range"), (lambda: cm.gatherv_bytes(b"x", root=-1), "root out of range"),
                  (lambda: cm.gather_compact(1), "source rank out of range")):
    try:
        bad()
        raise SystemExit(what + " accepted")
    except lib.LdsimError as e:
        assert what in str(e), str(e)
cm.accumulate_compact(reset=True)
assert (cm.gather_compact(0) == 0).all()
rng = np.random.default_rng(4)
for n in (0, 1, 7, 1001, 65537, 0, 3):
    data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    counts = cm.gatherv_bytes(data)
    assert list(counts) == [n]
    assert cm.gathered_bytes(0, counts) == data, n
cm.destroy()
print("gather ok", len(ranges), "launches")
'''


def test_gathered_compact_equals_local_compact(tmp_path):
    """several launches through ldsim_compact_accumulate -> ldsim_comm_gather_compact(root 0) ->
    ldsim_comm_gathered_compact_download equal the concatenation of their ldsim_chain_compact_download results; gather-v of
    host bytes round-trips odd lengths and 0; a root out of range is refused (fresh one-rank process)"""
    script = tmp_path / "gather.py"
    script.write_text(_GATHER_SCRIPT.format(pkg=PKG, tests=TESTS))
    r = _run([sys.executable, str(script)], 300, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    assert b"gather ok" in r.stdout


_NOISELESS_HEAD = r'''
import importlib.util
import sys
sys.path.insert(0, {pkg!r})
from larndsim_amd import consts
_load = consts.load_snapshot


def load_snapshot(*a, **k):
    r = _load(*a, **k)
    consts.detector.RESET_NOISE_CHARGE = consts.detector.UNCORRELATED_NOISE_CHARGE = consts.detector.DISCRIMINATOR_NOISE = 0
    return r


consts.load_snapshot = load_snapshot
spec = importlib.util.spec_from_file_location("sp_cli", {cli!r})
cli = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cli)
'''
_NOISELESS = _NOISELESS_HEAD + "cli.main(sys.argv[1:])\n"


def _compare_sharded(a, b, light):
    """a one-rank file against a sharded one, FEE noise 0: light off, every dataset; light on, the deterministic datasets and
    the charge packets with their association rows, the light datasets by schema"""
    if not light:
        assert len(a["packets"]) > 100
        _assert_same(a, b)
        return
    _assert_same(a, b, keys=["segments", "light_dat__light_dat_allmodules"])
    for k in ("light_trig", "light_wvfm", "light_wvfm_mc_assn"):
        if k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape[1:] == b[k].shape[1:], k
    assert len(b["light_wvfm"]) == len(b["light_trig"]) >= 2
    if "light_wvfm_mc_assn" in a:
        assert np.array_equal(np.unique(a["light_wvfm_mc_assn"]["event_id"]), np.unique(b["light_wvfm_mc_assn"]["event_id"]))
    da, db = a["packets"]["packet_type"] == 0, b["packets"]["packet_type"] == 0
    assert da.sum() > 100
    for f in a["packets"].dtype.names:
        assert np.array_equal(a["packets"][f][da], b["packets"][f][db]), f
    for f in a["mc_packets_assn"].dtype.names:
        assert np.array_equal(a["mc_packets_assn"][f][da], b["mc_packets_assn"][f][db]), f


_LOOPBACK = _NOISELESS_HEAD + r'''
import json
import os
import numpy as np
from larndsim_amd import comm, lib

Real = comm.Communicator
box = dict(light=[], compact=[])


class Loopback:
    """rank `rank` of a world-2 communicator, both ranks played one after the other in this process: rank 1's run leaves what
    it sends in `box`, rank 0's run receives it from there.  Rank 1's compact stream still goes through the device path
    (ldsim_compact_accumulate -> ldsim_comm_gather_compact -> ldsim_comm_gathered_compact_download) of a real one-rank
    communicator; only the ncclSend / ncclRecv between two GPUs is left out."""

    def __init__(self, ctx, rank, world):
        assert world == 2
        self.rank, self.world = rank, world
        self.real = Real(ctx, 0, 1)

    def count(self):
        return 2, self.rank

    def accumulate_compact(self, reset=False):
        self.real.accumulate_compact(reset)

    def gatherv_bytes(self, data, root=0):
        if self.rank == 1:
            box["light"].append(bytes(data))
            return None
        assert data == b""
        self.light = box["light"].pop(0)
        return np.array([0, len(self.light)])

    def gathered_bytes(self, r, counts):
        assert r == 1 and counts[1] == len(self.light)
        return self.light

    def gather_compact(self, src_rank, root=0):
        assert src_rank == 1 and root == 0
        if self.rank == 1:
            s = self.real.gather_compact(0)
            box["compact"].append((s[0].copy(), self.real.gathered_compact(0, s)))
            return None
        s, self.c = box["compact"].pop(0)
        return np.stack([np.zeros(5, dtype=np.int64), s])

    def gathered_compact(self, r, sizes, has_fractions=True):
        assert r == 1 and len(self.c["hit_rows"]) == sizes[1][2]
        return self.c

    def destroy(self):
        self.real.destroy()


comm.Communicator = Loopback
lib.device_count = lambda: 2
args = json.loads(sys.argv[1])
res = {{}}
os.environ["WORLD_SIZE"] = "2"
for rank in (1, 0):
    os.environ["RANK"] = str(rank)
    res[rank] = cli.run_simulation(**args)
assert res[1] is None and not box["light"] and not box["compact"]
print("LOOPBACK " + json.dumps(res[0]))
'''


def test_cli_rank_1_results_merged_by_rank_0(tmp_path):
    """The rank > 0 side of --n_gpus 2 on one GPU: both ranks of a world-2 run played one after the other in one process, the
    RCCL transfer between them replaced by a hand-over in memory (rank 1's compact stream still goes through the device
    accumulate / gather / download).  Rank 1 simulates its own events, writes nothing and ships its light results and compact
    stream; rank 0 merges them after its own (light rows, trigger tuples, truth trigger ids, the multi-launch compact stream
    exported batch by batch).  FEE noise 0: against a plain run, every dataset equal with the light leg off; with it on, what
    does not follow the rank-dependent random streams."""
    import json
    script = tmp_path / "loopback.py"
    script.write_text(_LOOPBACK.format(pkg=PKG, cli=CLI))
    plain = tmp_path / "noiseless.py"
    plain.write_text(_NOISELESS.format(pkg=PKG, cli=CLI))
    for light in (False, True):
        argv = _inputs(tmp_path, light=light) + ["--chunk_segments", "40"]
        one, two = tmp_path / f"one{int(light)}.npz", tmp_path / f"two{int(light)}.npz"
        _run([sys.executable, str(plain)] + argv + ["--output_filename", str(one)], 600)
        kw = dict(input_filename=argv[1], output_filename=str(two), config="module0", rand_seed=7, response_file=argv[7],
                  chunk_segments=40, n_gpus=2)
        if light:
            kw.update(light_lut_filename=argv[9], light_det_noise_filename=argv[11])
        else:
            kw.update(light_simulated=False)
        r = _run([sys.executable, str(script), json.dumps(kw)], 600)
        tot = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("LOOPBACK ")][0][9:])
        assert tot["n_ranks"] == 2 and min(tot["rows_per_rank"]) > 50 and sum(tot["rows_per_rank"]) == tot["n_hits"]
        a, b = dict(np.load(one)), dict(np.load(two))
        _compare_sharded(a, b, light)
        if light:
            assert tot["n_light_triggers"] == len(b["light_wvfm"])


def _devices():
    try:
        return lib.device_count()
    except Exception:
        return 0


@pytest.mark.skipif(_devices() < 2, reason="two ranks need two GPUs (RCCL does not put two ranks on one device)")
def test_cli_two_ranks_equal_one_rank(tmp_path):
    """--n_gpus 2 (ranks started by a launcher: larndsim_amd.launch.launch_ranks) against a plain run, FEE noise constants 0.
    Light leg off: every dataset equal.  Light leg on: segments, light_dat and the charge packets with their association rows
    equal; the light datasets have the same schema and cover the same events (threshold triggers follow the fluctuated light,
    whose random streams depend on the rank count)."""
    from larndsim_amd import launch
    script = tmp_path / "noiseless.py"
    script.write_text(_NOISELESS.format(pkg=PKG, cli=CLI))
    for light in (False, True):
        args = _inputs(tmp_path, light=light) + ["--chunk_segments", "80"]
        one, two = tmp_path / f"one{int(light)}.npz", tmp_path / f"two{int(light)}.npz"
        _run([sys.executable, str(script)] + args + ["--output_filename", str(one)], 600)
        code, bad = launch.launch_ranks([sys.executable, str(script)] + args + ["--output_filename", str(two), "--n_gpus", "2"], 2,
                                       timeout=600)
        assert code == 0, bad
        _compare_sharded(dict(np.load(one)), dict(np.load(two)), light)
