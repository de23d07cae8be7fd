"""GPU: charge statistics (ChargeChain.set_charge_statistics, simulate_pixels.py --charge_statistics).  The counts of
quench_drift_stat_kernel against the numpy restatement (larndsim_amd/charge_stats.py) fed with the device's own keyed draws,
the exact degenerate limits, the moments of the drawn charge, identity instead of position, off being off, the state rules
and the CLI's files at another chunking.  Every GPU run is a fresh process with a time limit of its own; nothing is retried;
the device work of the tests that share the 4 133-segment input runs once per session."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from larndsim_amd import abi, consts, rng
from larndsim_amd import charge_stats as cs
from larndsim_amd.layout import segments_dtype
from test_gpu_field_map import _tpc_of, _uniform_maps
from test_gpu_multirank import _assert_same, _inputs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "larnd-sim_amd")
CLI = os.path.join(PKG, "cli", "simulate_pixels.py")
TESTS = os.path.dirname(os.path.abspath(__file__))
HEAD = f"import sys, pickle\nsys.path[:0] = [{PKG!r}, {TESTS!r}]\n"
SEED = 0x5EED0C0FFEE
SIZES = [(0, 700), (1, 1203), (-1, 411), (2, 950), (3, 300), (4, 569)]      # (batch id, segments): 4 133 in all
TABLE = [(10, 0, 0, 700), (10, 1, 0, 1203), (11, 0, 0, 950), (11, 1, 0, 300), (12, 0, 0, 569)]
SPLIT = 700 + 1203 + 411
DRIFTED = ["n_electrons", "n_photons", "t", "t_start", "t_end", "long_diff", "tran_diff", "pixel_plane"]


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}


def _run(cmd, timeout):
    r = subprocess.run(cmd, env=_env(), capture_output=True, timeout=timeout)
    assert r.returncode == 0, (cmd, r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    return r


def _job(tmp, name, body, job, timeout=300):
    """run `body` (which reads `job` and leaves `res`) in a fresh process and return its `res`"""
    jp, rp, sp = tmp / f"{name}.job", tmp / f"{name}.res", tmp / f"{name}.py"
    pickle.dump(job, open(jp, "wb"))
    sp.write_text(HEAD + f"job = pickle.load(open({str(jp)!r}, 'rb'))\n" + body +
                  f"\npickle.dump(res, open({str(rp)!r}, 'wb'))\nprint('job ok')\n")
    _run([sys.executable, str(sp)], timeout)
    return pickle.load(open(rp, "rb"))


def _make_segments(n, seed, outside=0.03, dE=None, depth=None):
    """n segments in the simulation frame of module0: dE log-uniform in 1 keV .. 5 MeV, dE/dx in 1.5 .. 25 MeV/cm, the midpoint 0.05 cm .. the full
    drift away from its TPC's anode, a fraction `outside` of them beyond every TPC; `dE` / `depth` (0 .. 1 of the drift) fix
    those for every segment"""
    H.load_cfg("module0")
    rs = np.random.default_rng(seed)
    B = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)
    seg = np.zeros(n, dtype=segments_dtype)
    t = rs.integers(0, len(B), n)
    b = B[t]
    full = np.abs(b[:, 2, 1] - b[:, 2, 0])
    toward = np.sign(b[:, 2, 1] - b[:, 2, 0])
    d = 0.05 + (full - 0.05) * (rs.uniform(0, 1, n) if depth is None else depth)
    x = rs.uniform(b[:, 0, 0] + 1, b[:, 0, 1] - 1)
    y = rs.uniform(b[:, 1, 0] + 1, b[:, 1, 1] - 1)
    z = b[:, 2, 0] + toward * d
    out = rs.uniform(0, 1, n) < outside
    x = np.where(out, b[:, 0, 1] + 40.0 + rs.uniform(0, 5, n), x)
    length = rs.uniform(0.05, 0.4, n)
    u = rs.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    half = 0.5 * length[:, None] * u
    half[:, 2] = np.clip(half[:, 2], -0.02, 0.02)                      # both ends stay on the anode's side of the midpoint
    for k, f in enumerate("xyz"):
        mid = (x, y, z)[k]
        seg[f], seg[f + "_start"], seg[f + "_end"] = mid, mid - half[:, k], mid + half[:, k]
    seg["dx"] = length
    seg["dE"] = np.exp(rs.uniform(np.log(1e-3), np.log(5.0), n)) if dE is None else dE
    seg["dEdx"] = np.exp(rs.uniform(np.log(1.5), np.log(25.0), n)) if dE is None else 2.1     # R from 0.72 down to 0.29
    seg["t0"] = seg["t0_start"] = seg["t0_end"] = rs.uniform(0, 2, n)
    seg["event_id"] = 10
    seg["segment_id"] = np.arange(n)
    seg["pdg_id"] = 13
    return seg, out


def _batch_ids():
    return np.concatenate([np.full(k, b, dtype=np.int32) for b, k in SIZES])


def _restate(seg, zn, un, mode, fano):
    """(n_electrons, n_photons, recombination branch, attachment branch) the kernel must give for the simulated segments,
    from the device's draws zn / un [n][5]"""
    c = abi.pack_consts(noise_zero=True)
    B = np.ctypeslib.as_array(c.tpc_borders)
    x, y, z = (seg[f].astype(np.float64) for f in "xyz")
    plane = _tpc_of(c, x, y, z)
    inside = plane != c.default_plane_index
    z_anode = B[np.where(inside, plane, 0), 2, 0]
    life = np.where(inside, np.exp(-(np.abs(z - z_anode) / c.v_drift) / c.electron_lifetime), np.nan)
    R = cs.recombination(seg["dEdx"].astype(np.float64), mode, c)
    n_ion, n_q, n_e, n_ph = cs.counts(seg["dE"], R, life, zn, un, c.w_ion, c.w_ph, c.scint_prescale, fano)
    rb = cs.binomial_branch(n_ion, np.clip(R, 0, 1))
    ab = np.where(inside, cs.binomial_branch(n_q, np.where(inside, life, 0.0)), False)
    live = (n_ion > 0) & (R > 0) & (R < 1)
    return n_e, n_ph, (rb, live & ~rb), (ab, inside & (n_q > 0) & ~ab)


_SHARED = r'''
import numpy as np
import helpers as H
from larndsim_amd import charge_stats as cs, consts, lib, rng, synth
from larndsim_amd.chain import ChargeChain
H.load_cfg("module0")
seg, bid, table, seed, split = job["seg"], job["bid"], job["table"], job["seed"], job["split"]
res = {}
ch = ChargeChain()


def qd(s, b, t, mode=consts.physics.BIRKS):
    ch.upload(s, b)
    ch.set_batch_keys(t, 1)
    ch.quench_drift(mode)
    return ch.download_segments(s.copy())


# never enabled
ch.upload(seg, bid)
ch.quench_drift()
res["off"] = ch.download_segments(seg.copy())
ch.upload(seg, bid)
ch.quench_drift(consts.physics.BOX)
res["off_box"] = ch.download_segments(seg.copy())
ch.seed_keyed(seed)
res["off_keyed"] = qd(seg, bid, table)
# enabled then disabled
ch.set_charge_statistics(True, 0.107)
assert ch.charge_statistics() == (True, 0.107)
ch.set_charge_statistics(False)
assert ch.charge_statistics() == (False, 0.107)
res["on_off"] = qd(seg, bid, table)
# enabled: Birks, Box, again after reset()
ch.set_charge_statistics(True, 0.107)
res["birks"] = qd(seg, bid, table)
ch.upload(seg, bid)                  # (reset() re-unpacks the staged records, which a download rewrites: reset before any download)
ch.set_batch_keys(table, 1)
ch.quench_drift()
ch.reset()
ch.quench_drift()
res["birks_reset"] = ch.download_segments(seg.copy())
res["box"] = qd(seg, bid, table, consts.physics.BOX)
# the device's own draws 0-4 of every segment's stream
keys = cs.segment_keys(rng.batch_keys(table, 1), bid)
res["keys"] = keys
res["zn"] = rng.keyed_draws(keys, 5, tag=rng.TAG_CHARGE, normal=True, ctx=ch.ctx)
res["un"] = rng.keyed_draws(keys, 5, tag=rng.TAG_CHARGE, normal=False, ctx=ch.ctx)
# two uploads split on a batch boundary: the second with its ids counted from 0 and its own keys, and with the ids and keys kept
first = qd(seg[:split], bid[:split], table[:2])
b2 = bid[split:]
res["split_renumbered"] = np.concatenate([first, qd(seg[split:], b2 - b2.min(), table[2:])])
res["split_kept"] = np.concatenate([first, qd(seg[split:], b2, table)])
# a uniform map on every TPC
ch.set_field_map(job["maps"])
res["uniform_map"] = qd(seg, bid, table)
res["uniform_map_view"] = ch.download_anode_view()
ch.clear_field_map()
ch.set_charge_statistics(False)
'''


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    seg, out = _make_segments(4133, seed=41)
    bid = _batch_ids()
    assert len(bid) == 4133 and len(bid) % 256 != 0 and 0.02 < out.mean() < 0.04
    H.load_cfg("module0")
    maps = _uniform_maps(E=consts.detector.E_FIELD, dx=0, dy=0, dz=0)
    job = dict(seg=seg, bid=bid, table=TABLE, seed=SEED, split=SPLIT, maps=maps)
    res = _job(tmp_path_factory.mktemp("charge_stats"), "shared", _SHARED, job)
    res.update(seg=seg, bid=bid, outside=out)
    return res


@pytest.mark.parametrize("mode", ["birks", "box"])
def test_parity_with_restatement_on_device_draws(shared, mode):
    """n_electrons and n_photons of every simulated segment equal the restatement run on draws 0-4 the device reports for the
    segment's stream; at most 1 segment in 1 000 may differ, by exactly one electron (the device's log / exp against the
    host's in the last bit under a rounding or a CDF comparison); each sampler branch taken by at least 10 % of the segments;
    segments with batch id < 0 hold the values of the mode being off"""
    H.load_cfg("module0")
    seg, bid, got = shared["seg"], shared["bid"], shared[mode]
    sim = bid >= 0
    assert np.array_equal(shared["keys"], cs.segment_keys(rng.batch_keys(TABLE, 1), bid))
    want_e, want_ph, (r_norm, r_inv), (a_norm, a_inv) = _restate(
        seg, shared["zn"], shared["un"], consts.physics.BIRKS if mode == "birks" else consts.physics.BOX, 0.107)
    frac = {k: float(v[sim].mean()) for k, v in dict(recomb_normal=r_norm, recomb_inversion=r_inv, attach_normal=a_norm,
                                                      attach_inversion=a_inv, normal=r_norm | a_norm,
                                                      inversion=r_inv | a_inv).items()}
    print(mode, "sampler branches:", frac)
    assert frac["normal"] >= 0.10 and frac["inversion"] >= 0.10
    assert frac["attach_normal"] >= 0.10 and frac["attach_inversion"] >= 0.10
    de = got["n_electrons"][sim].astype(np.float64) - want_e[sim].astype(got.dtype["n_electrons"]).astype(np.float64)
    ph_want = want_ph[sim].astype(got.dtype["n_photons"])
    dp = got["n_photons"][sim].astype(np.float64) - ph_want.astype(np.float64)
    differ = (de != 0) | (dp != 0)
    print(mode, "segments that differ:", int(differ.sum()), "of", int(sim.sum()), "largest electron difference", np.abs(de).max())
    assert differ.sum() <= sim.sum() / 1000
    assert (np.abs(de) <= 1).all()
    c = abi.pack_consts(noise_zero=True)
    assert (np.abs(dp) <= c.scint_prescale + np.spacing(np.abs(ph_want)).astype(np.float64)).all()
    assert sim.sum() > 3000 and (want_e[sim] > 0).mean() > 0.99
    off = shared["off" if mode == "birks" else "off_box"]
    for f in DRIFTED:                                   # not simulated: the mean values; everything but the counts: as before
        assert np.array_equal(got[f][~sim], off[f][~sim]), f
    for f in ("t", "t_start", "t_end", "long_diff", "tran_diff", "pixel_plane"):
        assert np.array_equal(got[f], off[f]), f
    assert not np.array_equal(got["n_electrons"][sim], off["n_electrons"][sim])


_DEGENERATE = r'''
import numpy as np
import helpers as H
from larndsim_amd import consts
from larndsim_amd.chain import ChargeChain
H.load_cfg("module0")
consts.physics.BIRKS_Ab, consts.physics.BIRKS_kb, consts.detector.ELECTRON_LIFETIME = 1.0, 0.0, 1e30
res = {}
ch = ChargeChain()
ch.seed_keyed(job["seed"])
ch.set_charge_statistics(True, 0.0)
for name in ("seg_u4", "seg_f4"):
    ch.upload(job[name], job["bid"])
    ch.set_batch_keys(job["table"], 1)
    ch.quench_drift(consts.physics.BIRKS)
    res[name] = ch.download_segments(job[name].copy())
ch.set_charge_statistics(False)
'''


def test_degenerate_limits_are_exact(tmp_path):
    """F = 0, Birks with A_b = 1 and k_b = 0, lifetime 10^30: n_electrons = rint(dE / W_ion) in the record's dtype (u4, and
    f4) for every segment, inside a TPC or not"""
    seg, _ = _make_segments(777, seed=43)
    f4_dtype = np.dtype([(n, "f4" if n == "n_electrons" else segments_dtype[n]) for n in segments_dtype.names], align=True)
    seg_f4 = np.zeros(len(seg), dtype=f4_dtype)
    for n in segments_dtype.names:
        seg_f4[n] = seg[n]
    bid = np.repeat(np.arange(3, dtype=np.int32), 259)
    table = [(1, 0, 0, 259), (2, 0, 0, 259), (3, 0, 0, 259)]
    res = _job(tmp_path, "degenerate", _DEGENERATE, dict(seg_u4=seg, seg_f4=seg_f4, bid=bid, table=table, seed=SEED))
    want = np.rint(seg["dE"].astype(np.float64) / consts.physics.W_ION)
    assert want.min() > 30 and want.max() > 1e5
    assert np.array_equal(res["seg_u4"]["n_electrons"], want.astype("u4"))
    assert np.array_equal(res["seg_f4"]["n_electrons"], want.astype("f4"))
    ph = (seg["dE"].astype(np.float64) / consts.light.W_PH - want) * consts.light.SCINT_PRESCALE
    assert np.array_equal(res["seg_u4"]["n_photons"], ph.astype("f4"))


_CLOSURE = r'''
import numpy as np
import helpers as H
from larndsim_amd import consts
from larndsim_amd.chain import ChargeChain
H.load_cfg("module0")
consts.light.SCINT_PRESCALE = job["prescale"]
res = {}
ch = ChargeChain()
ch.seed_keyed(job["seed"])
ch.set_charge_statistics(True, job["fano"])
ch.upload(job["seg"], job["bid"])
ch.set_batch_keys(job["table"], 1)
ch.quench_drift(consts.physics.BIRKS)
res["seg"] = ch.download_segments(job["seg"].copy())
ch.set_charge_statistics(False)
'''


def test_statistical_closure_on_the_device(tmp_path):
    """two groups of 4 096 identical segments, one drawn by inversion and one by the rounded normal in both samplers: sample
    mean and variance of n_electrons within 5 standard errors of N R L and N RL (1 - RL) + F N (RL)^2; outside every TPC
    n_photons + scint_prescale n_q = scint_prescale dE / W_ph to the rounding of the stored fields"""
    M, fano, prescale = 4096, 0.107, 0.25
    low, _ = _make_segments(M, seed=44, outside=0, dE=1.5e-3, depth=0.9)
    high, _ = _make_segments(M, seed=45, outside=0, dE=2.0, depth=0.9)
    far, out = _make_segments(512, seed=46, outside=1.0)
    assert out.all()
    seg = np.concatenate([low, high, far])
    bid = np.concatenate([np.full(M, 0), np.full(M, 1), np.full(512, 2)]).astype(np.int32)
    table = [(1, 0, 0, M), (1, 1, 0, M), (2, 0, 0, 512)]
    got = _job(tmp_path, "closure", _CLOSURE, dict(seg=seg, bid=bid, table=table, seed=SEED + 1, fano=fano,
                                                   prescale=prescale))["seg"]
    H.load_cfg("module0")
    c = abi.pack_consts(noise_zero=True)
    B = np.ctypeslib.as_array(c.tpc_borders)
    for name, sl, normal in (("inversion", slice(0, M), False), ("normal", slice(M, 2 * M), True)):
        s, g = seg[sl], got[sl]
        assert (g["pixel_plane"] != c.default_plane_index).all()
        # the group is identical in what the charge depends on, up to the f4 midpoint's z: use each segment's own L
        z_anode = B[g["pixel_plane"], 2, 0]
        L = np.exp(-(np.abs(s["z"].astype(np.float64) - z_anode) / c.v_drift) / c.electron_lifetime)
        R = cs.recombination(s["dEdx"].astype(np.float64), 2, c)
        N = s["dE"].astype(np.float64) / c.w_ion
        assert np.ptp(R) == 0 and np.ptp(N) == 0 and np.ptp(L) < 2e-3 * L.mean() and L.mean() < 0.95
        assert bool(cs.binomial_branch(np.rint(N[0]), R[0])) is normal
        assert bool(cs.binomial_branch(np.rint(N[0] * R[0]), L.mean())) is normal
        mean, var = cs.mean_variance(s["dE"], R, L, c.w_ion, fano)
        k = g["n_electrons"].astype(np.float64)
        got_mean, got_var = k.mean(), k.var(ddof=1)
        se_mean, se_var = np.sqrt(var.mean() / M), var.mean() * np.sqrt(2.0 / (M - 1))
        print(f"{name}: mean {got_mean:.3f} vs {mean.mean():.3f} ({(got_mean - mean.mean()) / se_mean:+.2f} SE), variance "
              f"{got_var:.3f} vs {var.mean():.3f} ({(got_var - var.mean()) / se_var:+.2f} SE)")
        assert abs(got_mean - mean.mean()) <= 5 * se_mean
        assert abs(got_var - var.mean()) <= 5 * se_var
    f, g = far, got[2 * M:]
    assert (g["pixel_plane"] == c.default_plane_index).all()
    n_q = g["n_electrons"].astype(np.float64)                # u4: a count is stored exactly
    total = prescale * f["dE"].astype(np.float64) / c.w_ph
    err = np.abs(g["n_photons"].astype(np.float64) + prescale * n_q - total)
    tol = 0.5 * np.spacing(np.abs(g["n_photons"])).astype(np.float64) + 4 * np.spacing(total)
    assert (err <= tol).all(), (err / tol).max()
    assert n_q.max() > 1e4 and (g["n_photons"] > 0).all()


def test_identity_not_position(shared):
    """reset() + quench_drift again gives the same records; the same segments in two uploads split on a batch boundary (ids
    renumbered and keys re-set, or ids and keys kept) give the same per-segment values; a uniform map on every TPC is
    bit-identical to no map"""
    ref = shared["birks"]
    for name in ("birks_reset", "split_renumbered", "split_kept", "uniform_map"):
        _assert_same({"s": ref}, {"s": shared[name]})
    view = np.stack([shared["seg"][f].astype(np.float64) for f in
                     ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end", "x", "y", "z")])
    assert np.array_equal(shared["uniform_map_view"], view)
    assert not np.array_equal(shared["box"]["n_electrons"], ref["n_electrons"])


def test_off_is_off(shared):
    """enabling then disabling gives the records of a chain that never enabled, keyed or not"""
    _assert_same({"s": shared["off"]}, {"s": shared["on_off"]})
    _assert_same({"s": shared["off"]}, {"s": shared["off_keyed"]})


_STATE = r'''
import ctypes as C
import numpy as np
import helpers as H
from larndsim_amd import consts, lib, quenching, synth
from larndsim_amd.chain import ChargeChain
from larndsim_amd.layout import make_layout
H.load_cfg("module0")
seg, bid, table = job["seg"], job["bid"], job["table"]
ch = ChargeChain(synth.make_response("survey"))
L = lib.load()


def refused(call, *words):
    try:
        call()
    except lib.LdsimError as e:
        assert "ldsim error -4" in str(e) and all(w in str(e) for w in words), str(e)
        return
    raise SystemExit("accepted: " + " ".join(words))


ch.set_charge_statistics(True)
ch.upload(seg, bid)
refused(ch.quench_drift, "ldsim_rng_keyed_seed")                    # no random mode at all
ch.seed_rng(3, 16)
refused(ch.quench_drift, "ldsim_rng_keyed_seed")                    # table mode
ch.seed_keyed(5)
refused(ch.quench_drift, "ldsim_chain_set_batch_keys")              # keyed, no batch keys
ch.set_batch_keys(table[:2], 1)
refused(ch.quench_drift, "ldsim_chain_set_batch_keys", "batch id 4")     # keys for some of the batches only
ch.set_batch_keys(table, 1)
# host-array stage calls refuse while the mode is enabled
lay = make_layout(seg.dtype)
t = seg.copy()
for name, args in [("ldsim_quench", (C.c_int32(2),)), ("ldsim_drift", ())]:
    rc = getattr(L, name)(ch.ctx, lib.ptr(t), C.c_int64(len(t)), C.byref(lay), *args)
    assert rc == -4 and "charge statistics" in L.ldsim_last_error().decode(), (name, rc)
refused(lambda: quenching.quench(t.copy(), consts.physics.BIRKS), "charge statistics")
# the chain runs on the charge of the setting that holds now
n0 = job["n0"]
refused(lambda: ch.run(0, n0), "changed since")                      # enabled, no quench_drift since the upload
ch.quench_drift()
st = ch.run(0, n0)
assert st.n_unique > 0
ch.set_charge_statistics(False)
refused(lambda: ch.run(0, n0), "changed since")
ch.set_charge_statistics(True, 0.3)
refused(lambda: ch.run(0, n0), "changed since")                      # another Fano factor
ch.set_charge_statistics(True)
ch.run(0, n0)                                                        # the setting of the quench_drift again
ch.set_charge_statistics(False)
ch.reset()
ch.quench_drift()
ch.run(0, n0)
ch.set_charge_statistics(True)
refused(lambda: ch.run(0, n0), "changed since")
assert L.ldsim_set_charge_statistics(ch.ctx, C.c_int32(1), C.c_double(-0.1)) == -1
assert L.ldsim_set_charge_statistics(ch.ctx, C.c_int32(1), C.c_double(float("nan"))) == -1
ch2 = ChargeChain()                                                  # a new chain clears the mode
assert ch2.charge_statistics()[0] is False
quenching.quench(t.copy(), consts.physics.BIRKS)                     # stage calls work again
res = dict(ok=True)
'''


def test_state_rules(shared, tmp_path):
    """quench_drift without keyed mode or without batch keys, a host-array ldsim_quench / ldsim_drift while enabled, and run()
    after the setting changed without a new quench_drift all return LDSIM_ESTATE; a bad Fano factor LDSIM_EINVAL"""
    res = _job(tmp_path, "state", _STATE, dict(seg=shared["seg"], bid=shared["bid"], table=TABLE, n0=SIZES[0][1]))
    assert res["ok"]


def _cli(tmp_path, args, name, timeout=600):
    out = tmp_path / name
    r = _run([sys.executable, CLI] + args + ["--output_filename", str(out)], timeout)
    return dict(np.load(out)), r.stdout.decode()


def test_cli_charge_statistics(tmp_path):
    """--rng keyed --charge_statistics writes the same file at --chunk_segments 40 and 100000 and under --n_gpus 1
    --force_dist, and another one than without the flag (the plain --rng keyed run, whose code path the flag's absence
    leaves alone); the run header names the mode and the Fano factor; the file's counts are whole numbers"""
    keyed = _inputs(tmp_path) + ["--rng", "keyed"]
    plain, log = _cli(tmp_path, keyed + ["--chunk_segments", "40"], "plain.npz")
    assert "Charge statistics: off" in log
    a, log = _cli(tmp_path, keyed + ["--charge_statistics", "--chunk_segments", "40"], "s40.npz")
    assert "Charge statistics: on (--charge_statistics, Fano factor 0.107)" in log
    b, _ = _cli(tmp_path, keyed + ["--charge_statistics", "--chunk_segments", "100000"], "s1e5.npz")
    c, _ = _cli(tmp_path, keyed + ["--charge_statistics", "--chunk_segments", "40", "--n_gpus", "1", "--force_dist"], "dist.npz")
    _assert_same(a, b)
    _assert_same(a, c)
    assert len(a["packets"]) > 100
    assert not np.array_equal(a["segments"]["n_electrons"], plain["segments"]["n_electrons"])
    assert not np.array_equal(a["segments"]["n_photons"], plain["segments"]["n_photons"])
    assert not np.array_equal(a["packets"], plain["packets"])
    ne = a["segments"]["n_electrons"].astype(np.float64)
    assert np.array_equal(ne, np.rint(ne))
