"""GPU: SiPM correlated noise of the light fluctuation stage (ChargeChain.set_sipm_noise, ldsim_sipm_stat_fluctuations,
simulate_pixels.py --sipm_*).  The counts of light_sipm_count_kernel against the numpy restatement (larndsim_amd/sipm_noise.py)
fed with the device's own keyed draws, off being off, determinism and identity, the cascade's moments on the device, the resident
response and the nominal light universe against the stage call, the state rules and the CLI's light_wvfm at another chunking.
Every GPU run is a fresh process with a time limit of its own; nothing is retried; the stage-call work that several tests read
runs once per session."""
import subprocess
import sys

import numpy as np
import pytest

from larndsim_amd import rng
from larndsim_amd import sipm_noise as sn
from test_cpu_sipm_noise import TICK, check_moments
from test_gpu_charge_stats import CLI, REPO, _cli, _job
from test_gpu_multirank import _inputs

pytestmark = pytest.mark.gpu

SEED = 0x51B3A11CE
KEY, OTHER_KEY = rng.call_key(1, 3, 0, 0), rng.call_key(1, 3, 0, 1)
N_DET, N_TICKS = 3, 700                 # 700 is no multiple of 256: a tail block, and row ends inside a block
PARAMS = sn.params(crosstalk=0.3, afterpulse=0.1, afterpulse_tau=0.05, dark_rate=2.0)
IMPULSE = 2000.0


def _rate():
    """per element 0, a mean in (0, 30) or a mean in [30, 400] (a third each), and an impulse on the last tick of rows 0 and 1"""
    rs = np.random.default_rng(17)
    kind = rs.integers(0, 3, (N_DET, N_TICKS))
    mean = np.where(kind == 0, 0.0, np.where(kind == 1, rs.uniform(0.01, 29.9, kind.shape), rs.uniform(30.0, 400.0, kind.shape)))
    mean[0, -1] = mean[1, -1] = IMPULSE
    return (mean / TICK).astype(np.float32)


_SHARED = r'''
import numpy as np
import helpers as H
from larndsim_amd import consts, rng
from larndsim_amd import sipm_noise as sn
from larndsim_amd.chain import ChargeChain
H.load_cfg("module0")
assert consts.light.LIGHT_TICK_SIZE == job["tick"]
rate, P = job["rate"], job["params"]
res = {}
ch = ChargeChain()
ch.seed_keyed(job["seed"])
ch.set_rng_key(job["key"])
assert ch.sipm_noise()[0] is False
res["off"] = sn.stat_fluctuations(rate, ctx=ch.ctx)                       # never enabled: the plain keyed stage
ch.set_sipm_noise()                                                        # enabled, the four constants zero
assert ch.sipm_noise() == (True, sn.params())
res["zero"], res["zero_counts"] = sn.stat_fluctuations(rate, counts=True, ctx=ch.ctx)
ch.set_sipm_noise(**P)
assert ch.sipm_noise() == (True, P)
res["out"], res["counts"] = sn.stat_fluctuations(rate, counts=True, ctx=ch.ctx)
res["again"] = sn.stat_fluctuations(rate, counts=True, ctx=ch.ctx)
# the same rows with nothing before them but other rows behind them, and the first row alone
res["longer"] = sn.stat_fluctuations(np.concatenate([rate, job["behind"]]), counts=True, ctx=ch.ctx)
res["row0"] = sn.stat_fluctuations(rate[:1], counts=True, ctx=ch.ctx)
ch.set_rng_key(job["other_key"])
res["other_key"] = sn.stat_fluctuations(rate, counts=True, ctx=ch.ctx)
# the device's own draws of every element's stream: 0 .. 35 tell the largest n_ap, then 0 .. 64 + that
keys = sn.element_keys(job["key"], *rate.shape).ravel()
draws = lambda nd, normal: rng.keyed_draws(keys, nd, tag=rng.TAG_LIGHT_FLUCT, normal=normal, ctx=ch.ctx)
n_ap = sn.avalanches(rate, job["tick"], P, draws(sn.N_FIXED_DRAWS, False), draws(sn.N_FIXED_DRAWS, True))["n_ap"]
nd = sn.DRAW_DELAY + int(n_ap.max()) + 1
res["un"], res["zn"] = draws(nd, False), draws(nd, True)
# the cascade's moments: 8 x 8192 elements of constant mean 3, lambda = 0.2, no after-pulses or dark counts
ch.set_rng_key(job["key"])
ch.set_sipm_noise(crosstalk=0.2)
res["moments"] = sn.stat_fluctuations(np.full((8, 8192), 3.0 / job["tick"], dtype=np.float32), counts=True, ctx=ch.ctx)[1]
ch.set_sipm_noise(enable=False)
assert ch.sipm_noise() == (False, sn.params(crosstalk=0.2))
res["on_off"] = sn.stat_fluctuations(rate, ctx=ch.ctx)
'''


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    rate = _rate()
    behind = np.full((2, N_TICKS), 300.0 / TICK, dtype=np.float32)
    job = dict(rate=rate, behind=behind, params=PARAMS, seed=SEED, key=KEY, other_key=OTHER_KEY, tick=TICK)
    res = _job(tmp_path_factory.mktemp("sipm_noise"), "shared", _SHARED, job, timeout=240)
    res["rate"] = rate
    return res


def test_counts_equal_the_twin_on_device_draws(shared):
    """[3][700] rates (zeros, both Poisson branches, an impulse on the last tick of rows 0 and 1) at lambda = 0.3, p = 0.1,
    tau = 0.05 us, r = 2 per us: the device's counts equal sipm_noise.counts on the device's own uniforms and normals integer
    for integer, and the output is float32(1 / tick * count) bit for bit"""
    rate, got = shared["rate"], shared["counts"]
    want, d = sn.counts(rate, TICK, PARAMS, shared["un"], shared["zn"], detail=True)
    mean = rate.astype(np.float64) * TICK
    assert (rate == 0).mean() > 0.25 and ((mean > 0) & (mean < 30)).mean() > 0.25 and (mean >= 30).mean() > 0.25
    assert shared["un"].shape[1] == sn.DRAW_DELAY + d["n_ap"].max() + 1 and d["n_ap"].max() > 150
    print("avalanches", int(d["N"].sum()), "dark", int(d["n_d"].sum()), "after-pulses", int(d["n_ap"].sum()), "dropped",
          int(d["dropped"].sum()), "elements that differ", int((got != want).sum()))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert shared["out"].tobytes() == sn.to_rate(got, TICK).tobytes()
    # what the case is meant to exercise did happen
    assert (d["N"] > d["n_p"] + d["n_d"]).mean() > 0.3 and (d["n_d"][rate == 0] > 0).any()
    assert d["dropped"][0, -1] == d["n_ap"][0, -1] > 150 and d["dropped"][1, -1] == d["n_ap"][1, -1] > 150
    assert (want != d["N"]).mean() > 0.3 and 0 < d["dropped"].sum() < d["n_ap"].sum()
    assert want.sum() == d["N"].sum() + d["n_ap"].sum() - d["dropped"].sum()


def test_off_is_off(shared):
    """enabled with the four constants zero, and enabled then disabled, give the never-enabled output bit for bit"""
    assert shared["zero"].tobytes() == shared["off"].tobytes()
    assert shared["on_off"].tobytes() == shared["off"].tobytes()
    assert shared["zero"].tobytes() == sn.to_rate(shared["zero_counts"], TICK).tobytes()
    assert shared["out"].tobytes() != shared["off"].tobytes() and shared["off"].any()


def test_determinism_and_identity(shared):
    """the same call twice gives the same bits; the three rows equal themselves as the first rows of a longer array (bright rows
    behind them) and row 0 equals itself alone: a count depends on (call key, row, tick) and on nothing else in the call; under
    another call key the counts change"""
    out, cnt = shared["out"], shared["counts"]
    assert shared["again"][0].tobytes() == out.tobytes() and np.array_equal(shared["again"][1], cnt)
    longer_out, longer_cnt = shared["longer"]
    assert longer_cnt.shape == (N_DET + 2, N_TICKS) and longer_cnt[N_DET:].min() > 100
    assert np.array_equal(longer_cnt[:N_DET], cnt) and longer_out[:N_DET].tobytes() == out.tobytes()
    assert np.array_equal(shared["row0"][1], cnt[:1]) and shared["row0"][0].tobytes() == out[:1].tobytes()
    assert (shared["other_key"][1] != cnt).mean() > 0.3


def test_cascade_moments_on_the_device(shared):
    """8 x 8192 elements of constant mean 3 at lambda = 0.2: mean and variance of the device's counts within the CPU test's
    bounds of the analytic values"""
    n = shared["moments"]
    assert n.shape == (8, 8192)
    check_moments(n, 3.0, 0.2, "device")


_RESIDENT = r'''
sys.path.insert(0, job["repo"])                         # (the light universes' tests read the oracle package)
import numpy as np
from larndsim_amd import lib
from larndsim_amd import light_universes as LU
from larndsim_amd import sipm_noise as sn
from test_gpu_light_universes import T_SHORT, _launch
P = job["params"]
res = {}
ch, opc, nt = _launch(n_ticks=T_SHORT)                    # keyed, the call key set
ch.light_response(fluctuate=True)
res["never_on"] = ch.download_light_response(stages=True)[1]
ch.set_sipm_noise(**P)
ch.light_response(fluctuate=True)
sc, res["disc"], rp, _, _ = ch.download_light_response(stages=True)
res["scint"] = sc
res["stage"] = sn.stat_fluctuations(sc, ctx=ch.ctx)       # the same call key
ch.light_universes([LU.nominal()], fluctuate=True, keep_stages=True)
sc_u, res["disc_universe"], rp_u = ch.download_light_universe(0, stages=True)
assert sc_u.tobytes() == sc.tobytes() and rp_u.tobytes() == rp.tobytes()
ch.set_sipm_noise(enable=False)
ch.light_response(fluctuate=True)
res["off_again"] = ch.download_light_response(stages=True)[1]
# table mode: the setter accepts, the fluctuation refuses
ch.seed_rng(3, 1024)
ch.set_sipm_noise(**P)
try:
    ch.light_response(fluctuate=True)
    raise SystemExit("accepted in table mode")
except lib.LdsimError as e:
    assert "ldsim error -4" in str(e) and "ldsim_rng_keyed_seed" in str(e), str(e)
ch.set_sipm_noise(enable=False)
'''


def test_resident_response_and_nominal_universe(tmp_path):
    """the smallest launch of the light universes' tests (96 rows of 1 003 ticks): under set_sipm_noise the disc of
    light_response(fluctuate=True) equals the stage call on the downloaded scint under the same call key, and so does the
    nominal light universe's; after set_sipm_noise(enable=False) disc equals the launch that never had it on; in table mode
    the fluctuation is refused"""
    res = _job(tmp_path, "resident", _RESIDENT, dict(params=sn.params(0.2, 0.03, 0.1, 1.0), repo=REPO), timeout=240)
    assert res["scint"].shape == (96, 1003) and res["scint"].sum() > 0
    assert res["disc"].tobytes() == res["stage"].tobytes()
    assert res["disc_universe"].tobytes() == res["stage"].tobytes()
    assert res["off_again"].tobytes() == res["never_on"].tobytes()
    assert res["disc"].tobytes() != res["never_on"].tobytes()
    assert (res["disc"][res["scint"] <= 0] > 0).any()                  # dark counts where no light fell


_STATE = r'''
import ctypes as C
import numpy as np
import helpers as H
from larndsim_amd import lib
from larndsim_amd import sipm_noise as sn
from larndsim_amd.chain import ChargeChain
H.load_cfg("module0")
tick = job["tick"]
good = job["params"]
rate = np.full((2, 300), 5.0 / tick, dtype=np.float32)
ch = ChargeChain()


def refused(call, code, *words):
    try:
        call()
    except lib.LdsimError as e:
        assert f"ldsim error {code}:" in str(e) and all(w in str(e) for w in words), str(e)
        return
    raise SystemExit("accepted: " + " ".join(words))


ch.seed_keyed(5)
ch.set_rng_key(9)
ch.set_sipm_noise(**good)
BAD = [("crosstalk", dict(crosstalk=0.6)), ("crosstalk", dict(crosstalk=-0.1)), ("crosstalk", dict(crosstalk=float("nan"))),
       ("afterpulse", dict(afterpulse=0.7)), ("afterpulse", dict(afterpulse=-0.01)),
       ("afterpulse_tau", dict(afterpulse=0.1, afterpulse_tau=0.0)), ("afterpulse_tau", dict(afterpulse=0.1, afterpulse_tau=-1.0)),
       ("afterpulse_tau", dict(afterpulse=0.1, afterpulse_tau=float("inf"))),
       ("dark_rate", dict(dark_rate=-1.0)), ("dark_rate", dict(dark_rate=30.0 / tick)), ("dark_rate", dict(dark_rate=float("inf")))]
for enabled in (True, False):
    for field, change in BAD:
        refused(lambda: ch.set_sipm_noise(**dict(good, **change)), -1, "SiPM noise: " + field + " ")
        assert ch.sipm_noise() == (enabled, good), (field, change)
    if enabled:
        ch.set_sipm_noise(0.5, 0.5, 1e-6, 29.0 / tick)              # the ends of the ranges are inside
        ch.set_sipm_noise(afterpulse_tau=0.0)                       # tau is free while afterpulse = 0
        ch.set_sipm_noise(**good)
        ch.set_sipm_noise(enable=False)                             # the values are kept
# counts exist only while enabled
refused(lambda: sn.stat_fluctuations(rate, counts=True, ctx=ch.ctx), -4, "ldsim_set_sipm_noise")
plain = sn.stat_fluctuations(rate, ctx=ch.ctx)
# enabling outside keyed mode: the setter accepts, the fluctuation refuses
ch.seed_rng(3, 16)
ch.set_sipm_noise(**good)
refused(lambda: sn.stat_fluctuations(rate, ctx=ch.ctx), -4, "ldsim_rng_keyed_seed")
assert ch.sipm_noise() == (True, good)
ch.seed_keyed(5)
ch.set_rng_key(9)
noisy = sn.stat_fluctuations(rate, ctx=ch.ctx)
assert noisy.tobytes() != plain.tobytes()
L = lib.load()
assert L.ldsim_set_sipm_noise(ch.ctx, C.c_int32(1), None) == -1      # enabling needs the constants
ch2 = ChargeChain()                                                  # a new chain switches it off and keeps the values
assert ch2.sipm_noise() == (False, good)
assert sn.stat_fluctuations(rate, ctx=ch2.ctx).tobytes() == plain.tobytes()
res = dict(ok=True)
'''


def test_state_and_errors(tmp_path):
    """every out-of-range field is refused (LDSIM_EINVAL) with its name in the message and leaves the getter's values as they
    were, enabled or not; counts while disabled and a fluctuation while enabled in table mode are refused (LDSIM_ESTATE); the
    values survive enable = 0 and a new ChargeChain starts with the noise off"""
    assert _job(tmp_path, "state", _STATE, dict(params=PARAMS, tick=TICK), timeout=240)["ok"]


def test_cli_sipm_noise(tmp_path):
    """--rng keyed --light_simulated true --sipm_crosstalk 0.2 --sipm_afterpulse 0.03 --sipm_afterpulse_tau 0.1 on the smallest
    input of the CLI tests: light_wvfm is identical at --chunk_segments 40 and 100000 and differs from the run without the
    flags; the run header names the setting; the flags without --rng keyed exit with the parser's error"""
    base = _inputs(tmp_path) + ["--light_simulated", "true"]
    keyed = base + ["--rng", "keyed"]
    flags = ["--sipm_crosstalk", "0.2", "--sipm_afterpulse", "0.03", "--sipm_afterpulse_tau", "0.1"]
    plain, log = _cli(tmp_path, keyed + ["--chunk_segments", "40"], "plain.npz")
    assert "SiPM noise: off" in log
    a, log = _cli(tmp_path, keyed + flags + ["--chunk_segments", "40"], "s40.npz")
    assert "SiPM noise: on (--sipm_crosstalk 0.2, --sipm_afterpulse 0.03, --sipm_afterpulse_tau 0.1 us, --sipm_dark_rate 0 per us)" in log
    b, _ = _cli(tmp_path, keyed + flags + ["--chunk_segments", "100000"], "s1e5.npz")
    assert a["light_wvfm"].shape == b["light_wvfm"].shape and len(a["light_wvfm"]) >= 2
    assert a["light_wvfm"].tobytes() == b["light_wvfm"].tobytes()
    assert a["light_wvfm"].shape != plain["light_wvfm"].shape or not np.array_equal(a["light_wvfm"], plain["light_wvfm"])
    r = subprocess.run([sys.executable, CLI] + base + flags + ["--output_filename", str(tmp_path / "no.npz")],
                       capture_output=True, timeout=120)
    assert r.returncode == 2 and b"--sipm_crosstalk" in r.stderr and b"--rng keyed" in r.stderr
    assert not (tmp_path / "no.npz").exists()
