"""CPU: charge statistics (larndsim_amd/charge_stats.py, simulate_pixels.py --charge_statistics) -- the binomial sampler of
quench_drift_stat_kernel as restated in numpy: exact on degenerate inputs, both branches taken, and on keyed draws made with
the numpy Philox of test_cpu_keyed_rng its sample mean and variance within 5 standard errors of n p and n p (1 - p); the
CLI's switch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from larndsim_amd import charge_stats as cs
from larndsim_amd import rng
from test_cpu_keyed_rng import keyed_normals, keyed_uniforms

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
SEED = 20260101
M = 20000


def _draws(case, idx_normal, idx_uniform, m=M):
    keys = rng.key_mix(np.uint64(rng.KEY_ROOT), np.full(m, case, dtype=np.int64), np.arange(m, dtype=np.int64))
    z, _ = keyed_normals(SEED, rng.TAG_CHARGE, keys, idx_normal)
    return z, keyed_uniforms(SEED, rng.TAG_CHARGE, keys, idx_uniform)


def test_sampler_degenerate_inputs_are_exact():
    z, u = _draws(0, cs.DRAW_RECOMB_Z, cs.DRAW_RECOMB_U, 512)
    for n in (0.0, 1.0, 7.0, 300.0, 40000.0, 212000.0):
        assert np.array_equal(cs.binomial(n, 0.0, z, u), np.zeros(512))
        assert np.array_equal(cs.binomial(n, -0.5, z, u), np.zeros(512))
        assert np.array_equal(cs.binomial(n, 1.0, z, u), np.full(512, n))
        assert np.array_equal(cs.binomial(n, 1.5, z, u), np.full(512, n))
    for p in (0.0, 1e-9, 0.3, 0.5, 0.999, 1.0):
        assert np.array_equal(cs.binomial(0.0, p, z, u), np.zeros(512))
    # every draw is a whole number in [0, n], whatever the branch
    n = np.repeat([1.0, 5.0, 50.0, 256.0, 1000.0, 5000.0, 60000.0, 212000.0], 64)
    for p in (1e-6, 0.004, 0.3, 0.5, 0.7, 0.996, 1 - 1e-9):
        k = cs.binomial(n, p, z, u)
        assert np.array_equal(k, np.rint(k)) and (k >= 0).all() and (k <= n).all(), p


@pytest.mark.parametrize("case,n,p,normal", [(1, 50, 0.3, False), (2, 5000, 0.999, False), (3, 5000, 0.7, True),
                                             (4, 40000, 0.92, True)])
def test_sampler_mean_and_variance_within_5_standard_errors(case, n, p, normal):
    assert bool(cs.binomial_branch(n, p)) is normal
    z, u = _draws(case, cs.DRAW_RECOMB_Z, cs.DRAW_RECOMB_U)
    k = cs.binomial(float(n), p, z, u)
    mean, var = n * p, n * p * (1 - p)
    se_mean, se_var = np.sqrt(var / M), var * np.sqrt(2.0 / (M - 1))
    got_mean, got_var = k.mean(), k.var(ddof=1)
    print(f"(n, p) = ({n}, {p}): mean {got_mean:.4f} vs {mean:.4f} ({(got_mean - mean) / se_mean:+.2f} SE), "
          f"variance {got_var:.4f} vs {var:.4f} ({(got_var - var) / se_var:+.2f} SE)")
    assert abs(got_mean - mean) <= 5 * se_mean
    assert abs(got_var - var) <= 5 * se_var
    assert len(np.unique(k)) > 5


def test_counts_limits_and_moments():
    """F = 0, R = 1, no attachment: n_electrons = rint(dE / W_ion) and the photons close the energy balance; with all three
    processes on, the analytic mean and variance hold within 5 standard errors"""
    w_ion, w_ph = 23.6e-6, 19.5e-6
    dE = np.exp(np.random.default_rng(1).uniform(np.log(1e-3), np.log(5.0), 3000))
    keys = rng.key_mix(np.uint64(rng.KEY_ROOT), np.arange(3000, dtype=np.int64))
    zn = np.stack([keyed_normals(SEED, rng.TAG_CHARGE, keys, i)[0] for i in range(5)], 1)
    un = np.stack([keyed_uniforms(SEED, rng.TAG_CHARGE, keys, i) for i in range(5)], 1)
    n_ion, n_q, n_e, n_ph = cs.counts(dE, np.ones(3000), np.ones(3000), zn, un, w_ion, w_ph, 0.5, fano=0.0)
    assert np.array_equal(n_ion, np.rint(dE / w_ion)) and np.array_equal(n_q, n_ion) and np.array_equal(n_e, n_ion)
    assert np.array_equal(n_ph, (dE / w_ph - n_q) * 0.5)
    outside = np.full(3000, np.nan)
    _, n_q, n_e, _ = cs.counts(dE, np.full(3000, 0.7), outside, zn, un, w_ion, w_ph)
    assert np.array_equal(n_q, n_e)                      # outside every TPC: nothing attaches
    for case, (e, r, life) in enumerate([(0.004, 0.66, 0.93), (2.0, 0.71, 0.85)]):      # inversion / normal branches
        z5 = np.stack([_draws(10 + case, i, i)[0] for i in range(5)], 1)
        u5 = np.stack([_draws(10 + case, i, i)[1] for i in range(5)], 1)
        _, _, n_e, _ = cs.counts(np.full(M, e), np.full(M, r), np.full(M, life), z5, u5, w_ion, w_ph)
        mean, var = cs.mean_variance(e, r, life, w_ion)
        assert abs(n_e.mean() - mean) <= 5 * np.sqrt(var / M)
        assert abs(n_e.var(ddof=1) - var) <= 5 * var * np.sqrt(2.0 / (M - 1))


def test_segment_keys_follow_the_index_within_the_batch():
    bk = rng.batch_keys([(3, 0, 0, 2), (3, 1, 0, 3), (4, 0, 0, 1)], 1)
    bid = np.array([0, 0, -1, -1, 1, 1, 1, 2], dtype=np.int32)
    keys = cs.segment_keys(bk, bid)
    want = [rng.key_mix(bk[0], 0), rng.key_mix(bk[0], 1), 0, 0, rng.key_mix(bk[1], 0), rng.key_mix(bk[1], 1),
            rng.key_mix(bk[1], 2), rng.key_mix(bk[2], 0)]
    assert [int(k) for k in keys] == [int(k) for k in want]
    assert np.array_equal(cs.segment_keys(bk[1:], bid[4:] - 1), keys[4:])      # the second part uploaded on its own


def test_cli_charge_statistics_needs_keyed_streams():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sp_cli_charge", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--input_filename", "x.npy", "--output_filename", "y.npz"]
    a = cli._parse_args(base)
    assert a.charge_statistics is False and a.fano_factor is None
    a = cli._parse_args(base + ["--rng", "keyed", "--charge_statistics"])
    assert a.charge_statistics is True and a.fano_factor is None and a.rng == "keyed"
    a = cli._parse_args(base + ["--rng", "keyed", "--charge_statistics", "--fano_factor", "0.2"])
    assert a.fano_factor == 0.2
    for bad in (["--charge_statistics"], ["--charge_statistics", "--rng", "table"], ["--rng", "keyed", "--fano_factor", "0.1"],
                ["--rng", "keyed", "--charge_statistics", "--fano_factor", "-1"]):
        with pytest.raises(SystemExit):
            cli._parse_args(base + bad)
    r = subprocess.run([sys.executable, CLI] + base + ["--charge_statistics"], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"--charge_statistics" in r.stderr and b"--rng keyed" in r.stderr
    assert not os.path.exists("y.npz")
