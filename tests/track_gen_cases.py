"""Inputs shared by the track generator's tests and tools (not a test module)."""
import numpy as np

from larndsim_amd import track_generator as TG

# test 1 of tests/test_gpu_track_generator.py: 2048 primaries of mixed particles, energies and directions.  SEED1 is a seed for
# which the numpy twin in f64 and in longdouble agree on every primary's segment count and end state and on every column to
# 1e-6 (found on the host: seeds 20250101, 20250102, .. tried in order, the first that passes taken; see `twin_self_check`).
N1 = 2048
SEED1 = 20250101
WORLD1 = ([-25.0, -25.0, -25.0], [25.0, 25.0, 25.0])       # some 100 MeV muons leave it (range 31 cm), most walks stop inside


def mixed_primaries(n=N1, seed=SEED1):
    """muons of both signs and protons, 30 .. 100 MeV log-uniform, isotropic, 8 tracks per event, from a point off the centre"""
    prim = TG.gun_primaries(13, [3.0, -4.0, 5.0], None, (30.0, 100.0), 8, (n + 7) // 8, seed)[:n]
    prim["pdg"] = np.array([13, -13, 2212, 13])[np.arange(n) % 4]
    prim["time"] = 0.25 * (np.arange(n) // 8)
    return prim


def params1():
    return TG.params(world=WORLD1)


def compare(got, exp, what, tol=1e-6):
    """primaries that differ in segment count or end state (returned), and every column of the others within ``tol`` cm / MeV
    (times: ``tol`` relative to their magnitude)"""
    n = len(exp["counts"])
    differ = (np.asarray(got["counts"]) != np.asarray(exp["counts"])) | (np.asarray(got["end_state"]) != np.asarray(exp["end_state"]))
    print(f"{what}: {int(differ.sum())} of {n} primaries differ in segment count or end state")
    keep_g, keep_e = ~differ[np.asarray(got["primary"])], ~differ[np.asarray(exp["primary"])]
    assert keep_g.sum() == keep_e.sum()
    worst = {}
    for k in TG.F64_COLUMNS:
        a, b = np.asarray(got[k], dtype=np.float64)[keep_g], np.asarray(exp[k], dtype=np.float64)[keep_e]
        scale = np.maximum(np.abs(b), 1e-300) if k in ("t_start", "t_end", "t") else 1.0
        worst[k] = float(np.max(np.abs(a - b) / scale)) if len(a) else 0.0
    print(f"{what}: largest deviations " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k in ("primary", "step", "pdg_id", "event_id"):
        assert np.array_equal(np.asarray(got[k])[keep_g], np.asarray(exp[k])[keep_e]), (what, k)
    same = ~differ
    for k, scale in (("end_pos", 1.0), ("path", 1.0), ("end_energy", 1.0)):
        assert np.max(np.abs(np.asarray(got[k], dtype=np.float64)[same] - np.asarray(exp[k], dtype=np.float64)[same])) <= tol, (what, k)
    assert max(worst.values()) <= tol, (what, worst)
    return int(differ.sum())


def twin_self_check(seed=SEED1, n=N1):
    """the twin in f64 against itself in longdouble: the number of primaries whose walk hangs on a comparison's last bit"""
    prim, p = mixed_primaries(n, seed), params1()
    return compare(TG.generate_twin(prim, p, seed), TG.generate_twin(prim, p, seed, float_type=np.longdouble),
                   f"seed {seed}: twin f64 against longdouble")
