"""Inputs shared by the track cascade's tests and tools (not a test module)."""
import numpy as np

from larndsim_amd import track_cascade as TC, track_generator as TG

# test 1 of tests/test_gpu_track_cascade.py: 512 generation-0 particles of mixed kinds.  SEED1 is a seed for which the numpy twin
# in f64 and in longdouble agree on every particle's segment count, secondary count and end state in every generation and on
# every secondary's pos, dir, kinetic_energy and time to 1e-12 (found on the host: seeds 20250201, 20250202, .. tried in order,
# the first that passes taken; test 8 of tests/test_cpu_track_cascade.py repeats the check).  The second condition matters: a
# secondary inherits its parent's place and direction, and the scattering rotation loses digits where a direction comes close
# to the z axis (1 - dz^2 cancels) -- at 20250201 the two twins agree on every count, but one electron's secondaries are
# 4.6e-12 apart, which no kernel could then match to 1e-12.
N1 = 512
SEED1 = 20250202
WORLD1 = ([-30.0, -30.0, -30.0], [30.0, 30.0, 30.0])       # 60 cm: muons above some 130 MeV leave it


def mixed_particles(n=N1, seed=SEED1):
    """mu+- of 30 .. 300 MeV, protons of 50 .. 150 MeV, e+- of 2 .. 20 MeV (log-uniform), isotropic, 8 tracks per event"""
    ne = (n + 7) // 8
    mu = TG.gun_primaries(13, [3.0, -4.0, 5.0], None, (30.0, 300.0), 8, ne, seed)[:n]
    pr = TG.gun_primaries(2212, [3.0, -4.0, 5.0], None, (50.0, 150.0), 8, ne, seed)[:n]
    el = TG.gun_primaries(11, [3.0, -4.0, 5.0], None, (2.0, 20.0), 8, ne, seed)[:n]
    kind = np.arange(n) % 8                                 # mu- mu+ p e- mu- mu+ p e+
    prim = mu.copy()
    prim[kind % 4 == 2] = pr[kind % 4 == 2]
    prim[kind % 4 == 3] = el[kind % 4 == 3]
    prim["pdg"] = np.array([13, -13, 2212, 11, 13, -13, 2212, -11])[kind]
    prim["time"] = 0.25 * (np.arange(n) // 8)
    return TC.particles(prim)


def params1():
    return TG.params(world=WORLD1, step=0.1)


def cascade1():
    return TC.cascade_params(t_track=0.5, decays=True, max_generations=3)


def same_counts(a, b):
    """families (generation-0 ancestors) in which two cascades differ in a count, an end state or a secondary's integer field"""
    n = len(a[0]["particles"])
    bad = np.zeros(n, dtype=bool)
    ra, rb = TC.ancestors(a), TC.ancestors(b)
    if len(a) != len(b):
        return ~bad
    for k in range(len(a)):
        ga, gb = a[k], b[k]
        if len(ga["particles"]) != len(gb["particles"]):    # (the generations no longer line up: nothing can be matched)
            return ~bad
        for key in ("counts", "secondary_counts", "end_state"):
            bad[ra[k][np.asarray(ga[key]) != np.asarray(gb[key])]] = True
        for key in ("pdg", "event_id", "track_in_event", "parent", "generation", "process", "parent_step", "key"):
            bad[ra[k][ga["particles"][key] != gb["particles"][key]]] = True
    return bad


def secondary_deviation(a, b):
    """largest absolute deviation of a secondary's pos (cm), dir, kinetic_energy (MeV) and time (us) between two cascades with
    the same counts, per generation"""
    out = []
    for ga, gb in zip(a, b):
        sa, sb = ga["secondaries"], gb["secondaries"]
        worst = {}
        for f in ("pos", "dir", "kinetic_energy", "time"):
            worst[f] = float(np.max(np.abs(sa[f] - sb[f]))) if len(sa) else 0.0
        out.append(worst)
    return out
