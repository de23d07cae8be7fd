"""CPU: the track cascade's host side (larndsim_amd/track_cascade.py, cli/generate_segments.py --secondaries) -- struct layouts
against the header text, the Moller formulas against ones written out here and against quadratures, the two samplers' distributions,
energy accounting over the generations, the delta-ray rate, the emission kinematics, the decays, the independence of a family from
the rest of its list, the datasets through the driver's own readers, the refusals.  No GPU call.

Bounds.  Formulas: the same f64 expression, only log rounding differs: rtol 1e-12; quadratures: rtol 1e-9 (scipy's own estimate is
below 1e-12).  Kolmogorov-Smirnov: 1.63 / sqrt(n), the 1 % point, at a fixed seed.  Monte Carlo: 5 standard errors of the sample.
Energy: sums of some thousand f64 terms of at most 300 MeV: 1e-9 MeV.  Kinematics: a dozen f64 operations on unit vectors: 1e-12."""
import ctypes as C
import functools
import importlib.util
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.integrate import quad

import helpers as H
import track_cascade_cases as CC
from larndsim_amd import abi, consts, lib, rng, track_cascade as TC, track_generator as TG

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "larnd-sim_amd", "cli", "generate_segments.py")
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")
BIG = ([-1e4] * 3, [1e4] * 3)
CTYPE = {"double": C.c_double, "int32_t": C.c_int32, "uint64_t": C.c_uint64}
ME, K, ZA, I_EXC = 0.51099895, 0.307075, 18.0 / 39.948, 188e-6


@pytest.fixture(autouse=True)
def _cfg():
    H.load_cfg("module0")


def _struct_fields(name):
    hdr = open(os.path.join(REPO, "include", "ldsim.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, flags=re.S).group(1)
    offsets = [int(v) for v in re.findall(r"/\* (?:offset )?(\d+)(?! bytes)[: ]", body)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", rest.strip())
            out.append((m.group(1), CTYPE[ctype] * int(m.group(2)) if m.group(2) else CTYPE[ctype]))
    return out, offsets


def test_struct_layouts_match_the_header():
    """1. sizes, offsets (the header's own comments, ctypes and numpy), entries, constants; the ABI version stays 8"""
    for name, cls, size in (("LdsimTrackGenParticle", abi.LdsimTrackGenParticle, 104),
                            ("LdsimTrackGenCascadeParams", abi.LdsimTrackGenCascadeParams, 48)):
        fields, offsets = _struct_fields(name)
        assert [f for f, _ in fields] == [f for f, _ in cls._fields_], name
        for (f, t), (_, mine) in zip(fields, cls._fields_):
            if hasattr(t, "_length_"):
                assert (t._length_, t._type_) == (mine._length_, mine._type_), (name, f)
            else:
                assert t is mine, (name, f)
        assert C.sizeof(cls) == size
        assert [getattr(cls, f).offset for f, _ in cls._fields_] == offsets, name
    q = abi.LdsimTrackGenParticle
    assert [getattr(q, f).offset for f, _ in q._fields_] == [0, 24, 48, 56, 64, 68, 72, 76, 80, 88, 92, 96, 100]
    assert TC.particle_dtype.itemsize == 104
    assert [TC.particle_dtype.fields[f][1] for f, _ in q._fields_] == [getattr(q, f).offset for f, _ in q._fields_]
    assert C.sizeof(abi.LdsimTrackGenParams) == 192 and C.sizeof(abi.LdsimTrackGenPrimary) == 80
    hdr = open(os.path.join(REPO, "include", "ldsim.h")).read()
    for entry in ("ldsim_track_cascade_count", "ldsim_track_cascade", "ldsim_track_cascade_ms"):
        assert re.search(r"\bint " + entry + r"\(ldsim_ctx\* ctx", hdr), entry
        assert entry in lib.EXPORTS and hasattr(lib.load(), entry)
    assert "ldsim_track_cascade_particles" in lib.EXPORTS and "int ldsim_track_cascade_particles(" in hdr
    for name, value in (("MOLLER_TRIES", TC.MOLLER_TRIES), ("MICHEL_NEWTON", TC.MICHEL_NEWTON), ("DRAW_AZIMUTH", TC.DRAW_AZIMUTH),
                        ("DRAW_PLACE", TC.DRAW_PLACE), ("DRAW_MOLLER", TC.DRAW_MOLLER), ("DECAY_KEY", TC.DECAY_KEY),
                        ("NF64", 15), ("NI32", 4)):
        m = re.search(r"#define LDSIM_TRACK_GEN_" + name + r" (\S+)", hdr)
        assert m and float(m.group(1)) == value, name
    # the draws fit in the 128 a step owns, and no two uses share one
    used = [0, 1, 2, 3, 4]
    for j in range(TG.HARD_CAP):
        used += [8 + 8 * j + k for k in range(8)] + [TC.DRAW_MOLLER + 5 * j + k for k in range(5)]
        used += [TC.DRAW_AZIMUTH + j, TC.DRAW_PLACE + j]
    assert len(set(used)) == len(used) and max(used) < 4 * TG.STEP_BLOCKS
    # generation 0 by the library's helper (host only) and by the module
    prim = TG.gun_primaries(13, [0, 0, 0], None, 100.0, 4, 3, 5, event_id0=7)
    got = np.zeros(len(prim), dtype=TC.particle_dtype)
    assert lib.load().ldsim_track_cascade_particles(lib.ptr(prim), C.c_int64(len(prim)), lib.ptr(got)) == 0
    assert got.tobytes() == TC.particles(prim).tobytes()
    assert lib.load().ldsim_abi_version() == abi.ABI_VERSION == 8
    assert "#define LDSIM_ABI_VERSION 8" in hdr


# ---- the Moller formulas, written out independently -----------------------------------------------------------------------------
def _delta(bg):
    x = math.log10(bg)
    if x >= 3.0:
        return 2 * math.log(10) * x - 5.2146
    if x >= 0.2:
        return 2 * math.log(10) * x - 5.2146 + 0.19559 * (3.0 - x) ** 3.0
    return 0.0


def _moller_restricted(T, tc):
    """restricted electron stopping power, MeV cm^2 / g (ICRU 37, eq. for collisions below tc <= T / 2)"""
    tau = T / ME
    gamma = tau + 1
    beta2 = 1 - 1 / gamma ** 2
    d = min(tc, T / 2) / ME
    e = I_EXC / ME
    br = (math.log(2 * (tau + 2) / e ** 2) - 1 - beta2 + math.log((tau - d) * d) + tau / (tau - d)
          + (d * d / 2 + (2 * tau + 1) * math.log(1 - d / tau)) / gamma ** 2 - _delta(math.sqrt(gamma ** 2 - 1)))
    return K / 2 * ZA / beta2 * br


def _moller_dsigma(eps, T):
    """Moller collisions per (g / cm^2) and MeV"""
    gamma = T / ME + 1
    beta2 = 1 - 1 / gamma ** 2
    g = (2 * gamma - 1) / gamma ** 2
    x = eps / T
    return K / 2 * ZA / beta2 / T ** 2 * (1 / x ** 2 + 1 / (1 - x) ** 2 + (1 - g) - g / (x * (1 - x)))


def test_moller_formulas():
    """2. the stopping power against the formula written out here (rtol 1e-12) and the header's anchor values (1e-3); restricted loss +
    the quadrature of eps dsigma over [t_cut, T / 2] = the unrestricted loss (1e-9); lambda against the quadrature of dsigma"""
    p = TG.params(world=BIG)
    rho, t_cut = p["density"], p["t_cut"]
    anchors = {1.0: 1.369, 5.0: 1.473, 10.0: 1.555, 50.0: 1.718}
    for T in (0.5, 1.0, 5.0, 10.0, 50.0):
        full = float(TC.moller_stopping_power(T, p))
        assert abs(full / _moller_restricted(T, T / 2) - 1) <= 1e-12, T
        restricted = float(TC.moller_stopping_power(T, p, t_cut))
        assert abs(restricted / _moller_restricted(T, t_cut) - 1) <= 1e-12, T
        if T in anchors:
            assert abs(full / anchors[T] - 1) <= 1e-3, (T, full)
        hard = quad(lambda e: e * _moller_dsigma(e, T), t_cut, T / 2, epsabs=0, epsrel=1e-13, limit=200)[0]
        assert abs((restricted + hard) / full - 1) <= 1e-9, (T, restricted, hard, full)
        n = quad(lambda e: _moller_dsigma(e, T), t_cut, T / 2, epsabs=0, epsrel=1e-13, limit=200)[0]
        assert abs(float(TC.moller_lambda(T, 0.1, p)) / (n * rho * 0.1) - 1) <= 1e-9, T
        assert abs(float(TC.moller_lambda(T, 0.1, p, 0.2)) /
                   (quad(lambda e: _moller_dsigma(e, T), 0.2, T / 2, epsabs=0, epsrel=1e-13, limit=200)[0] * rho * 0.1) - 1) <= 1e-9
    assert float(TC.moller_stopping_power(0.5, p, t_cut)) > 0                 # t_min's own check


def _uniforms(n, seed, tries):
    """keyed uniforms [n][tries] x 2, as the kernel's draws are made (f32 in (0, 1])"""
    nb = (2 * tries + 3) // 4
    u = np.concatenate([rng.keyed_block_uniforms(seed, TG.TAG_GEN, np.arange(n, dtype=np.uint64), b) for b in range(nb)], axis=1)
    return u[:, :tries].astype(np.float64), u[:, tries:2 * tries].astype(np.float64)


def _ks(sample, cdf):
    s = np.sort(sample)
    c, n = cdf(s), len(s)
    return max(np.max(np.arange(1, n + 1) / n - c), np.max(c - np.arange(n) / n))


def test_sampler_distributions():
    """3. 2e5 Moller draws at T = 10 MeV, t_cut = 0.1 MeV and 2e5 Michel draws: Kolmogorov-Smirnov distance to the analytic CDF
    below 1.63 / sqrt(n); Moller's forced last try is never taken (the Michel x is an inversion and has none); the Michel mean is 0.7"""
    n, T, t_cut = 200_000, 10.0, 0.1
    ue, ua = _uniforms(n, 31, TC.MOLLER_TRIES)
    th, kept = TC.sample_moller(ue, ua, np.full(n, T), t_cut)
    gamma = T / ME + 1
    g = (2 * gamma - 1) / gamma ** 2

    def prim(x):
        return -1 / x + 1 / (1 - x) + (1 - g) * x - g * np.log(x / (1 - x))
    x0 = t_cut / T
    dist = _ks(th / T, lambda x: (prim(x) - prim(x0)) / (prim(0.5) - prim(x0)))
    print(f"Moller: KS distance {dist:.2e}, bound {1.63 / math.sqrt(n):.2e}; tries used: {np.bincount(kept, minlength=TC.MOLLER_TRIES)}")
    assert dist <= 1.63 / math.sqrt(n)
    assert (kept < TC.MOLLER_TRIES - 1).all() and th.min() >= t_cut * (1 - 1e-12) and th.max() <= T / 2
    u = _uniforms(n, 32, 1)[0][:, 0]
    x = TC.sample_michel(u)
    dist = _ks(x, lambda v: 2 * v ** 3 - v ** 4)
    print(f"Michel: KS distance {dist:.2e}; mean {x.mean():.5f}")
    assert dist <= 1.63 / math.sqrt(n)
    assert np.abs(2 * x ** 3 - x ** 4 - u).max() <= 1e-15 and x.min() > 0 and x.max() <= 1      # (an inversion: no try is forced)
    assert abs(x.mean() - 0.7) <= 5 * x.std(ddof=1) / math.sqrt(n)


def _family_sums(gens):
    """(summed dE, summed kinetic energy of the decay electrons) per generation-0 particle"""
    n = len(gens[0]["particles"])
    dE, dec = np.zeros(n), np.zeros(n)
    for g, r in zip(gens, TC.ancestors(gens)):
        dE += np.bincount(r[g["primary"]], weights=np.asarray(g["dE"], dtype=np.float64), minlength=n)
        d = g["particles"]["process"] == TC.DECAY
        dec += np.bincount(r[d], weights=g["particles"]["kinetic_energy"][d], minlength=n)
    return dE, dec


def test_energy_is_conserved_whatever_the_cap():
    """4. 64 stopping muons of 300 MeV and 64 electrons of 5 MeV in a box nothing leaves, t_track 0.5 MeV: every family's dE adds
    up to T0 within 1e-9 MeV at max_generations 1, 2 and 4; at 1 the muons' segments are generate_twin's, bit for bit; with
    decays the sum is T0 plus the decay electrons' kinetic energies"""
    p = TG.params(world=BIG)
    mu = TG.primaries(np.where(np.arange(64) % 2, 13, -13), [0, 0, 0], [0, 0, 1], 300.0, event_id=np.arange(64))
    el = TG.primaries(np.where(np.arange(64) % 2, 11, -11), [0, 0, 0], [0, 0, 1], 5.0, event_id=np.arange(64), track_in_event=1)
    for prim, T0 in ((mu, 300.0), (el, 5.0)):
        sizes = {}
        for mg in (1, 2, 4):
            gens = TC.cascade_twin(prim, p, TC.cascade_params(t_track=0.5, max_generations=mg), 5)
            dE, _ = _family_sums(gens)
            sizes[mg] = [len(g["particles"]) for g in gens]
            assert len(gens) <= mg and np.abs(dE - T0).max() <= 1e-9, (T0, mg, np.abs(dE - T0).max())
            assert all((g["end_state"] == TG.STOPPED).all() for g in gens)
            assert len(gens[-1]["secondaries"]) == 0
            if mg == 1 and T0 == 300.0:
                ref = TG.generate_twin(prim, p, 5)
                assert len(gens) == 1 and all(np.asarray(ref[k]).tobytes() == np.asarray(gens[0][k]).tobytes() for k in ref)
        print(f"T0 {T0} MeV: particles per generation {sizes}")
        assert sizes[1] == [64] and len(sizes[4]) >= 2 and sizes[2][1] > 0
    gens = TC.cascade_twin(mu, p, TC.cascade_params(t_track=0.5, max_generations=4, decays=True), 5)
    dE, dec = _family_sums(gens)
    assert (dec > 0).sum() >= 32 and np.abs(dE - (300.0 + dec)).max() <= 1e-9       # (every mu+ decays)
    assert (dec[1::2] > 0).sum() < 32                                              # (most mu- are captured)


def test_delta_ray_rate():
    """5. 2e4 single steps of a 1 GeV muon: the emitted secondaries are Poisson of mean lambda(t_track) N, segment dE + emitted
    energy averages S rho h, every emitted T_h >= t_track"""
    n, h, tt = 20_000, 0.1, 1.0
    p = TG.params(world=BIG, step=h, max_steps=1, mcs=False)
    part = TC.particles(TG.primaries(13, [0, 0, 0], [0, 0, 1], 1000.0, event_id=np.arange(n)))
    g = TC.walk_generation_twin(part, p, TC.cascade_params(t_track=tt), 11)
    sec = g["secondaries"]
    Tm = 1000.0 - 0.5 * float(TG.stopping_power(1000.0, 13, p)) * p["density"] * h
    M = TG.MASSES[13]
    gamma = Tm / M + 1
    beta2 = 1 - 1 / gamma ** 2
    tmax = float(TG.tmax(Tm, 13))
    xi = 0.5 * K * ZA * p["density"] * h / beta2
    lam = xi * ((1 / tt - 1 / tmax) - beta2 / tmax * math.log(tmax / tt))
    print(f"{len(sec)} delta rays, expected {lam * n:.1f} +- {math.sqrt(lam * n):.1f}")
    assert abs(len(sec) - lam * n) <= 5 * math.sqrt(lam * n)
    assert (sec["kinetic_energy"] >= tt).all() and (sec["pdg"] == 11).all() and (sec["process"] == TC.DELTA_RAY).all()
    total = g["dE"] + np.bincount(sec["parent"], weights=sec["kinetic_energy"], minlength=n)
    want = float(TG.stopping_power(Tm, 13, p)) * p["density"] * h
    se = total.std(ddof=1) / math.sqrt(n)
    print(f"mean loss {total.mean():.6f} MeV, Bethe {want:.6f} MeV, standard error {se:.6f} MeV")
    assert abs(total.mean() - want) <= 5 * se
    assert np.array_equal(g["secondary_counts"], np.bincount(sec["parent"], minlength=n))
    # below t_track the collisions are deposited as before: with no threshold reached the segments are generate_twin's
    quiet = TC.walk_generation_twin(part[:2000], p, TC.cascade_params(t_track=900.0), 11)
    ref = TG.generate_twin(TG.primaries(13, [0, 0, 0], [0, 0, 1], 1000.0, event_id=np.arange(2000)), p, 11)
    assert len(quiet["secondaries"]) == 0 and quiet["dE"].tobytes() == ref["dE"].tobytes()


def test_emission_kinematics():
    """6. every secondary of a 256-muon run: the angle against the parent's direction, the unit direction, the origin on the
    parent's segment, the time inside it, the links"""
    p = TG.params(world=([-20.0] * 3, [20.0] * 3))
    part = TC.particles(TG.gun_primaries(13, [1.0, 2.0, 3.0], None, (50.0, 400.0), 8, 32, 3))
    g = TC.walk_generation_twin(part, p, TC.cascade_params(t_track=0.5), 3)
    sec = g["secondaries"]
    assert len(sec) > 500 and set(np.unique(g["end_state"])) == {TG.STOPPED, TG.EXITED}
    d = sec["dir"]
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1).max() <= 1e-12
    Tm, th, M = g["sec_parent_tm"], sec["kinetic_energy"], TG.MASSES[13]
    want = np.minimum(th * (Tm + M + ME) / (np.sqrt(Tm * (Tm + 2 * M)) * np.sqrt(th * (th + 2 * ME))), 1.0)
    assert np.abs((d * g["sec_parent_dir"]).sum(axis=1) - want).max() <= 1e-12
    assert (want > 0.3).all() and (want < 1).all()
    first = np.concatenate([[0], np.cumsum(g["counts"])])
    row = first[sec["parent"]] + sec["parent_step"]
    # the midpoint energy itself, from the file's own columns: T at a step's start is T0 less what the earlier steps deposited and
    # emitted, Tm = T - S(T) rho h / 2 with h the segment's length (a stopping segment is shortened afterwards: left out).  Some
    # thousand terms of at most 400 MeV sum to within 4000 ulp(400) = 2e-10 MeV, and cos theta moves by less than 0.1 / MeV: 1e-9
    lost = g["dE"] + np.bincount(row, weights=th, minlength=len(g["dE"]))
    T_start = np.concatenate([part["kinetic_energy"][i] - (np.cumsum(lost[a:b]) - lost[a:b])
                              for i, (a, b) in enumerate(zip(first[:-1], first[1:]))])
    going = np.ones(len(g["dE"]), dtype=bool)
    going[first[1:][g["end_state"] == TG.STOPPED] - 1] = False
    keep = going[row]
    Ts = T_start[row][keep]
    Tm_own = np.maximum(Ts - 0.5 * TG.stopping_power(Ts, 13, p) * p["density"] * g["dx"][row][keep], p["t_min"])
    assert keep.sum() > 500 and (sec["parent_step"][keep] == 0).sum() >= 1
    assert np.abs(Tm_own - Tm[keep]).max() <= 1e-9
    own = np.minimum(th[keep] * (Tm_own + M + ME) / (np.sqrt(Tm_own * (Tm_own + 2 * M)) * np.sqrt(th[keep] * (th[keep] + 2 * ME))), 1.0)
    assert np.abs((d * g["sec_parent_dir"]).sum(axis=1)[keep] - own).max() <= 1e-9
    assert np.array_equal(g["primary"][row], sec["parent"]) and np.array_equal(g["step"][row], sec["parent_step"])
    a = np.stack([g[k + "_start"][row] for k in "xyz"], axis=1)
    b = np.stack([g[k + "_end"][row] for k in "xyz"], axis=1)
    ab, ap = b - a, sec["pos"] - a
    L = np.sqrt((ab * ab).sum(axis=1))
    assert (np.sqrt((np.cross(ap, ab) ** 2).sum(axis=1)) / L).max() <= 1e-12
    u = (ap * ab).sum(axis=1) / (L * L)
    assert u.min() >= 0 and u.max() <= 1 and 0.4 < u.mean() < 0.6
    assert (sec["time"] >= g["t_start"][row]).all() and (sec["time"] <= g["t_end"][row]).all()
    # the parent's segment follows the direction the secondary was turned against (the collision does not deflect the parent)
    straight = L > 0
    assert np.abs(ab[straight] / L[straight, None] - g["sec_parent_dir"][straight]).max() <= 1e-9
    assert (sec["generation"] == 1).all() and (sec["process"] == TC.DELTA_RAY).all() and (sec["pdg"] == 11).all()
    assert np.array_equal(sec["event_id"], part["event_id"][sec["parent"]])
    assert np.array_equal(sec["track_in_event"], part["track_in_event"][sec["parent"]])
    assert np.all(np.diff(sec["parent"]) >= 0) and len(np.unique(sec["key"])) == len(sec)
    same = np.diff(sec["parent"]) == 0
    assert np.all(np.diff(sec["parent_step"])[same] >= 0)


def test_decays():
    """7. 2e4 stopped muons of each sign: every mu+ decays, the mu- share is 1 - capture_fraction, the delays average the
    lifetimes, the directions are isotropic; a muon that left the box, a pion and a proton emit nothing"""
    n = 20_000
    p = TG.params(world=BIG)
    cp = TC.cascade_params(decays=True, delta_tracks=False)
    for pdg, life, share in ((-13, cp["mu_plus_lifetime"], 1.0), (13, cp["mu_minus_lifetime"], 1 - cp["capture_fraction"])):
        part = TC.particles(TG.primaries(pdg, [0, 0, 0], [0, 0, 1], 0.51, event_id=np.arange(n)))
        g = TC.walk_generation_twin(part, p, cp, 7)
        sec = g["secondaries"]
        assert (g["end_state"] == TG.STOPPED).all() and (sec["process"] == TC.DECAY).all() and (sec["pdg"] == (11 if pdg > 0 else -11)).all()
        k = len(sec)
        print(f"pdg {pdg}: {k} of {n} decay, expected share {share}")
        assert abs(k - share * n) <= 5 * math.sqrt(n * share * (1 - share))
        delay = sec["time"] - g["end_time"][sec["parent"]]
        assert abs(delay.mean() - life) <= 5 * delay.std(ddof=1) / math.sqrt(k)
        for a in range(3):
            assert abs(sec["dir"][:, a].mean()) <= 5 * sec["dir"][:, a].std(ddof=1) / math.sqrt(k)
        assert np.abs(np.sqrt((sec["dir"] ** 2).sum(axis=1)) - 1).max() <= 1e-12
        etot = sec["kinetic_energy"] + ME
        assert etot.max() <= TC.MICHEL_W and abs((etot / TC.MICHEL_W).mean() - 0.7) <= 5 * (etot / TC.MICHEL_W).std(ddof=1) / math.sqrt(k)
        assert np.array_equal(sec["pos"], g["end_pos"][sec["parent"]]) and np.array_equal(sec["parent_step"], g["counts"][sec["parent"]])
        assert g["forced_tries"] == 0
    small = TG.params(world=([-1.0] * 3, [1.0] * 3))
    others = TC.particles(TG.primaries([-13, 211, -211, 2212], [0, 0, 0], [0, 0, 1], [100.0, 0.6, 0.6, 0.6]))
    g = TC.walk_generation_twin(others, small, cp, 7)
    assert list(g["end_state"]) == [TG.EXITED, TG.STOPPED, TG.STOPPED, TG.STOPPED] and len(g["secondaries"]) == 0
    off = TC.walk_generation_twin(TC.particles(TG.primaries(-13, [0, 0, 0], [0, 0, 1], 0.51)), p, cp, 7, emit=False)
    assert len(off["secondaries"]) == 0


@functools.lru_cache(maxsize=None)
def _twin1(long=False):
    H.load_cfg("module0")
    return TC.cascade_twin(CC.mixed_particles(), CC.params1(), CC.cascade1(), CC.SEED1, float_type=np.longdouble if long else np.float64)


def _family(gens, i):
    """the family of generation-0 particle i: per generation (particles without their parent index, segment columns)"""
    out = []
    for g, r in zip(gens, TC.ancestors(gens)):
        m = r == i
        part = g["particles"][m].copy()
        part["parent"] = 0
        rows = m[g["primary"]]
        out.append((part.tobytes(), [np.asarray(g[k])[rows].tobytes() for k in TG.F64_COLUMNS + ("step", "pdg_id", "event_id")],
                    np.asarray(g["counts"])[m].tobytes(), np.asarray(g["end_state"])[m].tobytes()))
    return out


def test_a_family_does_not_depend_on_its_list():
    """8. a family walked alone is the family inside a list of 200, bit for bit; the f64 and the longdouble twin agree on every
    count of every generation, and on the secondaries' floats to 1e-12, for the GPU test's input and seed"""
    part, p, cp = CC.mixed_particles(200), CC.params1(), CC.cascade1()
    gens = TC.cascade_twin(part, p, cp, CC.SEED1)
    assert len(gens) == 3
    for i in (0, 37, 75, 199):                                           # a mu-, a mu+, an e-, an e+
        alone = TC.cascade_twin(part[i:i + 1], p, cp, CC.SEED1)
        fam = _family(gens, i)
        fam = [f for f in fam if len(f[0])]
        assert len(alone) == len(fam) and _family(alone, 0) == fam, i
    a, b = _twin1(), _twin1(True)
    bad = CC.same_counts(a, b)
    print(f"seed {CC.SEED1}: {int(bad.sum())} of {CC.N1} families differ between f64 and longdouble; particles per generation "
          f"{[len(g['particles']) for g in a]}")
    assert bad.sum() == 0
    dev = CC.secondary_deviation(a, b)
    print("secondaries, f64 against longdouble: " + "; ".join(", ".join(f"{f} {v:.1e}" for f, v in w.items()) for w in dev))
    assert max(max(w.values()) for w in dev) <= 1e-12
    kinds = set(np.unique(a[0]["particles"]["pdg"]))
    assert kinds == {11, -11, 13, -13, 2212} and set(np.unique(a[0]["end_state"])) == {TG.STOPPED, TG.EXITED}
    assert (a[1]["particles"]["process"] == TC.DECAY).sum() > 20 and sum(g["forced_tries"] for g in a) == 0


def _sp_cli():
    spec = importlib.util.spec_from_file_location("sp_cli_track_cascade", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _tool(*args):
    return subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True)


def test_file_surface(tmp_path):
    """9. to_datasets' links; the --twin tool's file through the driver's readers; --pdg 11 with --secondaries; the tool without
    --secondaries writes what it wrote before"""
    gens = _twin1()
    seg, traj, vert = TC.to_datasets(gens)
    n = [len(g["particles"]) for g in gens]
    assert len(traj) == sum(n) and np.array_equal(traj["traj_id"], np.arange(len(traj))) and len(vert) == CC.N1 // 8
    assert (traj["parent_id"][:n[0]] == -1).all() and traj["primary"][:n[0]].all() and not traj["primary"][n[0]:].any()
    child = traj[n[0]:]
    assert (child["parent_id"] >= 0).all() and (child["parent_id"] < child["traj_id"]).all()
    assert np.array_equal(traj["event_id"][child["parent_id"]], child["event_id"])
    assert np.array_equal(traj["vertex_id"][child["parent_id"]], child["vertex_id"])
    assert (traj["parent_id"][n[0]:n[0] + n[1]] < n[0]).all() and (traj["parent_id"][n[0] + n[1]:] >= n[0]).all()
    assert np.array_equal(np.bincount(seg["traj_id"], minlength=len(traj)), traj["n_segments"])
    assert np.array_equal(traj["event_id"][seg["traj_id"]], seg["event_id"]) and np.array_equal(seg["segment_id"], np.arange(len(seg)))
    assert np.all(np.diff(seg["vertex_id"].astype(np.int64)) >= 0)                   # an event's segments are contiguous
    assert np.array_equal(vert["event_id"][seg["vertex_id"]], seg["event_id"])
    el = np.abs(traj["pdg_id"]) == 11
    np.testing.assert_allclose(traj["E_start"][el], np.concatenate([g["particles"]["kinetic_energy"] for g in gens])[el] + ME, rtol=1e-6)
    b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)
    c = b[0].mean(axis=1)
    where = ["--position", str(c[2]), str(c[1]), str(c[0]), "--isotropic", "--tracks_per_event", "3", "--n_events", "2", "--seed", "4"]
    out = str(tmp_path / "cascade.npz")
    r = _tool("--config", "module0", "--source", "gun", "--pdg", "-13", "--energy", "40", *where, "--secondaries", "--decays",
              "--t_track", "0.5", "--twin", "--output", out)
    assert r.returncode == 0, r.stderr
    assert "6 primaries in 2 events" in r.stdout and "6 decay electrons" in r.stdout
    cli = _sp_cli()
    H.load_cfg("module0")
    seg, truth = cli.load_input(out)
    traj, vert = truth["trajectories"], truth["vertices"]
    assert len(vert) == 2 and list(vert["n_primaries"]) == [3, 3] and traj["primary"].sum() == 6 and len(traj) > 12
    assert (traj["pdg_id"][~traj["primary"]] != -13).all() and ((traj["pdg_id"] == -11).sum() == 6)
    assert np.array_equal(np.bincount(seg["traj_id"], minlength=len(traj)), traj["n_segments"])
    assert np.all(np.diff(seg["event_id"].astype(np.int64)) >= 0)
    dec = traj[traj["pdg_id"] == -11]
    want = 6 * 40.0 + float((dec["E_start"].astype(np.float64) - ME).sum())
    assert abs(float(seg["dE"].astype(np.float64).sum()) - want) < 1e-2                 # f4 columns
    tracks = cli.prepare_tracks(seg.copy())
    assert len(tracks) == len(seg)
    cli.attach_event_times(truth, np.array([10.0, 20.0]), consts.sim)
    assert list(truth["vertices"]["t_event"]) == [10.0, 20.0]
    r = _tool("--source", "gun", "--pdg", "11", "--energy", "5", *where, "--secondaries", "--twin", "--output", str(tmp_path / "e.npz"))
    assert r.returncode == 0 and "6 primaries in 2 events" in r.stdout, r.stderr
    with np.load(tmp_path / "e.npz") as f:
        assert (f["trajectories"]["pdg_id"] == 11).all() and abs(float(f["segments"]["dE"].astype(np.float64).sum()) - 30.0) < 1e-3
    # without --secondaries: the existing test's command line, the arrays of track_generator.to_datasets(generate_twin)
    r = _tool("--config", "module0", "--source", "gun", "--pdg", "13", "--energy", "40", *where, "--twin", "--output",
              str(tmp_path / "plain.npz"))
    assert r.returncode == 0 and "6 stopped, 0 left the world box, 0 truncated" in r.stdout
    H.load_cfg("module0")
    prim = TG.gun_primaries(13, [float(c[2]), float(c[1]), float(c[0])], None, 40.0, 3, 2, 4)
    ref = TG.to_datasets(prim, TG.generate_twin(prim, TG.params(TG.default_world(10.0), min_step=1e-4), 4))
    with np.load(tmp_path / "plain.npz") as f:
        for name, want in zip(("segments", "trajectories", "vertices"), ref):
            assert f[name].dtype == want.dtype and all(np.array_equal(f[name][k], want[k]) for k in want.dtype.names), name
    for extra in (["--pdg", "11"], ["--pdg", "-11"]):
        bad = _tool("--source", "gun", *extra, "--twin", "--output", str(tmp_path / "bad.npz"))
        assert bad.returncode == 2 and "unknown pdg" in bad.stderr
    assert _tool("--source", "gun", "--decays", "--twin", "--output", str(tmp_path / "bad.npz")).returncode == 2


def test_refusals_name_what_is_wrong():
    """10. the Python layer refuses what the C-ABI refuses"""
    p = TG.params(world=([0, 0, 0], [10, 10, 10]))
    ok = dict(pdg=11, pos=[5, 5, 5], direction=[0, 0, 1], kinetic_energy=5.0)
    one = TC.particles(TG.primaries(**ok))
    assert len(TC.walk_generation_twin(one, p, TC.cascade_params(), 0)["dx"]) > 5
    inf, nan = math.inf, math.nan
    for kw, what in (({"t_track": 0.05}, "t_track"), ({"t_track": 0.3}, "t_track"), ({"t_track": nan}, "t_track"),
                     ({"t_track": inf}, "t_track"), ({"capture_fraction": -0.1}, "capture_fraction"),
                     ({"capture_fraction": 1.5}, "capture_fraction"), ({"capture_fraction": nan}, "capture_fraction"),
                     ({"mu_plus_lifetime": 0.0}, "mu_plus_lifetime"), ({"mu_minus_lifetime": -1.0}, "mu_minus_lifetime"),
                     ({"mu_minus_lifetime": inf}, "mu_minus_lifetime"), ({"max_generations": 0}, "max_generations")):
        with pytest.raises(TG.TrackGenError, match=what):
            TC.cascade_twin(one, p, TC.cascade_params(**kw), 0)
    low = dict(p, t_min=0.25, t_cut=0.2)                                  # (t_track may go down with both)
    assert len(TC.cascade_twin(one, low, TC.cascade_params(t_track=0.25), 0)) >= 1
    with pytest.raises(TG.TrackGenError, match="stopping power"):
        TC.cascade_twin(one, dict(p, t_min=0.01), TC.cascade_params(), 0)
    with pytest.raises(TG.TrackGenError, match="step"):
        TC.cascade_twin(one, dict(p, step=0.0), TC.cascade_params(), 0)
    for kw, what in (({"pdg": 22}, "unknown pdg 22"), ({"pdg": -2212}, "unknown pdg -2212"), ({"pos": [5, 5, 11]}, "outside the world box"),
                     ({"pos": [nan, 5, 5]}, "outside the world box"), ({"direction": [0, 0, 0]}, "zero direction"),
                     ({"kinetic_energy": 0.0}, "kinetic energy"), ({"kinetic_energy": inf}, "kinetic energy"), ({"time": inf}, "time")):
        bad = np.concatenate([one, TC.particles(TG.primaries(**dict(ok, **kw)))])
        with pytest.raises(TG.TrackGenError, match=what) as e:
            TC.walk_generation_twin(bad, p, TC.cascade_params(), 0)
        assert "particle 1" in str(e.value)
    with pytest.raises(TG.TrackGenError, match="unknown pdg 11"):        # the old entries' refusal stays
        TG.generate_twin(TG.primaries(**ok), p, 0)
