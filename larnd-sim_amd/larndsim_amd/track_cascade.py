"""Track cascade: delta rays, electrons and muon decays as tracks of their own (csrc/kernels_trackgen.hip gen_step<true>,
cas_kernel; include/ldsim.h "track cascade" states the model).

The track generator's walk with three additions: electrons (pdg +-11) are transported under Moller loss and collisions; hard
collisions from ``t_track`` on leave the parent's segment as electrons of their own; a stopped muon decays to a Michel electron.
What a walk emits is walked in turn, generation by generation.  Units and frame are ``track_generator``'s.

* ``cascade_params``: the cascade's switches (``LdsimTrackGenCascadeParams``); the walk's parameters are ``track_generator.params``.
* ``particles``: generation 0 (``LdsimTrackGenParticle`` records) from ``track_generator.primaries`` output.
* ``walk_generation`` / ``walk_generation_twin``: one generation on the GPU (``ldsim_track_cascade``) / in numpy, operation for
  operation in f64.
* ``cascade`` / ``cascade_twin``: the loop over generations on the host; the last generation walks with emission off.
* ``moller_stopping_power`` / ``moller_lambda``: the electron model's building blocks.
* ``to_datasets``: ``segments`` (events contiguous), ``trajectories`` (one row per particle, with parent links), ``vertices``.
"""
import ctypes as C
import math

import numpy as np

from . import rng as R
from . import track_generator as TG
from .track_generator import (C_LIGHT, ELECTRON_MASS, EXITED, F64_COLUMNS, HARD_CAP, HARD_TRIES, I32_COLUMNS, STEP_BLOCKS, STOPPED,
                              TAG_GEN, TRUNCATED, TWO_PI, TrackGenError)

MUON_MASS = TG.MASSES[13]
MOLLER_TRIES, MICHEL_NEWTON = 7, 8                          # include/ldsim.h LDSIM_TRACK_GEN_MOLLER_TRIES / _MICHEL_NEWTON
DRAW_AZIMUTH, DRAW_PLACE, DRAW_MOLLER = 72, 80, 88          # include/ldsim.h LDSIM_TRACK_GEN_DRAW_*
DECAY_KEY = 256                                             # include/ldsim.h LDSIM_TRACK_GEN_DECAY_KEY
MICHEL_W = (MUON_MASS * MUON_MASS + ELECTRON_MASS * ELECTRON_MASS) / (2.0 * MUON_MASS)
PRIMARY, DELTA_RAY, DECAY = 0, 1, 2                         # process
PDGS = (11, -11, 13, -13, 211, -211, 2212)

particle_dtype = np.dtype(TG.primary_dtype.descr + [("key", "u8"), ("parent", "i4"), ("generation", "i4"), ("process", "i4"),
                                                    ("parent_step", "i4")])          # LdsimTrackGenParticle, 104 bytes


# ---- parameters -------------------------------------------------------------------------------------------------------------
def cascade_params(t_track=1.0, delta_tracks=True, decays=False, max_generations=4, mu_plus_lifetime=2.1969811,
                   mu_minus_lifetime=0.537, capture_fraction=0.76):
    """the cascade's switches as a dict.  ``t_track`` (MeV): hard collisions from here on become tracks; ``max_generations``: the
    loop's cap (the last one walks with emission off); ``mu_minus_lifetime`` (us) and ``capture_fraction`` are parameters of the
    argon medium, not measurements of this project"""
    return {"t_track": float(t_track), "delta_tracks": int(bool(delta_tracks)), "decays": int(bool(decays)),
            "max_generations": int(max_generations), "mu_plus_lifetime": float(mu_plus_lifetime),
            "mu_minus_lifetime": float(mu_minus_lifetime), "capture_fraction": float(capture_fraction)}


def validate(p, cp):
    """refuses what ``ldsim_track_cascade`` refuses of the parameters"""
    TG.validate(p)
    if not float(moller_stopping_power(p["t_min"], p, p["t_cut"])) > 0:
        raise TrackGenError(f"t_min {p['t_min']} MeV: the stopping power of pdg 11 is not positive there; raise t_min")
    tt = cp["t_track"]
    if not (math.isfinite(tt) and tt >= p["t_cut"] and tt >= p["t_min"]):
        raise TrackGenError(f"t_track {tt} MeV must be finite and at least t_cut {p['t_cut']} and t_min {p['t_min']}")
    if not 0 <= cp["capture_fraction"] <= 1:
        raise TrackGenError(f"capture_fraction {cp['capture_fraction']} must lie in [0, 1]")
    for k in ("mu_plus_lifetime", "mu_minus_lifetime"):
        if not TG._pos(cp[k]):
            raise TrackGenError(f"{k} {cp[k]} us must be finite and > 0")
    if cp["max_generations"] < 1:
        raise TrackGenError(f"max_generations {cp['max_generations']}: at least 1")


def particles(prim):
    """generation 0: the primaries with the stream keys the track generator gives them, parent -1, process 0"""
    prim = np.ascontiguousarray(prim, dtype=TG.primary_dtype)
    out = np.zeros(len(prim), dtype=particle_dtype)
    for k in TG.primary_dtype.names:
        out[k] = prim[k]
    out["key"] = TG.stream_keys(prim["event_id"], prim["track_in_event"])
    out["parent"], out["generation"], out["process"], out["parent_step"] = -1, 0, PRIMARY, -1
    return out


def validate_particles(part, p):
    """refuses what ``ldsim_track_cascade`` refuses of the particles"""
    part = np.ascontiguousarray(part, dtype=particle_dtype)
    lo, hi = np.array(p["world_lo"]), np.array(p["world_hi"])
    bad = np.nonzero(~np.isin(part["pdg"], PDGS))[0]
    if len(bad):
        raise TrackGenError(f"particle {bad[0]}: unknown pdg {int(part['pdg'][bad[0]])} (11, -11, 13, -13, 211, -211 and 2212 are "
                            "transported)")
    ke = part["kinetic_energy"]
    bad = np.nonzero(~(np.isfinite(ke) & (ke > 0)))[0]
    if len(bad):
        raise TrackGenError(f"particle {bad[0]}: kinetic energy {float(ke[bad[0]])} MeV must be finite and > 0")
    bad = np.nonzero(~(np.isfinite(part["pos"]) & (part["pos"] >= lo) & (part["pos"] <= hi)).all(axis=1))[0]
    if len(bad):
        raise TrackGenError(f"particle {bad[0]}: starts outside the world box, at {part['pos'][bad[0]].tolist()}")
    nn = np.sqrt((part["dir"] * part["dir"]).sum(axis=1))
    bad = np.nonzero(~(np.isfinite(nn) & (nn > 0)))[0]
    if len(bad):
        raise TrackGenError(f"particle {bad[0]}: zero direction")
    bad = np.nonzero(~np.isfinite(part["time"]))[0]
    if len(bad):
        raise TrackGenError(f"particle {bad[0]}: time is not finite")
    return part


def _pack(cp, emit):
    from .abi import LdsimTrackGenCascadeParams
    P = LdsimTrackGenCascadeParams()
    for k in ("t_track", "mu_plus_lifetime", "mu_minus_lifetime", "capture_fraction", "delta_tracks", "decays"):
        setattr(P, k, cp[k])
    P.emit = int(bool(emit))
    return P


# ---- the electron model's building blocks (f64, the kernel's operations in the kernel's order) ------------------------------------
def _mass(pdg):
    return np.where(np.abs(np.asarray(pdg, dtype=np.int64)) == 11, ELECTRON_MASS, TG._mass(pdg))


def _rate_e(bg2, beta2, gamma, T, tc, p):
    """Moller restricted stopping power in MeV / cm (gen_rate_e); tc = T / 2 gives the unrestricted ICRU-37 mean"""
    kzr = p["k_coeff"] * p["z_over_a"] * p["density"]
    i2 = p["mean_excitation"] * p["mean_excitation"]
    tau, d = T / ELECTRON_MASS, np.minimum(tc, 0.5 * T) / ELECTRON_MASS
    e2 = i2 / (ELECTRON_MASS * ELECTRON_MASS)
    return 0.5 * kzr / beta2 * (np.log(2.0 * (tau + 2.0) / e2) - 1.0 - beta2 + np.log((tau - d) * d) + tau / (tau - d)
                                + (0.5 * d * d + (2.0 * tau + 1.0) * np.log(1.0 - d / tau)) / (gamma * gamma) - TG._delta(bg2, p))


def _lambda_e(gamma, T, t_cut):
    """Moller collisions above t_cut per unit of xi (gen_lambda_e)"""
    gm = (2.0 * gamma - 1.0) / (gamma * gamma)
    x0, x1 = t_cut / T, 0.5
    return ((x1 - x0) * (1.0 - gm + 1.0 / (x0 * x1) + 1.0 / ((1.0 - x0) * (1.0 - x1)))
            - gm * np.log(x1 * (1.0 - x0) / (x0 * (1.0 - x1)))) / T


def _moller_ratio(gm, x):
    y = x * (1.0 - x)
    return 1.0 + ((1.0 - gm) * y * y - gm * y) / (1.0 - 2.0 * y)


def moller_stopping_power(T, p=None, t_cut=None):
    """electron mass stopping power of the collisions below min(t_cut, T / 2), MeV cm^2 / g; ``t_cut`` None: unrestricted"""
    p = p or TG.params()
    T = np.asarray(T, dtype=np.float64)
    bg2, beta2, gamma, _ = TG._kin(T, ELECTRON_MASS)
    return _rate_e(bg2, beta2, gamma, T, 0.5 * T if t_cut is None else np.minimum(t_cut, 0.5 * T), p) / p["density"]


def moller_lambda(T, h, p=None, t_cut=None):
    """mean number of Moller collisions above ``t_cut`` (default the parameters') in ``h`` cm at kinetic energy T > 2 t_cut"""
    p = p or TG.params()
    T = np.asarray(T, dtype=np.float64)
    _, beta2, gamma, _ = TG._kin(T, ELECTRON_MASS)
    xi = 0.5 * p["k_coeff"] * p["z_over_a"] * p["density"] * h / beta2
    return xi * _lambda_e(gamma, T, p["t_cut"] if t_cut is None else t_cut)


def _draw(seed, keys, blk, i):
    """draw i of the steps whose first block is blk"""
    return R.keyed_block_uniforms(seed, TAG_GEN, keys, np.asarray(blk, dtype=np.uint64) + np.uint64(i >> 2))[..., i & 3]


def sample_moller(ue, ua, T, t_cut):
    """the kernel's Moller sampler on given uniforms ue, ua [n][MOLLER_TRIES]: (T_h, try that was kept)"""
    T = np.asarray(T)
    gamma = T / ELECTRON_MASS + 1.0
    gm = (2.0 * gamma - 1.0) / (gamma * gamma)
    xl = t_cut / T
    g0 = (2.0 * xl - 1.0) / (xl * (1.0 - xl))
    top = np.maximum(_moller_ratio(gm, xl), _moller_ratio(gm, 0.5 + 0.0 * xl))
    th = np.zeros(ue.shape[0], dtype=ue.dtype)
    kept = np.full(ue.shape[0], -1)
    for r in range(MOLLER_TRIES):
        c = g0 * (1.0 - ue[:, r])
        x = 2.0 / ((2.0 - c) + np.sqrt(4.0 + c * c))
        ok = (kept < 0) & ((r == MOLLER_TRIES - 1) | (ua[:, r] * top <= _moller_ratio(gm, x)))
        th = np.where(ok, x * T, th)
        kept = np.where(ok, r, kept)
    return th, kept


def sample_michel(u):
    """the kernel's Michel x of the uniforms u: F(x) = x^3 (2 - x) = u by Newton from cbrt(u / 2)"""
    x = np.cbrt(0.5 * u)
    for _ in range(MICHEL_NEWTON):
        x = x - (x * x * x * (2.0 - x) - u) / (2.0 * x * x * (3.0 - 2.0 * x))
    return np.minimum(x, 1.0)


def _rotate(D, a, b, mu):
    """gen_rotate: the local direction (a, b, mu) in the frame of the unit vectors D, renormalised"""
    polar = np.abs(D[:, 2]) > 0.99999
    dx, dy, dz = np.where(polar, D[:, 1], D[:, 0]), np.where(polar, D[:, 2], D[:, 1]), np.where(polar, D[:, 0], D[:, 2])
    den = np.sqrt(1.0 - dz * dz)
    rx = (dx * dz * a - dy * b) / den + dx * mu
    ry = (dy * dz * a + dx * b) / den + dy * mu
    rz = -a * den + dz * mu
    nx, ny, nz = np.where(polar, rz, rx), np.where(polar, rx, ry), np.where(polar, ry, rz)
    nn = np.sqrt(nx * nx + ny * ny + nz * nz)
    return np.stack([nx / nn, ny / nn, nz / nn], axis=1)


# ---- the numpy twin ---------------------------------------------------------------------------------------------------------
def walk_generation_twin(part, p=None, cp=None, seed=0, emit=True, float_type=np.float64):
    """``walk_generation`` on the host: gen_step<true> and cas_decay of csrc/kernels_trackgen.hip operation for operation.  Besides
    ``walk_generation``'s keys: "sec_parent_dir", "sec_parent_tm" (the parent's direction at the emitting step's start and its
    midpoint energy; decays: the end values) and "forced_tries" (Moller samplers that reached their forced last try)."""
    p = TG.params() if p is None else p
    cp = cascade_params() if cp is None else cp
    validate(p, cp)
    part = validate_particles(part, p)
    F = float_type
    n = len(part)
    seed = int(seed) & R.MASK64
    key = part["key"].astype(np.uint64)
    M = _mass(part["pdg"]).astype(F)
    is_el = np.abs(part["pdg"]) == 11
    lo, hi = np.array(p["world_lo"], dtype=F), np.array(p["world_hi"], dtype=F)
    d = part["dir"].astype(F)
    d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    pos = part["pos"].astype(F)
    T = part["kinetic_energy"].astype(F)
    t = part["time"].astype(F)
    path = np.zeros(n, dtype=F)
    counts = np.zeros(n, dtype=np.int32)
    state = np.full(n, -1, dtype=np.int32)
    x0cm = F(p["rad_length"]) / F(p["density"])
    kzr = F(p["k_coeff"]) * F(p["z_over_a"]) * F(p["density"])
    t_cut, t_min, t_track = F(p["t_cut"]), F(p["t_min"]), F(cp["t_track"])
    delta = bool(emit) and bool(cp["delta_tracks"])
    decays = bool(emit) and bool(cp["decays"])
    me = F(ELECTRON_MASS)
    seg = {k: [] for k in F64_COLUMNS}
    seg_prim, seg_step = [], []
    sec = {k: [] for k in ("parent", "step", "j", "dir", "ke", "u", "pos", "time", "pdg", "process", "pdir", "ptm")}
    forced = 0
    act = np.arange(n)
    s = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while len(act):
            P0, D, Ta, Ma, ka, el = pos[act], d[act], T[act], M[act], key[act], is_el[act]
            m = len(act)
            blk = STEP_BLOCKS * s
            bg2, beta2, gamma, tmx = TG._kin(Ta, Ma)
            tmx = np.where(el, 0.5 * Ta, tmx)
            s_full = TG._rate(bg2, beta2, tmx, tmx, p)
            s_full = np.where(el, _rate_e(bg2, beta2, gamma, Ta, tmx, p), s_full)
            h = np.maximum(np.minimum(F(p["step"]), F(p["max_loss_fraction"]) * Ta / s_full), F(p["min_step"]))
            dw = np.full(m, np.inf, dtype=F)
            axis = np.zeros(m, dtype=np.int64)
            far = np.zeros(m, dtype=bool)
            for k in range(3):
                tk = np.full(m, np.inf, dtype=F)
                pl, mi = D[:, k] > 0, D[:, k] < 0
                tk[pl] = np.maximum((hi[k] - P0[pl, k]) / D[pl, k], 0.0)
                tk[mi] = np.maximum((P0[mi, k] - lo[k]) / -D[mi, k], 0.0)
                less = tk < dw
                dw = np.where(less, tk, dw)
                axis = np.where(less, k, axis)
                far = np.where(less, D[:, k] > 0, far)
            leaves = dw <= h
            h = np.where(leaves, dw, h)
            u0 = None
            if (p["straggling"] and p["energy_loss"]) or p["mcs"]:
                u0 = R.keyed_block_uniforms(seed, TAG_GEN, ka, blk).astype(F)
            eem = np.zeros(m, dtype=F)
            emitted = []                # (rows of act, j, th, direction, u) of this step, filled in below
            if p["energy_loss"]:
                Tm = np.maximum(Ta - 0.5 * s_full * h, t_min)
                bg2, beta2, gamma, tmx = TG._kin(Tm, Ma)
                tmx = np.where(el, 0.5 * Tm, tmx)
                tc = np.minimum(t_cut, tmx) if p["straggling"] else tmx
                s_mean = TG._rate(bg2, beta2, tmx, tc, p)
                s_mean = np.where(el, _rate_e(bg2, beta2, gamma, Tm, tc, p), s_mean)
                dE = s_mean * h
                if p["straggling"]:
                    xi = 0.5 * kzr * h / beta2
                    var = xi * tc * (1.0 - beta2 * tc / (2.0 * tmx))
                    dE = np.maximum(dE + np.sqrt(var) * TG._normal(u0[:, 0], u0[:, 1]), 0.0)
                    hard = tmx > t_cut
                    if hard.any():
                        u1 = R.keyed_block_uniforms(seed, TAG_GEN, ka, blk + 1).astype(F)
                        lam = xi * ((1.0 / t_cut - 1.0 / tmx) - (beta2 / tmx) * np.log(tmx / t_cut))
                        lam = np.where(el, xi * _lambda_e(gamma, Tm, t_cut), lam)
                        up = u1[:, 0] - F(2.0 ** -25)
                        pk = np.exp(-lam)
                        c = pk.copy()
                        nh = np.zeros(m, dtype=np.int64)
                        go = hard.copy()
                        for k in range(1, HARD_CAP + 1):
                            go = go & (up > c)
                            nh = np.where(go, k, nh)
                            pk = pk * lam / F(k)
                            c = c + pk
                        for j in range(int(nh.max())):
                            want = np.nonzero(nh > j)[0]
                            th = np.zeros(len(want), dtype=F)
                            done = np.zeros(len(want), dtype=bool)
                            hv = ~el[want]
                            for r in range(HARD_TRIES):
                                if done[hv].all():
                                    break
                                if r % 2 == 0:
                                    uj = R.keyed_block_uniforms(seed, TAG_GEN, ka[want], blk + 2 + 2 * j + r // 2).astype(F)
                                ue, uacc = uj[:, 2 * (r % 2)], uj[:, 2 * (r % 2) + 1]
                                cand = 1.0 / (1.0 / t_cut - ue * (1.0 / t_cut - 1.0 / tmx[want]))
                                ok = hv & ~done & ((uacc > beta2[want] * cand / tmx[want]) | (r == HARD_TRIES - 1))
                                th = np.where(ok, cand, th)
                                done = done | ok
                            we = want[el[want]]
                            if len(we):
                                idx = [8 + 8 * j + 2 * r if r < HARD_TRIES else DRAW_MOLLER + 5 * j + 2 * (r - HARD_TRIES)
                                       for r in range(MOLLER_TRIES)]
                                ue = np.stack([_draw(seed, ka[we], blk, i) for i in idx], axis=1).astype(F)
                                ua = np.stack([_draw(seed, ka[we], blk, i + 1) for i in idx[:-1]] + [np.zeros(len(we), np.float32)],
                                              axis=1).astype(F)
                                the, kept = sample_moller(ue, ua, Tm[we], t_cut)
                                forced += int((kept == MOLLER_TRIES - 1).sum())
                                th[el[want]] = the
                            out = np.zeros(len(want), dtype=bool)
                            if delta:
                                out = (th >= t_track) & (eem[want] + th < Ta[want])
                            eem[want] = np.where(out, eem[want] + th, eem[want])
                            dE[want] = np.where(out, dE[want], dE[want] + th)
                            if out.any():
                                wo, tho = want[out], th[out]
                                E, pp = Tm[wo] + Ma[wo], np.sqrt(Tm[wo] * (Tm[wo] + 2.0 * Ma[wo]))
                                pe = np.sqrt(tho * (tho + 2.0 * me))
                                ct = np.minimum(tho * (E + me) / (pp * pe), 1.0)
                                st = np.sqrt(1.0 - ct * ct)
                                phi = F(TWO_PI) * _draw(seed, ka[wo], blk, DRAW_AZIMUTH + j).astype(F)
                                dirs = _rotate(D[wo], st * np.cos(phi), st * np.sin(phi), ct)
                                emitted.append((wo, j, tho, dirs, _draw(seed, ka[wo], blk, DRAW_PLACE + j).astype(F), Tm[wo]))
                spent = dE + eem
                stops = (spent >= Ta) | (Ta - spent < t_min)
                dE = np.where(stops, Ta - eem, dE)
                h = np.where(stops, np.minimum(h, Ta / s_mean), h)
            else:
                Tm = Ta
                dE = np.zeros(m, dtype=F)
                stops = np.zeros(m, dtype=bool)
            leaves = leaves & ~stops
            E = Tm + Ma
            beta = np.sqrt(beta2)
            P1 = P0 + h[:, None] * D
            rows = np.arange(m)
            wall = np.where(far, hi[axis], lo[axis])
            P1[rows, axis] = np.where(leaves, wall, P1[rows, axis])
            P1 = np.minimum(np.maximum(P1, lo), hi)
            t1 = t[act] + h / (beta * F(C_LIGHT))
            for wo, j, tho, dirs, u, tmo in emitted:
                sec["parent"].append(act[wo])
                sec["step"].append(np.full(len(wo), s, dtype=np.int64))
                sec["j"].append(np.full(len(wo), j, dtype=np.int64))
                sec["dir"].append(dirs)
                sec["ke"].append(tho)
                sec["pos"].append(np.minimum(np.maximum(P0[wo] + (u * h[wo])[:, None] * D[wo], lo), hi))
                sec["time"].append(t[act][wo] + u * (t1[wo] - t[act][wo]))
                sec["pdg"].append(np.full(len(wo), 11, dtype=np.int32))
                sec["process"].append(np.full(len(wo), DELTA_RAY, dtype=np.int32))
                sec["pdir"].append(D[wo])
                sec["ptm"].append(tmo)
            last = s + 1 >= p["max_steps"]
            newstate = np.where(stops, STOPPED, np.where(leaves, EXITED, TRUNCATED if last else -1)).astype(np.int32)
            if p["mcs"]:
                th0 = TG._theta0(h, beta2, E, p)
                ax, ay = th0 * TG._normal(u0[:, 2], u0[:, 3]), th0 * TG._normal_sin(u0[:, 2], u0[:, 3])
                nrm = np.sqrt(1.0 + ax * ax + ay * ay)
                D1 = np.where((newstate == -1)[:, None], _rotate(D, ax / nrm, ay / nrm, 1.0 / nrm), D)
            else:
                D1 = D
            for k, name in enumerate("xyz"):
                seg[name + "_start"].append(P0[:, k])
                seg[name + "_end"].append(P1[:, k])
                seg[name].append(0.5 * (P0[:, k] + P1[:, k]))
            seg["dx"].append(h)
            seg["dE"].append(dE)
            seg["dEdx"].append(np.where(h > 0, dE / h, 0.0))
            seg["t_start"].append(t[act])
            seg["t_end"].append(t1)
            seg["t"].append(0.5 * (t[act] + t1))
            seg_prim.append(act.copy())
            seg_step.append(np.full(m, s, dtype=np.int32))
            pos[act], d[act], t[act] = P1, D1, t1
            T[act] = np.where(stops, 0.0, (Ta - dE) - eem)
            path[act] = path[act] + h
            counts[act] = s + 1
            state[act] = newstate
            act = act[newstate == -1]
            s += 1
        # decays of the muons that stopped: draws of the step index after the last
        mu = np.nonzero((state == STOPPED) & (np.abs(part["pdg"]) == 13))[0] if decays else np.zeros(0, dtype=np.int64)
        if len(mu):
            blk = STEP_BLOCKS * counts[mu].astype(np.int64)
            u0 = R.keyed_block_uniforms(seed, TAG_GEN, key[mu], blk).astype(F)
            minus = part["pdg"][mu] == 13
            x = sample_michel(_draw(seed, key[mu], blk, 4).astype(F))
            etot = x * F(MICHEL_W)
            go = ~(minus & (u0[:, 0] <= F(cp["capture_fraction"]))) & ~(etot <= me)
            cm, phi = 1.0 - 2.0 * u0[:, 2], F(TWO_PI) * u0[:, 3]
            sm = np.sqrt(np.maximum(0.0, 1.0 - cm * cm))
            life = np.where(minus, F(cp["mu_minus_lifetime"]), F(cp["mu_plus_lifetime"]))
            w = mu[go]
            sec["parent"].append(w)
            sec["step"].append(counts[w].astype(np.int64))
            sec["j"].append(np.full(len(w), HARD_CAP, dtype=np.int64))
            sec["dir"].append(np.stack([sm * np.cos(phi), sm * np.sin(phi), cm], axis=1)[go])
            sec["ke"].append((etot - me)[go])
            sec["pos"].append(pos[w])
            sec["time"].append((t[mu] - life * np.log(u0[:, 1]))[go])
            sec["pdg"].append(np.where(minus, 11, -11).astype(np.int32)[go])
            sec["process"].append(np.full(len(w), DECAY, dtype=np.int32))
            sec["pdir"].append(d[w])
            sec["ptm"].append(T[w])
    prim_i = np.concatenate(seg_prim) if seg_prim else np.zeros(0, dtype=np.int64)
    step_i = np.concatenate(seg_step) if seg_step else np.zeros(0, dtype=np.int32)
    order = np.lexsort((step_i, prim_i))
    out = {k: np.concatenate(v)[order] if v else np.zeros(0, dtype=F) for k, v in seg.items()}
    out["primary"] = prim_i[order].astype(np.int32)
    out["step"] = step_i[order]
    out["pdg_id"] = part["pdg"][out["primary"]].astype(np.int32)
    out["event_id"] = part["event_id"][out["primary"]].astype(np.int32)
    out.update(counts=counts, end_state=state, end_pos=pos, end_time=t, path=path, end_energy=T)
    # the secondaries in the order (parent, step, collision; the decay last)
    cat = {k: (np.concatenate(v) if v else np.zeros((0, 3) if k in ("dir", "pos", "pdir") else 0)) for k, v in sec.items()}
    par, stp, jj = cat["parent"].astype(np.int64), cat["step"].astype(np.int64), cat["j"].astype(np.int64)
    order = np.lexsort((jj, stp, par))
    par, stp, jj = par[order], stp[order], jj[order]
    rec = np.zeros(len(par), dtype=particle_dtype)
    rec["pos"], rec["dir"] = cat["pos"][order].astype(np.float64), cat["dir"][order].astype(np.float64)
    rec["kinetic_energy"], rec["time"] = cat["ke"][order].astype(np.float64), cat["time"][order].astype(np.float64)
    rec["pdg"], rec["process"] = cat["pdg"][order], cat["process"][order]
    rec["event_id"], rec["track_in_event"] = part["event_id"][par], part["track_in_event"][par]
    rec["parent"], rec["parent_step"], rec["generation"] = par, stp, part["generation"][par] + 1
    last = np.where(rec["process"] == DECAY, DECAY_KEY, 1 + jj)
    rec["key"] = R.key_mix(R.key_mix(key[par], 1 + stp), last) if len(par) else 0
    out["secondaries"] = rec
    out["secondary_counts"] = np.bincount(par, minlength=n).astype(np.int32)
    out["sec_parent_dir"], out["sec_parent_tm"] = cat["pdir"][order].astype(np.float64), cat["ptm"][order].astype(np.float64)
    out["forced_tries"] = forced
    return out


# ---- the GPU walk -----------------------------------------------------------------------------------------------------------
def count_generation(part, p=None, cp=None, seed=0, emit=True, ctx=None):
    """the count pass of one generation: ``track_generator.count``'s keys and "secondary_counts" i4 [n]"""
    from . import lib
    p = TG.params() if p is None else p
    cp = cascade_params() if cp is None else cp
    validate(p, cp)
    P, CP = TG._pack(p), _pack(cp, emit)
    part = validate_particles(part, p)
    n = len(part)
    counts, scounts, state = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    end = np.zeros((n, 6))
    ctx = ctx or lib.context(refresh_consts=False)
    lib.check(lib.load().ldsim_track_cascade_count(ctx, C.byref(P), C.byref(CP), lib.ptr(part), C.c_int64(n),
                                                   C.c_uint64(int(seed) & R.MASK64), lib.ptr(counts), lib.ptr(scounts),
                                                   lib.ptr(state), lib.ptr(end)))
    return {"counts": counts, "secondary_counts": scounts, "end_state": state, "end_pos": end[:, :3].copy(),
            "end_time": end[:, 3].copy(), "path": end[:, 4].copy(), "end_energy": end[:, 5].copy()}


def walk_generation(part, p=None, cp=None, seed=0, emit=True, ctx=None):
    """One generation on the GPU: the segments of every particle ordered by (particle index, step index) -- ``F64_COLUMNS``,
    ``I32_COLUMNS`` ("primary" = the particle's index), the count pass's per-particle results -- and "secondaries", the emitted
    ``particle_dtype`` records in the order (parent, step, collision; the decay last).  The capacities come from the count pass."""
    from . import lib
    p = TG.params() if p is None else p
    cp = cascade_params() if cp is None else cp
    ctx = ctx or lib.context(refresh_consts=False)
    out = count_generation(part, p, cp, seed, emit, ctx)
    P, CP = TG._pack(p), _pack(cp, emit)
    part = validate_particles(part, p)
    total, stotal = int(out["counts"].astype(np.int64).sum()), int(out["secondary_counts"].astype(np.int64).sum())
    cap, scap = max(total, 1), max(stotal, 1)
    f = np.zeros((len(F64_COLUMNS), cap))
    i = np.zeros((len(I32_COLUMNS), cap), dtype=np.int32)
    sec = np.zeros(scap, dtype=particle_dtype)
    nseg, nsec = C.c_int64(), C.c_int64()
    lib.check(lib.load().ldsim_track_cascade(ctx, C.byref(P), C.byref(CP), lib.ptr(part), C.c_int64(len(part)),
                                             C.c_uint64(int(seed) & R.MASK64), C.c_int64(cap), lib.ptr(f), lib.ptr(i), C.byref(nseg),
                                             C.c_int64(scap), lib.ptr(sec), C.byref(nsec)))
    assert nseg.value == total and nsec.value == stotal
    out.update({k: f[j, :total] for j, k in enumerate(F64_COLUMNS)})
    out.update({k: i[j, :total] for j, k in enumerate(I32_COLUMNS)})
    out["secondaries"] = sec[:stotal]
    return out


def walk_generation_ms(ctx=None):
    """HIP-event time (ms) of the last write pass"""
    from . import lib
    ms = C.c_double()
    lib.check(lib.load().ldsim_track_cascade_ms(ctx or lib.context(refresh_consts=False), C.byref(ms)))
    return ms.value


# ---- the loop over generations ------------------------------------------------------------------------------------------------
def _loop(walk, prim_or_part, p, cp, seed):
    p = TG.params() if p is None else p
    cp = cascade_params() if cp is None else cp
    validate(p, cp)
    part = np.asarray(prim_or_part)
    part = particles(part) if part.dtype != particle_dtype else part
    gens = []
    for g in range(cp["max_generations"]):
        out = walk(part, p, cp, seed, g + 1 < cp["max_generations"])
        out["particles"] = part
        gens.append(out)
        part = out["secondaries"]
        if not len(part):
            break
    return gens


def cascade_twin(prim, p=None, cp=None, seed=0, float_type=np.float64):
    """``cascade`` in numpy: a list with one ``walk_generation_twin`` result (and its "particles") per generation"""
    return _loop(lambda a, b, c, d, e: walk_generation_twin(a, b, c, d, e, float_type), prim, p, cp, seed)


def cascade(prim, p=None, cp=None, seed=0, ctx=None):
    """The generations of ``prim`` (``track_generator.primaries`` output, or generation-0 ``particles``) on the GPU: a list with one
    ``walk_generation`` result (and its "particles") per generation, until nothing is emitted or ``max_generations``; the last
    allowed generation walks with emission off, so that the segments' energy adds up whatever the cap"""
    return _loop(lambda a, b, c, d, e: walk_generation(a, b, c, d, e, ctx), prim, p, cp, seed)


def ancestors(gens):
    """per generation, the index in generation 0 of every particle's ancestor"""
    root = [np.arange(len(gens[0]["particles"]))]
    for g in gens[1:]:
        root.append(root[-1][g["particles"]["parent"]])
    return root


# ---- datasets ---------------------------------------------------------------------------------------------------------------
def to_datasets(gens, traj_id0=0, vertex_id0=0, segment_id0=0):
    """(segments, trajectories, vertices) of a ``cascade`` / ``cascade_twin`` result.  One trajectory per particle of every
    generation, ``traj_id`` in the order (generation, index), ``parent_id`` the parent's ``traj_id`` (-1 in generation 0, which
    alone is ``primary``); segments sorted by (vertex by first appearance, ``traj_id``, step), so that an event's segments are
    contiguous; vertices as ``track_generator.to_datasets``: of the primaries"""
    from .layout import segments_dtype
    part = np.concatenate([g["particles"] for g in gens])
    first = np.concatenate([[0], np.cumsum([len(g["particles"]) for g in gens])])
    prim = gens[0]["particles"]
    ev0 = prim["event_id"].astype(np.int64)
    uniq, head, inverse = np.unique(ev0, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(head))                 # events numbered by first appearance
    root = np.concatenate(ancestors(gens))
    vertex = rank[inverse][root] + int(vertex_id0)
    t0 = prim["time"][root]
    col = {k: np.concatenate([np.asarray(g[k]) for g in gens]) for k in F64_COLUMNS + ("pdg_id", "event_id", "step")}
    ip = np.concatenate([np.asarray(g["primary"], dtype=np.int64) + first[k] for k, g in enumerate(gens)])
    order = np.lexsort((col["step"], ip, vertex[ip]))
    ip = ip[order]
    seg = np.zeros(len(ip), dtype=segments_dtype)
    for k in F64_COLUMNS:
        seg[k] = col[k][order]
    for k in ("t0", "t0_start", "t0_end"):
        seg[k] = t0[ip]
    seg["pdg_id"], seg["event_id"] = col["pdg_id"][order], col["event_id"][order]
    seg["traj_id"] = seg["file_traj_id"] = ip + int(traj_id0)
    seg["vertex_id"] = seg["file_vertex_id"] = vertex[ip]
    seg["segment_id"] = np.arange(len(ip)) + int(segment_id0)
    traj = np.zeros(len(part), dtype=TG.trajectories_dtype)
    M = _mass(part["pdg"])
    d = part["dir"] / np.sqrt((part["dir"] * part["dir"]).sum(axis=1))[:, None]
    T = part["kinetic_energy"]
    cat = {k: np.concatenate([np.asarray(g[k], dtype=np.float64) for g in gens])
           for k in ("end_energy", "end_pos", "end_time", "path", "end_state", "counts")}
    traj["event_id"] = part["event_id"]
    traj["vertex_id"] = traj["file_vertex_id"] = vertex
    traj["traj_id"] = traj["file_traj_id"] = np.arange(len(part)) + int(traj_id0)
    gen_of = np.repeat(np.arange(len(gens)), np.diff(first))
    traj["parent_id"] = np.where(gen_of == 0, -1, part["parent"] + first[np.maximum(gen_of - 1, 0)] + int(traj_id0))
    traj["primary"], traj["pdg_id"] = gen_of == 0, part["pdg"]
    traj["E_start"], traj["E_end"] = T + M, cat["end_energy"] + M
    traj["pxyz_start"] = np.sqrt(T * (T + 2.0 * M))[:, None] * d
    traj["xyz_start"], traj["xyz_end"] = part["pos"], cat["end_pos"]
    traj["t_start"], traj["t_end"] = part["time"], cat["end_time"]
    traj["dist_travel"], traj["end_state"], traj["n_segments"] = cat["path"], cat["end_state"], cat["counts"]
    vert = np.zeros(len(uniq), dtype=TG.vertices_dtype)
    by_rank = np.argsort(rank)
    h = head[by_rank]
    vert["event_id"] = uniq[by_rank]
    vert["vertex_id"] = vert["file_vertex_id"] = np.arange(len(uniq)) + int(vertex_id0)
    vert["x_vert"], vert["y_vert"], vert["z_vert"] = prim["pos"][h, 0], prim["pos"][h, 1], prim["pos"][h, 2]
    vert["t_vert"] = prim["time"][h]
    vert["n_primaries"] = np.bincount(rank[inverse], minlength=len(uniq))
    return seg, traj, vert
