"""Track generator: keyed transport of muons, pions and protons through liquid argon to edep-sim segments
(csrc/kernels_trackgen.hip; include/ldsim.h states the model).

Heavy charged particles are walked through uniform LAr inside a world box under Bethe energy loss (restricted mean below a cut,
Gaussian soft fluctuation, sampled hard collisions above it) and Highland multiple scattering; every step becomes one segment of
the ``segments`` dataset the driver reads.  Units: cm, MeV, us; positions are in the input file's frame (drift axis in ``x``: what
``prepare_tracks`` / ``swap_coordinates`` expect).

* ``params`` / ``validate`` / ``_pack``: the walk's parameters (``LdsimTrackGenParams``); ``default_world``: the hull of
  ``TPC_BORDERS`` in the file frame plus a margin.
* ``primaries`` / ``gun_primaries`` / ``cosmic_primaries``: what is walked (``LdsimTrackGenPrimary`` records), made on the host
  from keyed draws.  The kernel does not know the source.
* ``count`` / ``generate`` / ``generate_ms``: the GPU walk (``ldsim_track_gen_count`` / ``ldsim_track_gen``).
* ``generate_twin``: the same walk in numpy, operation for operation in f64, from numpy-made keyed draws.
* ``stopping_power`` / ``restricted_stopping_power`` / ``tmax`` / ``highland_theta0``: the twin's building blocks.
* ``to_datasets``: ``segments`` (``layout.segments_dtype``), ``trajectories`` (one row per primary), ``vertices`` (one per event).
"""
import ctypes as C
import math

import numpy as np

from . import rng as R

TAG_GEN = R.TAG_GEN
ELECTRON_MASS = 0.51099895                     # MeV; include/ldsim.h LDSIM_TRACK_GEN_ME
MASSES = {13: 105.6583755, 211: 139.57039, 2212: 938.27208816}    # MeV by |pdg|; include/ldsim.h LDSIM_TRACK_GEN_M_*
C_LIGHT = 29979.2458                           # cm / us
HARD_CAP, HARD_TRIES, STEP_BLOCKS = 8, 4, 32   # include/ldsim.h LDSIM_TRACK_GEN_HARD_CAP / _HARD_TRIES / _STEP_BLOCKS
MAX_STEPS_LIMIT = 1 << 24                      # include/ldsim.h LDSIM_TRACK_GEN_MAX_STEPS
STOPPED, EXITED, TRUNCATED = 0, 1, 2           # end states
END_STATE_NAMES = ("stopped", "exited", "truncated")
TWO_PI = 6.283185307179586
LN10 = 2.302585092994046
F64_COLUMNS = ("x_start", "y_start", "z_start", "x_end", "y_end", "z_end", "x", "y", "z", "dx", "dE", "dEdx", "t_start", "t_end",
               "t")
I32_COLUMNS = ("primary", "step", "pdg_id", "event_id")

primary_dtype = np.dtype([("pos", "f8", 3), ("dir", "f8", 3), ("kinetic_energy", "f8"), ("time", "f8"), ("pdg", "i4"),
                          ("event_id", "i4"), ("track_in_event", "i4"), ("_pad", "i4")])          # LdsimTrackGenPrimary, 80 bytes

# The two truth datasets the driver passes through, restated from what it reads of them: the event separator (``event_id``) for
# its event selection and for ``attach_event_times``; the ids the segments point at; and what a reader of a trajectory expects
# (where it started and ended, with what energy and when).  ``t_event`` is prepended to ``vertices`` by the driver itself.
trajectories_dtype = np.dtype([
    ("event_id", "u4"), ("vertex_id", "u8"), ("file_vertex_id", "u8"), ("traj_id", "u4"), ("file_traj_id", "u4"),
    ("parent_id", "i4"), ("primary", "?"), ("pdg_id", "i4"), ("E_start", "f4"), ("E_end", "f4"), ("pxyz_start", "f4", 3),
    ("xyz_start", "f4", 3), ("xyz_end", "f4", 3), ("t_start", "f8"), ("t_end", "f8"), ("dist_travel", "f4"),
    ("end_state", "i4"), ("n_segments", "u4")], align=True)
vertices_dtype = np.dtype([("event_id", "u4"), ("vertex_id", "u8"), ("file_vertex_id", "u8"), ("x_vert", "f4"),
                           ("y_vert", "f4"), ("z_vert", "f4"), ("t_vert", "f8"), ("n_primaries", "u4")], align=True)


class TrackGenError(ValueError):
    pass


# ---- parameters -------------------------------------------------------------------------------------------------------------
def default_world(margin=10.0):
    """(lo, hi) of the hull of ``consts.detector.TPC_BORDERS`` in the file frame (x <-> z swapped back) plus ``margin`` cm"""
    from . import consts
    b = np.sort(np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64), axis=-1)
    lo, hi = b[:, :, 0].min(axis=0) - margin, b[:, :, 1].max(axis=0) + margin
    return lo[::-1].copy(), hi[::-1].copy()


def params(world=None, step=0.1, min_step=1e-4, max_loss_fraction=0.05, t_cut=0.1, t_min=0.5, straggling=True, mcs=True,
           energy_loss=True, max_steps=100000, density=None, z_over_a=18.0 / 39.948, mean_excitation=188e-6, rad_length=19.55,
           k_coeff=0.307075, sternheimer=(0.19559, 3.0, 0.2, 3.0, 5.2146, 0.0)):
    """the walk's parameters as a dict.  ``world``: (lo, hi) in cm, default ``default_world()``; ``step``: the largest step;
    ``t_cut``: collisions above it are sampled one by one; ``t_min``: kinetic energy below which a walk ends; ``mean_excitation``
    in MeV; ``rad_length`` in g/cm^2; ``sternheimer``: (a, k, x0, x1, Cbar, delta0); ``energy_loss`` False is for tests of the
    scattering alone"""
    if world is None:
        world = default_world()
    if density is None:
        from . import consts
        density = consts.detector.LAR_DENSITY
    p = {"world_lo": [float(v) for v in world[0]], "world_hi": [float(v) for v in world[1]], "step": float(step),
         "min_step": float(min_step), "max_loss_fraction": float(max_loss_fraction), "t_cut": float(t_cut), "t_min": float(t_min),
         "straggling": int(bool(straggling)), "mcs": int(bool(mcs)), "energy_loss": int(bool(energy_loss)),
         "max_steps": int(max_steps), "density": float(density), "z_over_a": float(z_over_a),
         "mean_excitation": float(mean_excitation), "rad_length": float(rad_length), "k_coeff": float(k_coeff),
         "sternheimer": [float(v) for v in sternheimer]}
    validate(p)
    return p


def _pos(v):
    return math.isfinite(v) and v > 0


def validate(p):
    """refuses what ``ldsim_track_gen`` refuses of the parameters"""
    for k in ("step", "min_step", "max_loss_fraction", "t_cut", "t_min", "density", "z_over_a", "mean_excitation", "rad_length",
              "k_coeff"):
        if not _pos(p[k]):
            raise TrackGenError(f"{k} = {p[k]}: must be finite and > 0")
    if p["min_step"] > p["step"]:
        raise TrackGenError(f"min_step {p['min_step']} exceeds step {p['step']}")
    if p["max_loss_fraction"] > 1:
        raise TrackGenError(f"max_loss_fraction = {p['max_loss_fraction']}: must lie in (0, 1]")
    if not p["t_cut"] > p["mean_excitation"]:
        raise TrackGenError(f"t_cut {p['t_cut']} MeV must exceed the mean excitation energy {p['mean_excitation']} MeV")
    if len(p["sternheimer"]) != 6 or not all(math.isfinite(v) for v in p["sternheimer"]):
        raise TrackGenError("sternheimer: six finite numbers (a, k, x0, x1, Cbar, delta0)")
    if len(p["world_lo"]) != 3 or len(p["world_hi"]) != 3:
        raise TrackGenError("world: (lo, hi), three coordinates each")
    for k in range(3):
        lo, hi = p["world_lo"][k], p["world_hi"][k]
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            raise TrackGenError(f"world box is empty or inverted along axis {k}: [{lo}, {hi}]")
    if not 1 <= p["max_steps"] <= MAX_STEPS_LIMIT:
        raise TrackGenError(f"max_steps = {p['max_steps']}: must lie in 1 .. {MAX_STEPS_LIMIT}")
    for pdg, m in MASSES.items():
        if not float(restricted_stopping_power(p["t_min"], pdg, p, p["t_cut"])) > 0:
            raise TrackGenError(f"t_min {p['t_min']} MeV: the stopping power of pdg {pdg} is not positive there (the Bethe formula "
                                "has ended); raise t_min")


def primaries(pdg, pos, direction, kinetic_energy, time=0.0, event_id=0, track_in_event=0):
    """``LdsimTrackGenPrimary`` records from broadcastable columns"""
    ke = np.atleast_1d(np.asarray(kinetic_energy, dtype=np.float64))
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    direction = np.asarray(direction, dtype=np.float64).reshape(-1, 3)
    n = max(len(ke), len(pos), len(direction), np.size(pdg), np.size(event_id), np.size(track_in_event), np.size(time))
    out = np.zeros(n, dtype=primary_dtype)
    out["pos"], out["dir"], out["kinetic_energy"], out["time"] = pos, direction, ke, time
    out["pdg"], out["event_id"], out["track_in_event"] = pdg, event_id, track_in_event
    return out


def validate_primaries(prim, p):
    """refuses what ``ldsim_track_gen`` refuses of the primaries"""
    prim = np.ascontiguousarray(prim, dtype=primary_dtype)
    lo, hi = np.array(p["world_lo"]), np.array(p["world_hi"])
    for i in range(len(prim)):
        r = prim[i]
        if abs(int(r["pdg"])) not in MASSES or int(r["pdg"]) == -2212:
            raise TrackGenError(f"primary {i}: unknown pdg {int(r['pdg'])} (13, -13, 211, -211 and 2212 are transported)")
        if not _pos(float(r["kinetic_energy"])):
            raise TrackGenError(f"primary {i}: kinetic energy {float(r['kinetic_energy'])} MeV must be finite and > 0")
        if not (np.isfinite(r["pos"]).all() and (r["pos"] >= lo).all() and (r["pos"] <= hi).all()):
            raise TrackGenError(f"primary {i}: starts outside the world box, at {r['pos'].tolist()}")
        nn = float(np.sqrt((r["dir"] * r["dir"]).sum()))
        if not (np.isfinite(r["dir"]).all() and nn > 0):
            raise TrackGenError(f"primary {i}: zero direction")
        if not math.isfinite(float(r["time"])):
            raise TrackGenError(f"primary {i}: time is not finite")
    return prim


def _pack(p):
    from .abi import LdsimTrackGenParams
    validate(p)
    P = LdsimTrackGenParams()
    P.world_lo[:] = p["world_lo"]
    P.world_hi[:] = p["world_hi"]
    for k in ("step", "min_step", "max_loss_fraction", "t_cut", "t_min", "density", "z_over_a", "mean_excitation", "rad_length",
              "k_coeff", "straggling", "mcs", "energy_loss", "max_steps"):
        setattr(P, k, p[k])
    P.sternheimer[:] = p["sternheimer"]
    return P


# ---- the model's building blocks (f64, the kernel's operations in the kernel's order) ---------------------------------------------
def _mass(pdg):
    a = np.abs(np.asarray(pdg, dtype=np.int64))
    return np.where(a == 13, MASSES[13], np.where(a == 211, MASSES[211], MASSES[2212]))


def _kin(T, M):
    """(beta gamma)^2, beta^2, gamma, Tmax (gen_kin)"""
    tau = T / M
    bg2 = tau * (tau + 2.0)
    gamma = tau + 1.0
    beta2 = bg2 / (gamma * gamma)
    r = ELECTRON_MASS / M
    tmx = 2.0 * ELECTRON_MASS * bg2 / (1.0 + 2.0 * gamma * r + r * r)
    return bg2, beta2, gamma, tmx


def _delta(bg2, p):
    """Sternheimer's density effect (gen_delta)"""
    a, k, x0, x1, cbar, d0 = p["sternheimer"]
    x = 0.5 * np.log10(bg2)
    hi = 2.0 * LN10 * x - cbar
    with np.errstate(invalid="ignore", over="ignore"):
        mid = hi + a * np.power(np.maximum(x1 - x, 0.0), k)
        low = d0 * np.power(10.0, 2.0 * (x - x0))
    return np.where(x >= x1, hi, np.where(x >= x0, mid, low))


def _rate(bg2, beta2, tmx, tc, p):
    """restricted stopping power in MeV / cm (gen_rate); tc = tmx gives the unrestricted Bethe mean"""
    kzr = p["k_coeff"] * p["z_over_a"] * p["density"]
    i2 = p["mean_excitation"] * p["mean_excitation"]
    return kzr / beta2 * (0.5 * np.log(2.0 * ELECTRON_MASS * bg2 * tc / i2) - 0.5 * beta2 * (1.0 + tc / tmx)
                          - 0.5 * _delta(bg2, p))


def tmax(T, pdg):
    """largest energy transfer to a free electron, MeV"""
    return _kin(np.asarray(T, dtype=np.float64), _mass(pdg))[3]


def stopping_power(T, pdg, p=None):
    """unrestricted Bethe mass stopping power, MeV cm^2 / g"""
    p = p or params()
    bg2, beta2, _, tmx = _kin(np.asarray(T, dtype=np.float64), _mass(pdg))
    return _rate(bg2, beta2, tmx, tmx, p) / p["density"]


def restricted_stopping_power(T, pdg, p=None, t_cut=None):
    """mass stopping power of the collisions below min(t_cut, Tmax), MeV cm^2 / g"""
    p = p or params()
    bg2, beta2, _, tmx = _kin(np.asarray(T, dtype=np.float64), _mass(pdg))
    return _rate(bg2, beta2, tmx, np.minimum(p["t_cut"] if t_cut is None else t_cut, tmx), p) / p["density"]


def _theta0(h, beta2, E, p):
    x0cm = p["rad_length"] / p["density"]
    with np.errstate(divide="ignore", invalid="ignore"):
        return 13.6 / (beta2 * E) * np.sqrt(h / x0cm) * np.maximum(1.0 + 0.038 * np.log(h / (x0cm * beta2)), 0.0)


def highland_theta0(h, T, pdg, p=None):
    """width (rad) of one plane angle after ``h`` cm: (13.6 MeV / (beta p)) sqrt(h / X0) (1 + 0.038 ln(h / (X0 beta^2)))"""
    p = p or params()
    T, M = np.asarray(T, dtype=np.float64), _mass(pdg)
    return _theta0(np.asarray(h, dtype=np.float64), _kin(T, M)[1], T + M, p)


# ---- keyed draws ----------------------------------------------------------------------------------------------------------------
def stream_keys(event_id, track_in_event):
    return R.key_mix(R.key_mix(np.uint64(R.KEY_ROOT), np.asarray(event_id, dtype=np.int64)),
                     np.asarray(track_in_event, dtype=np.int64))


def _normal(ua, ub):
    """keyed_normal's pairing of two uniforms (the cos member of the Box-Muller pair), evaluated in f64"""
    return np.sqrt(-2.0 * np.log(ua)) * np.cos(TWO_PI * ub)


def _normal_sin(ua, ub):
    return np.sqrt(-2.0 * np.log(ua)) * np.sin(TWO_PI * ub)


# ---- the numpy twin ---------------------------------------------------------------------------------------------------------
def generate_twin(prim, p=None, seed=0, float_type=np.float64):
    """``generate`` on the host: gen_step of csrc/kernels_trackgen.hip operation for operation, over all walking primaries at once.
    ``float_type`` np.longdouble repeats the walk in extended precision (to see which walks hang on a comparison's last bit)."""
    p = params() if p is None else p
    validate(p)
    prim = validate_primaries(prim, p)
    F = float_type
    n = len(prim)
    seed = int(seed) & R.MASK64
    key = stream_keys(prim["event_id"], prim["track_in_event"])
    M = _mass(prim["pdg"]).astype(F)
    lo, hi = np.array(p["world_lo"], dtype=F), np.array(p["world_hi"], dtype=F)
    d = prim["dir"].astype(F)
    d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    pos = prim["pos"].astype(F)
    T = prim["kinetic_energy"].astype(F)
    t = prim["time"].astype(F)
    path = np.zeros(n, dtype=F)
    counts = np.zeros(n, dtype=np.int32)
    state = np.full(n, -1, dtype=np.int32)
    x0cm = F(p["rad_length"]) / F(p["density"])
    kzr = F(p["k_coeff"]) * F(p["z_over_a"]) * F(p["density"])
    t_cut, t_min = F(p["t_cut"]), F(p["t_min"])
    seg = {k: [] for k in F64_COLUMNS}
    seg_prim, seg_step = [], []
    act = np.arange(n)
    s = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while len(act):
            P0, D, Ta, Ma, ka = pos[act], d[act], T[act], M[act], key[act]
            m = len(act)
            bg2, beta2, gamma, tmx = _kin(Ta, Ma)
            s_full = _rate(bg2, beta2, tmx, tmx, p)
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
            u0 = u1 = None
            if (p["straggling"] and p["energy_loss"]) or p["mcs"]:
                u0 = R.keyed_block_uniforms(seed, TAG_GEN, ka, STEP_BLOCKS * s).astype(F)
            if p["energy_loss"]:
                Tm = np.maximum(Ta - 0.5 * s_full * h, t_min)
                bg2, beta2, gamma, tmx = _kin(Tm, Ma)
                tc = np.minimum(t_cut, tmx) if p["straggling"] else tmx
                s_mean = _rate(bg2, beta2, tmx, tc, p)
                dE = s_mean * h
                if p["straggling"]:
                    xi = 0.5 * kzr * h / beta2
                    var = xi * tc * (1.0 - beta2 * tc / (2.0 * tmx))
                    dE = np.maximum(dE + np.sqrt(var) * _normal(u0[:, 0], u0[:, 1]), 0.0)
                    hard = tmx > t_cut
                    if hard.any():
                        u1 = R.keyed_block_uniforms(seed, TAG_GEN, ka, STEP_BLOCKS * s + 1).astype(F)
                        lam = xi * ((1.0 / t_cut - 1.0 / tmx) - (beta2 / tmx) * np.log(tmx / t_cut))
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
                            for r in range(HARD_TRIES):
                                if done.all():
                                    break
                                if r % 2 == 0:
                                    uj = R.keyed_block_uniforms(seed, TAG_GEN, ka[want], STEP_BLOCKS * s + 2 + 2 * j + r // 2).astype(F)
                                ue, uacc = uj[:, 2 * (r % 2)], uj[:, 2 * (r % 2) + 1]
                                cand = 1.0 / (1.0 / t_cut - ue * (1.0 / t_cut - 1.0 / tmx[want]))
                                ok = ~done & ((uacc > beta2[want] * cand / tmx[want]) | (r == HARD_TRIES - 1))
                                th = np.where(ok, cand, th)
                                done = done | ok
                            dE[want] = dE[want] + th
                stops = (dE >= Ta) | (Ta - dE < t_min)
                dE = np.where(stops, Ta, dE)
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
            last = s + 1 >= p["max_steps"]
            newstate = np.where(stops, STOPPED, np.where(leaves, EXITED, TRUNCATED if last else -1)).astype(np.int32)
            if p["mcs"]:
                th0 = _theta0(h, beta2, E, p)
                ax, ay = th0 * _normal(u0[:, 2], u0[:, 3]), th0 * _normal_sin(u0[:, 2], u0[:, 3])
                nrm = np.sqrt(1.0 + ax * ax + ay * ay)
                a, b, mu = ax / nrm, ay / nrm, 1.0 / nrm
                polar = np.abs(D[:, 2]) > 0.99999           # there the rotation is made about the x axis (cyclic permutation)
                dx, dy, dz = np.where(polar, D[:, 1], D[:, 0]), np.where(polar, D[:, 2], D[:, 1]), np.where(polar, D[:, 0], D[:, 2])
                den = np.sqrt(1.0 - dz * dz)
                rx = (dx * dz * a - dy * b) / den + dx * mu
                ry = (dy * dz * a + dx * b) / den + dy * mu
                rz = -a * den + dz * mu
                nx, ny, nz = np.where(polar, rz, rx), np.where(polar, rx, ry), np.where(polar, ry, rz)
                nn = np.sqrt(nx * nx + ny * ny + nz * nz)
                Dn = np.stack([nx / nn, ny / nn, nz / nn], axis=1)
                D1 = np.where((newstate == -1)[:, None], Dn, D)
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
            T[act] = Ta - dE
            path[act] = path[act] + h
            counts[act] = s + 1
            state[act] = newstate
            act = act[newstate == -1]
            s += 1
    prim_i = np.concatenate(seg_prim) if seg_prim else np.zeros(0, dtype=np.int64)
    step_i = np.concatenate(seg_step) if seg_step else np.zeros(0, dtype=np.int32)
    order = np.lexsort((step_i, prim_i))
    out = {k: np.concatenate(v)[order] if v else np.zeros(0, dtype=F) for k, v in seg.items()}
    out["primary"] = prim_i[order].astype(np.int32)
    out["step"] = step_i[order]
    out["pdg_id"] = prim["pdg"][out["primary"]].astype(np.int32)
    out["event_id"] = prim["event_id"][out["primary"]].astype(np.int32)
    out.update(counts=counts, end_state=state, end_pos=pos, end_time=t, path=path, end_energy=T)
    return out


# ---- the GPU walk -----------------------------------------------------------------------------------------------------------
def count(prim, p=None, seed=0, ctx=None):
    """the count pass: {"counts" i4 [n], "end_state" i4 [n] (0 stopped, 1 left the box, 2 truncated), "end_pos" f8 [n, 3],
    "end_time", "path", "end_energy" f8 [n]}"""
    from . import lib
    p = params() if p is None else p
    P = _pack(p)
    prim = validate_primaries(prim, p)
    n = len(prim)
    counts, state, end = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, 6))
    ctx = ctx or lib.context(refresh_consts=False)
    lib.check(lib.load().ldsim_track_gen_count(ctx, C.byref(P), lib.ptr(prim), C.c_int64(n), C.c_uint64(int(seed) & R.MASK64),
                                               lib.ptr(counts), lib.ptr(state), lib.ptr(end)))
    return {"counts": counts, "end_state": state, "end_pos": end[:, :3].copy(), "end_time": end[:, 3].copy(),
            "path": end[:, 4].copy(), "end_energy": end[:, 5].copy()}


def generate(prim, p=None, seed=0, ctx=None):
    """Segments of every primary, ordered by (primary index, step index): the f64 columns ``F64_COLUMNS``, the i4 columns
    ``I32_COLUMNS`` and the count pass's per-primary results (``count``).  The same bytes whatever else is in the call."""
    from . import lib
    p = params() if p is None else p
    P = _pack(p)
    prim = validate_primaries(prim, p)
    ctx = ctx or lib.context(refresh_consts=False)
    out = count(prim, p, seed, ctx)
    total = int(out["counts"].astype(np.int64).sum())
    cap = max(total, 1)
    f = np.zeros((len(F64_COLUMNS), cap))
    i = np.zeros((len(I32_COLUMNS), cap), dtype=np.int32)
    nseg = C.c_int64()
    lib.check(lib.load().ldsim_track_gen(ctx, C.byref(P), lib.ptr(prim), C.c_int64(len(prim)), C.c_uint64(int(seed) & R.MASK64),
                                         C.c_int64(cap), lib.ptr(f), lib.ptr(i), C.byref(nseg)))
    assert nseg.value == total
    out.update({k: f[j, :total] for j, k in enumerate(F64_COLUMNS)})
    out.update({k: i[j, :total] for j, k in enumerate(I32_COLUMNS)})
    return out


def generate_ms(ctx=None):
    """HIP-event time (ms) of the last write pass"""
    from . import lib
    ms = C.c_double()
    lib.check(lib.load().ldsim_track_gen_ms(ctx or lib.context(refresh_consts=False), C.byref(ms)))
    return ms.value


# ---- sources --------------------------------------------------------------------------------------------------------------------
def _source_uniforms(seed, source_tag, event, track, n_draws):
    """uniforms [len(event)][n_draws] (f64 of f32, in (0, 1]) of the stream (seed, TAG_GEN, key(source_tag, event, track))"""
    key = R.key_mix(np.uint64(R.KEY_ROOT), np.full(len(event), source_tag, dtype=np.int64), event, track)
    nb = (n_draws + 3) // 4
    u = np.concatenate([R.keyed_block_uniforms(int(seed) & R.MASK64, TAG_GEN, key, b) for b in range(nb)], axis=1)
    return u[:, :n_draws].astype(np.float64)


def _log_uniform(e, u):
    if np.ndim(e) == 0:
        return np.full(len(u), float(e))
    e0, e1 = float(e[0]), float(e[1])
    if not (_pos(e0) and _pos(e1) and e0 <= e1):
        raise TrackGenError(f"kinetic energy range {e}: 0 < low <= high, MeV")
    return e0 * np.exp(u * math.log(e1 / e0))


def gun_primaries(pdg, pos, direction, kinetic_energy, tracks_per_event=1, n_events=1, seed=0, event_id0=0, time=0.0):
    """``tracks_per_event`` x ``n_events`` primaries from one point.  ``kinetic_energy``: a value, or (low, high) for a log-uniform
    draw; ``direction``: a vector, or None / "isotropic".  The keyed draws depend on (seed, event id, track in event) alone."""
    nt, ne = int(tracks_per_event), int(n_events)
    if nt < 1 or ne < 1:
        raise TrackGenError("tracks_per_event and n_events: >= 1")
    ev = np.repeat(np.arange(ne, dtype=np.int64) + int(event_id0), nt)
    tr = np.tile(np.arange(nt, dtype=np.int64), ne)
    u = _source_uniforms(seed, 1, ev, tr, 3)
    ke = _log_uniform(kinetic_energy, u[:, 0])
    if direction is None or (isinstance(direction, str) and direction == "isotropic"):
        mu, phi = 1.0 - 2.0 * u[:, 1], TWO_PI * u[:, 2]
        st = np.sqrt(np.maximum(0.0, 1.0 - mu * mu))
        direction = np.stack([st * np.cos(phi), st * np.sin(phi), mu], axis=1)
    return primaries(pdg, np.broadcast_to(np.asarray(pos, dtype=np.float64), (len(ev), 3)), direction, ke, time, ev, tr)


def cosmic_primaries(world, kinetic_energy=(1000.0, 100000.0), tracks_per_event=1, n_events=1, seed=0, event_id0=0, pdg=13,
                     vertical_axis=1, time=0.0):
    """Tracks that start uniformly on the world box's top face (``vertical_axis`` of the file frame, y) and point downwards with a
    zenith angle following cos^2 (cos theta = u^(1/3)), azimuth uniform, energy log-uniform in the range"""
    nt, ne = int(tracks_per_event), int(n_events)
    if nt < 1 or ne < 1:
        raise TrackGenError("tracks_per_event and n_events: >= 1")
    lo, hi = np.asarray(world[0], dtype=np.float64), np.asarray(world[1], dtype=np.float64)
    ev = np.repeat(np.arange(ne, dtype=np.int64) + int(event_id0), nt)
    tr = np.tile(np.arange(nt, dtype=np.int64), ne)
    u = _source_uniforms(seed, 2, ev, tr, 5)
    v = int(vertical_axis)
    a, b = (v + 1) % 3, (v + 2) % 3
    pos = np.empty((len(ev), 3))
    pos[:, v] = hi[v]
    pos[:, a] = lo[a] + u[:, 0] * (hi[a] - lo[a])
    pos[:, b] = lo[b] + u[:, 1] * (hi[b] - lo[b])
    ct = np.cbrt(u[:, 2])
    st, phi = np.sqrt(np.maximum(0.0, 1.0 - ct * ct)), TWO_PI * u[:, 3]
    d = np.empty((len(ev), 3))
    d[:, v], d[:, a], d[:, b] = -ct, st * np.cos(phi), st * np.sin(phi)
    return primaries(pdg, pos, d, _log_uniform(kinetic_energy, u[:, 4]), time, ev, tr)


# ---- datasets ---------------------------------------------------------------------------------------------------------------
def to_datasets(prim, gen, traj_id0=0, vertex_id0=0, segment_id0=0):
    """(segments, trajectories, vertices) of one ``generate`` / ``generate_twin`` result.  ``traj_id`` / ``file_traj_id`` = the
    primary's index in the file (``traj_id0`` + index), ``vertex_id`` = the event's index in the file (events in order of first
    appearance), ``segment_id`` = the running index; the columns the simulation fills stay 0."""
    from .layout import segments_dtype
    prim = np.ascontiguousarray(prim, dtype=primary_dtype)
    ip = np.asarray(gen["primary"], dtype=np.int64)
    ev_of_prim = prim["event_id"].astype(np.int64)
    uniq, first, inverse = np.unique(ev_of_prim, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first))                 # events numbered by first appearance
    vertex_of_prim = rank[inverse] + int(vertex_id0)
    seg = np.zeros(len(ip), dtype=segments_dtype)
    for k in F64_COLUMNS:
        seg[k] = gen[k]
    for k in ("t0", "t0_start", "t0_end"):
        seg[k] = prim["time"][ip]
    seg["pdg_id"] = gen["pdg_id"]
    seg["event_id"] = gen["event_id"]
    seg["traj_id"] = seg["file_traj_id"] = ip + int(traj_id0)
    seg["vertex_id"] = seg["file_vertex_id"] = vertex_of_prim[ip]
    seg["segment_id"] = np.arange(len(ip)) + int(segment_id0)
    traj = np.zeros(len(prim), dtype=trajectories_dtype)
    M = _mass(prim["pdg"])
    d = prim["dir"] / np.sqrt((prim["dir"] * prim["dir"]).sum(axis=1))[:, None]
    T = prim["kinetic_energy"]
    traj["event_id"] = prim["event_id"]
    traj["vertex_id"] = traj["file_vertex_id"] = vertex_of_prim
    traj["traj_id"] = traj["file_traj_id"] = np.arange(len(prim)) + int(traj_id0)
    traj["parent_id"], traj["primary"], traj["pdg_id"] = -1, True, prim["pdg"]
    traj["E_start"], traj["E_end"] = T + M, np.asarray(gen["end_energy"], dtype=np.float64) + M
    traj["pxyz_start"] = np.sqrt(T * (T + 2.0 * M))[:, None] * d
    traj["xyz_start"], traj["xyz_end"] = prim["pos"], np.asarray(gen["end_pos"], dtype=np.float64)
    traj["t_start"], traj["t_end"] = prim["time"], np.asarray(gen["end_time"], dtype=np.float64)
    traj["dist_travel"], traj["end_state"], traj["n_segments"] = gen["path"], gen["end_state"], gen["counts"]
    vert = np.zeros(len(uniq), dtype=vertices_dtype)
    by_rank = np.argsort(rank)
    head = first[by_rank]
    vert["event_id"] = uniq[by_rank]
    vert["vertex_id"] = vert["file_vertex_id"] = np.arange(len(uniq)) + int(vertex_id0)
    vert["x_vert"], vert["y_vert"], vert["z_vert"] = prim["pos"][head, 0], prim["pos"][head, 1], prim["pos"][head, 2]
    vert["t_vert"] = prim["time"][head]
    vert["n_primaries"] = np.bincount(rank[inverse], minlength=len(uniq))[np.arange(len(uniq))]
    return seg, traj, vert
