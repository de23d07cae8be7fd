"""Light LUT builder: keyed photon transport in a TPC box (csrc/kernels_lutbuild.hip; include/ldsim.h states the model).

Scintillation photons are walked from every voxel of a box ``[0, Lu] x [0, Lv] x [0, Lw]`` cm to rectangular detectors on its
walls under Rayleigh scattering, bulk absorption and diffuse wall reflection; the tallies become ``vis``, ``t0``, ``t0_avg`` and
``time_dist`` in the structured layout ``lib.set_light`` and the driver's ``--light_lut_filename`` load (``synth.lut_dtype``).

* ``read`` / ``validate`` / ``dump``: the geometry file, JSON ``{"box": [Lu, Lv, Lw], "detectors": [{"wall": "u0", "lo": [a, b],
  "hi": [a, b]}, ..]}`` (standard library only).  ``wall`` is one of u0, u1, v0, v1, w0, w1; ``lo`` / ``hi`` are in the wall's two
  in-plane coordinates in cyclic axis order (u walls: (v, w); v walls: (w, u); w walls: (u, v)); the detector's LUT index is its
  position in the list.  ``tile_wall`` lays a regular grid of tiles on a wall, ``box_from_consts`` gives a TPC's padded extents
  (the frame ``lightLUT.get_voxel`` maps positions into: borders padded by 0.02 cm, x mirrored in odd TPCs, y flipped -- the
  mapping is not the builder's business).
* ``build`` / ``trace``: the GPU walk (``ldsim_light_lut_build`` / ``ldsim_light_lut_trace``); ``to_lut``: the table.
* ``trace_twin``: the same walk in numpy from numpy-made keyed draws (``rng.keyed_block_uniforms``), operation for operation.
* ``solid_angle_visibility``: the closed form a pure-geometry table is checked against.
"""
import ctypes as C
import json
import math

import numpy as np

from . import rng as R

WALLS = ("u0", "u1", "v0", "v1", "w0", "w1")
GROUP_VELOCITY_CM_NS = 13.4          # a literature value for 128 nm in LAr: a parameter, not a claim
MAX_DETECTORS, MAX_NPROF = 1024, 512      # include/ldsim.h LDSIM_LUT_MAX_DETECTORS, LDSIM_LUT_MAX_NPROF
FATE_BULK, FATE_WALL, FATE_TRUNCATED = -1, -2, -3
TWO_PI = 6.283185307179586


class GeometryError(ValueError):
    pass


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def wall_index(wall):
    if isinstance(wall, str):
        if wall not in WALLS:
            raise GeometryError(f"unknown wall {wall!r}: one of {', '.join(WALLS)}")
        return WALLS.index(wall)
    if isinstance(wall, (int, np.integer)) and 0 <= int(wall) < 6:
        return int(wall)
    raise GeometryError(f"unknown wall {wall!r}: one of {', '.join(WALLS)}")


def detector(wall, lo, hi):
    return {"wall": WALLS[wall_index(wall)], "lo": [float(lo[0]), float(lo[1])], "hi": [float(hi[0]), float(hi[1])]}


def wall_extents(wall, box):
    """extents of the wall's two in-plane coordinates (cyclic axis order)"""
    a = wall_index(wall) // 2
    return float(box[(a + 1) % 3]), float(box[(a + 2) % 3])


def validate(geometry):
    """Checks a geometry {"box", "detectors"}; raises GeometryError naming the entry.  Returns (box (3,) f8, detectors as a list
    of (wall index, lo (2,), hi (2,)))."""
    if not isinstance(geometry, dict) or "box" not in geometry or "detectors" not in geometry:
        raise GeometryError('geometry: needs the keys "box" and "detectors"')
    try:
        box = [float(v) for v in geometry["box"]]
    except (TypeError, ValueError):
        raise GeometryError(f'box: three lengths in cm, got {geometry["box"]!r}') from None
    if len(box) != 3 or not all(math.isfinite(v) and v > 0 for v in box):
        raise GeometryError(f"box: three finite lengths > 0 in cm, got {box}")
    dets = geometry["detectors"]
    if not isinstance(dets, (list, tuple)) or not 1 <= len(dets) <= MAX_DETECTORS:
        raise GeometryError(f"detectors: a list of 1 .. {MAX_DETECTORS} rectangles")
    out = []
    for i, d in enumerate(dets):
        if not isinstance(d, dict) or not {"wall", "lo", "hi"} <= set(d):
            raise GeometryError(f'detectors[{i}]: needs "wall", "lo" and "hi"')
        try:
            w = wall_index(d["wall"])
        except GeometryError as e:
            raise GeometryError(f"detectors[{i}]: {e}") from None
        try:
            lo, hi = [float(v) for v in d["lo"]], [float(v) for v in d["hi"]]
        except (TypeError, ValueError):
            raise GeometryError(f"detectors[{i}]: lo and hi are two numbers each") from None
        if len(lo) != 2 or len(hi) != 2 or not all(math.isfinite(v) for v in lo + hi):
            raise GeometryError(f"detectors[{i}]: lo and hi are two finite numbers each")
        ext = wall_extents(w, box)
        for c in range(2):
            if not lo[c] < hi[c]:
                raise GeometryError(f"detectors[{i}]: zero-sized rectangle (lo[{c}] = {lo[c]}, hi[{c}] = {hi[c]})")
            if lo[c] < 0 or hi[c] > ext[c]:
                raise GeometryError(f"detectors[{i}]: [{lo[c]}, {hi[c]}) lies off wall {WALLS[w]}, which spans [0, {ext[c]}] cm "
                                    f"in coordinate {c}")
        for j, (w2, lo2, hi2) in enumerate(out):
            if w2 == w and lo2[0] < hi[0] and lo[0] < hi2[0] and lo2[1] < hi[1] and lo[1] < hi2[1]:
                raise GeometryError(f"detectors[{i}]: overlaps detectors[{j}] on wall {WALLS[w]}")
        out.append((w, lo, hi))
    return np.array(box), out


def read(path):
    with open(path) as f:
        g = json.load(f)
    validate(g)
    return g


def dump(path, geometry):
    validate(geometry)
    with open(path, "w") as f:
        json.dump({"box": [float(v) for v in geometry["box"]], "detectors": list(geometry["detectors"])}, f, indent=1)


def tile_wall(wall, n_a, n_b, box, gap=0.0):
    """n_a x n_b equal tiles on ``wall`` of ``box``, ``gap`` cm between neighbours and to the wall's edges; first coordinate
    slowest"""
    ea, eb = wall_extents(wall, box)
    n_a, n_b, gap = int(n_a), int(n_b), float(gap)
    if n_a < 1 or n_b < 1 or gap < 0:
        raise GeometryError("tile_wall: n_a, n_b >= 1 and gap >= 0")
    sa, sb = (ea - (n_a + 1) * gap) / n_a, (eb - (n_b + 1) * gap) / n_b
    if not (sa > 0 and sb > 0):
        raise GeometryError(f"tile_wall: gap {gap} cm leaves no room for {n_a} x {n_b} tiles on wall {WALLS[wall_index(wall)]}")
    out = []
    for i in range(n_a):
        for j in range(n_b):
            la, lb = gap + i * (sa + gap), gap + j * (sb + gap)
            out.append(detector(wall, (la, lb), (min(la + sa, ea), min(lb + sb, eb))))
    return out


def box_from_consts(itpc=0):
    """extents (cm) of the frame ``lightLUT.get_voxel`` divides into voxels for TPC ``itpc``: its borders padded by 0.02 cm"""
    from . import consts
    b = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)[int(itpc)]
    return [float(abs(b[k, 1] - b[k, 0]) + 4e-2) for k in range(3)]


# ---- parameters -------------------------------------------------------------------------------------------------------------
def params(rayleigh_cm=math.inf, absorption_cm=math.inf, group_velocity_cm_ns=GROUP_VELOCITY_CM_NS, wall_reflectivity=0.0,
           emit_mode=0, max_steps=1000, nprof=100):
    """the walk's parameters as a dict; ``wall_reflectivity``: one value for all walls or six (u0 u1 v0 v1 w0 w1);
    ``emit_mode``: 0 / "volume" emits uniformly in the voxel (right for nearest-voxel lookup), 1 / "centre" at its centre
    (right for ``light_lut_interp 1``)"""
    rho = [float(wall_reflectivity)] * 6 if np.ndim(wall_reflectivity) == 0 else [float(v) for v in wall_reflectivity]
    mode = {"volume": 0, "centre": 1, "center": 1}.get(emit_mode, emit_mode)
    p = {"rayleigh_cm": float(rayleigh_cm), "absorption_cm": float(absorption_cm),
         "group_velocity_cm_ns": float(group_velocity_cm_ns), "wall_reflectivity": rho, "emit_mode": mode,
         "max_steps": int(max_steps), "nprof": int(nprof)}
    validate_params(p)
    return p


def validate_params(p):
    if not (p["rayleigh_cm"] > 0 and p["absorption_cm"] > 0):
        raise GeometryError("rayleigh_cm and absorption_cm: lengths > 0 (inf allowed)")
    if not (math.isfinite(p["group_velocity_cm_ns"]) and p["group_velocity_cm_ns"] > 0):
        raise GeometryError("group_velocity_cm_ns: a finite velocity > 0")
    rho = p["wall_reflectivity"]
    if len(rho) != 6:
        raise GeometryError("wall_reflectivity: one value or six (u0 u1 v0 v1 w0 w1)")
    for w, v in zip(WALLS, rho):
        if not 0 <= v < 1:
            raise GeometryError(f"wall_reflectivity[{w}] = {v}: must lie in [0, 1) (a wall that absorbs nothing never ends a walk)")
    if p["emit_mode"] not in (0, 1):
        raise GeometryError('emit_mode: 0 / "volume" or 1 / "centre"')
    if p["max_steps"] < 1:
        raise GeometryError("max_steps: >= 1")
    if not 1 <= p["nprof"] <= MAX_NPROF:
        raise GeometryError(f"nprof: 1 .. {MAX_NPROF} bins of 1 ns")


def _pack(geometry, p):
    from .abi import LdsimLutBuildParams, LdsimLutDetector
    box, dets = validate(geometry)
    validate_params(p)
    P = LdsimLutBuildParams()
    P.box[:] = list(box)
    P.rayleigh_cm, P.absorption_cm, P.group_velocity_cm_ns = p["rayleigh_cm"], p["absorption_cm"], p["group_velocity_cm_ns"]
    P.wall_reflectivity[:] = p["wall_reflectivity"]
    P.emit_mode, P.max_steps, P.nprof = p["emit_mode"], p["max_steps"], p["nprof"]
    D = (LdsimLutDetector * len(dets))()
    for k, (w, lo, hi) in enumerate(dets):
        D[k].wall = w
        D[k].lo[:] = lo
        D[k].hi[:] = hi
    return P, D


# ---- the GPU walk -----------------------------------------------------------------------------------------------------------
def build(geometry, vox_div, n_photons, seed, p=None, voxel_range=None, ctx=None):
    """Tallies of ``n_photons`` photons from each voxel of ``voxel_range`` (linear indices [begin, end); default: all) of the grid
    ``vox_div``: {"count" u4 [nv, ndet], "hist" u4 [nv, ndet, nprof], "tmin" f4 [nv, ndet] (+inf where nothing arrived),
    "tsum" u8 [nv, ndet] (sum of llrint(1024 t)), "fates" u8 [nv, 3] (absorbed in the bulk, at a wall, truncated),
    "voxel_range", "n_photons"}.  The same integers at any slicing of the voxel range: slices concatenate (``concatenate``)."""
    from . import lib
    p = params() if p is None else p
    P, D = _pack(geometry, p)
    nx, ny, nz = (int(v) for v in vox_div)
    nvox = nx * ny * nz
    vb, ve = (0, nvox) if voxel_range is None else (int(voxel_range[0]), int(voxel_range[1]))
    nv, nd, nprof = max(ve - vb, 0), len(D), p["nprof"]
    out = {"count": np.zeros((nv, nd), dtype=np.uint32), "hist": np.zeros((nv, nd, nprof), dtype=np.uint32),
           "tmin": np.zeros((nv, nd), dtype=np.float32), "tsum": np.zeros((nv, nd), dtype=np.uint64),
           "fates": np.zeros((nv, 3), dtype=np.uint64), "voxel_range": (vb, ve), "n_photons": int(n_photons)}
    ctx = ctx or lib.context(refresh_consts=False)
    lib.check(lib.load().ldsim_light_lut_build(
        ctx, C.byref(P), D, C.c_int32(nd), C.c_int32(nx), C.c_int32(ny), C.c_int32(nz), C.c_int64(vb), C.c_int64(ve),
        C.c_int64(int(n_photons)), C.c_uint64(int(seed) & R.MASK64), lib.ptr(out["count"]), lib.ptr(out["hist"]),
        lib.ptr(out["tmin"]), lib.ptr(out["tsum"]), lib.ptr(out["fates"])))
    return out


def build_ms(ctx=None):
    """HIP-event time (ms) of the last build's kernel"""
    from . import lib
    ms = C.c_double()
    lib.check(lib.load().ldsim_light_lut_build_ms(ctx or lib.context(refresh_consts=False), C.byref(ms)))
    return ms.value


def concatenate(parts):
    """tallies of consecutive voxel ranges as one"""
    parts = sorted(parts, key=lambda t: t["voxel_range"][0])
    for a, b in zip(parts, parts[1:]):
        if a["voxel_range"][1] != b["voxel_range"][0] or a["n_photons"] != b["n_photons"]:
            raise ValueError("concatenate: the voxel ranges must follow one another, at one photon count")
    out = {k: np.concatenate([t[k] for t in parts]) for k in ("count", "hist", "tmin", "tsum", "fates")}
    out["voxel_range"] = (parts[0]["voxel_range"][0], parts[-1]["voxel_range"][1])
    out["n_photons"] = parts[0]["n_photons"]
    return out


def trace(geometry, vox_div, voxel, photon_range, seed, p=None, ctx=None):
    """Per photon [begin, end) of one voxel: {"fate" i4 (detector index, or -1 absorbed in the bulk, -2 at a wall, -3 truncated),
    "steps" i4, "time" f8 (ns), "end" f8 [n, 3]}"""
    from . import lib
    p = params() if p is None else p
    P, D = _pack(geometry, p)
    nx, ny, nz = (int(v) for v in vox_div)
    b, e = int(photon_range[0]), int(photon_range[1])
    n = max(e - b, 0)
    out = {"fate": np.zeros(n, dtype=np.int32), "steps": np.zeros(n, dtype=np.int32), "time": np.zeros(n),
           "end": np.zeros((n, 3))}
    ctx = ctx or lib.context(refresh_consts=False)
    lib.check(lib.load().ldsim_light_lut_trace(
        ctx, C.byref(P), D, C.c_int32(len(D)), C.c_int32(nx), C.c_int32(ny), C.c_int32(nz), C.c_int64(int(voxel)), C.c_int64(b),
        C.c_int64(e), C.c_uint64(int(seed) & R.MASK64), lib.ptr(out["fate"]), lib.ptr(out["steps"]), lib.ptr(out["time"]),
        lib.ptr(out["end"])))
    return out


# ---- the table --------------------------------------------------------------------------------------------------------------
def tally(tr, ndet, nprof):
    """the build's tallies of one voxel from per-photon fates and times (``trace`` or ``trace_twin`` output), in numpy"""
    fate, t = np.asarray(tr["fate"]), np.asarray(tr["time"], dtype=np.float64)
    hit = fate >= 0
    f, t = fate[hit].astype(np.int64), t[hit]
    count = np.bincount(f, minlength=ndet).astype(np.uint32)
    b = np.minimum(np.floor(t), nprof - 1).astype(np.int64)
    hist = np.bincount(f * nprof + b, minlength=ndet * nprof).reshape(ndet, nprof).astype(np.uint32)
    tmin = np.full(ndet, np.inf, dtype=np.float32)
    np.minimum.at(tmin, f, t.astype(np.float32))
    tsum = np.zeros(ndet, dtype=np.uint64)
    np.add.at(tsum, f, np.rint(1024.0 * t).astype(np.int64).astype(np.uint64))
    fates = np.array([(fate == FATE_BULK).sum(), (fate == FATE_WALL).sum(), (fate == FATE_TRUNCATED).sum()], dtype=np.uint64)
    return {"count": count, "hist": hist, "tmin": tmin, "tsum": tsum, "fates": fates}


def to_lut(tallies, vox_div=None):
    """The structured table (``synth.lut_dtype(nprof)``): vis = count / n_photons; t0 = tmin, 0 where nothing arrived (like real
    tables); t0_avg = tsum / 1024 / count; time_dist = hist / count, zeros where nothing arrived.  Shape (nx, ny, nz, ndet) with
    ``vox_div`` (the tallies must cover the whole grid), else (nv, ndet)."""
    from .synth import lut_dtype
    count = np.asarray(tallies["count"])
    hist = np.asarray(tallies["hist"])
    nv, nd, nprof = hist.shape
    lut = np.zeros((nv, nd), dtype=lut_dtype(nprof))
    lit = count > 0
    safe = np.where(lit, count, 1).astype(np.float64)
    lut["vis"] = count / float(tallies["n_photons"])
    lut["t0"] = np.where(lit, np.asarray(tallies["tmin"], dtype=np.float32), np.float32(0))
    lut["t0_avg"] = np.where(lit, np.asarray(tallies["tsum"]).astype(np.float64) / 1024.0 / safe, 0.0)
    lut["time_dist"] = hist / safe[..., None]
    if vox_div is not None:
        nx, ny, nz = (int(v) for v in vox_div)
        if nv != nx * ny * nz:
            raise ValueError(f"to_lut: tallies of {nv} voxels do not fill a ({nx}, {ny}, {nz}) grid")
        lut = lut.reshape(nx, ny, nz, nd)
    return lut


# ---- the numpy twin ---------------------------------------------------------------------------------------------------------
def rayleigh_mu(u):
    """exact inverse of the (1 + mu^2) law: q = 4u - 2, A = cbrt(q + sqrt(q^2 + 1)), mu = A - 1/A"""
    q = 4.0 * np.asarray(u, dtype=np.float64) - 2.0
    A = np.cbrt(q + np.sqrt(q * q + 1.0))
    return np.minimum(np.maximum(A - 1.0 / A, -1.0), 1.0)


def lambert_cos(u):
    return np.sqrt(np.asarray(u, dtype=np.float64))


def trace_twin(geometry, vox_div, voxel, photon_range, seed, p=None):
    """``trace`` on the host: the kernel's walk (lut_emit / lut_step of csrc/kernels_lutbuild.hip) operation for operation in f64,
    over all photons at once, from numpy-made keyed draws"""
    p = params() if p is None else p
    box, dets = validate(geometry)
    validate_params(p)
    nx, ny, nz = (int(v) for v in vox_div)
    grid = np.array([nx, ny, nz])
    seed = int(seed) & R.MASK64
    b, e = int(photon_range[0]), int(photon_range[1])
    n = max(e - b, 0)
    L = box
    vsize = L / grid
    rate = 1.0 / p["rayleigh_cm"] + 1.0 / p["absorption_cm"]
    lam_t = 1.0 / rate if rate > 0 else math.inf
    lam_inf = math.isinf(lam_t)
    p_abs = 0.0 if lam_inf else lam_t / p["absorption_cm"]
    inv_vg = 1.0 / p["group_velocity_cm_ns"]
    rho = np.array(p["wall_reflectivity"])
    by_wall = [[(i, lo, hi) for i, (w, lo, hi) in enumerate(dets) if w == wall] for wall in range(6)]
    key = R.key_mix(R.key_mix(np.uint64(R.KEY_ROOT), np.full(n, int(voxel), dtype=np.int64)), np.arange(b, e, dtype=np.int64))
    iv = np.array([int(voxel) // nz // ny, int(voxel) // nz % ny, int(voxel) % nz])
    x0 = R.keyed_block_uniforms(seed, R.TAG_LUT, key, 0).astype(np.float64)
    x = R.keyed_block_uniforms(seed, R.TAG_LUT, key, 1).astype(np.float64)
    pos = np.empty((n, 3))
    for k in range(3):
        lo = float(iv[k]) * vsize[k]
        q = np.full(n, lo + 0.5 * vsize[k]) if p["emit_mode"] else lo + x0[:, k] * vsize[k]
        pos[:, k] = np.minimum(np.maximum(q, 0.0), L[k])
    mu = 1.0 - 2.0 * x0[:, 3]
    phi = TWO_PI * x[:, 0]
    s = np.sqrt(np.maximum(0.0, 1.0 - mu * mu))
    d = np.stack([s * np.cos(phi), s * np.sin(phi), mu], axis=1)
    path = np.zeros(n)
    fate = np.full(n, -100, dtype=np.int32)
    steps = np.zeros(n, dtype=np.int32)
    act = np.arange(n)
    step = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while len(act) and step < p["max_steps"]:
            ua, ub, uc = x[act, 1], x[act, 2], x[act, 3]
            xn = R.keyed_block_uniforms(seed, R.TAG_LUT, key[act], 2 + step).astype(np.float64)
            ue = xn[:, 0]
            step += 1
            steps[act] = step
            P, D = pos[act], d[act]
            l = np.full(len(act), np.inf) if lam_inf else -lam_t * np.log(ua)
            dw = np.full(len(act), np.inf)
            axis = np.zeros(len(act), dtype=np.int64)
            far = np.zeros(len(act), dtype=bool)
            for k in range(3):
                t = np.full(len(act), np.inf)
                pl, mi = D[:, k] > 0, D[:, k] < 0
                t[pl] = np.maximum((L[k] - P[pl, k]) / D[pl, k], 0.0)
                t[mi] = np.maximum(P[mi, k] / -D[mi, k], 0.0)
                less = t < dw
                dw = np.where(less, t, dw)
                axis = np.where(less, k, axis)
                far = np.where(less, D[:, k] > 0, far)
            phi = TWO_PI * ue
            cp, sp = np.cos(phi), np.sin(phi)
            bulk = l < dw
            newfate = np.full(len(act), -100, dtype=np.int32)
            # bulk interaction
            lb = np.where(bulk, l, 0.0)
            Pb = P + lb[:, None] * D
            absorbed = bulk & (ub <= p_abs)
            newfate[absorbed] = FATE_BULK
            mu = rayleigh_mu(uc)
            st = np.sqrt(np.maximum(0.0, 1.0 - mu * mu))
            dx, dy, dz = D[:, 0], D[:, 1], D[:, 2]
            polar = np.abs(dz) > 0.99999
            den = np.sqrt(1.0 - dz * dz)
            nxv = np.where(polar, st * cp, st * (dx * dz * cp - dy * sp) / den + dx * mu)
            nyv = np.where(polar, st * sp, st * (dy * dz * cp + dx * sp) / den + dy * mu)
            nzv = np.where(polar, np.where(dz > 0, mu, -mu), -st * cp * den + dz * mu)
            nn = np.sqrt(nxv * nxv + nyv * nyv + nzv * nzv)
            Db = np.stack([nxv / nn, nyv / nn, nzv / nn], axis=1)
            # wall hit
            wl = np.where(bulk, 0.0, dw)
            Pw = P + wl[:, None] * D
            a1, a2 = (axis + 1) % 3, (axis + 2) % 3
            rows = np.arange(len(act))
            pa, pb = Pw[rows, a1], Pw[rows, a2]
            Pw[rows, axis] = np.where(far, L[axis], 0.0)
            wall = 2 * axis + far
            hitdet = np.full(len(act), -1, dtype=np.int64)
            for w in range(6):
                on = ~bulk & (wall == w)
                for i, lo, hi in by_wall[w]:
                    inside = on & (hitdet < 0) & (lo[0] <= pa) & (pa < hi[0]) & (lo[1] <= pb) & (pb < hi[1])
                    hitdet[inside] = i
            det = ~bulk & (hitdet >= 0)
            newfate[det] = hitdet[det]
            lost = ~bulk & ~det & ~(ub <= rho[wall])
            newfate[lost] = FATE_WALL
            ct, sl = np.sqrt(uc), np.sqrt(1.0 - uc)
            dn, da, db = np.where(far, -ct, ct), sl * cp, sl * sp
            Dw = np.empty_like(D)
            Dw[rows, axis], Dw[rows, a1], Dw[rows, a2] = dn, da, db
            # commit
            pos[act] = np.where(bulk[:, None], Pb, Pw)
            path[act] = path[act] + np.where(bulk, l, dw)
            d[act] = np.where(bulk[:, None], Db, Dw)
            fate[act] = newfate
            x[act] = xn
            act = act[newfate == -100]
    fate[act] = FATE_TRUNCATED
    return {"fate": fate, "steps": steps, "time": path * inv_vg, "end": pos}


# ---- closed form ------------------------------------------------------------------------------------------------------------
def solid_angle(point, det, box):
    """solid angle (sr) of a wall rectangle seen from ``point`` inside the box: with height h above the wall and corner offsets
    A0, A1, B0, B1 of the rectangle from the point's foot, Omega = f(A1, B1) - f(A0, B1) - f(A1, B0) + f(A0, B0),
    f(a, b) = atan(a b / (h sqrt(h^2 + a^2 + b^2)))"""
    w = wall_index(det["wall"])
    axis, far = w // 2, w % 2
    pt = [float(v) for v in point]
    h = (float(box[axis]) - pt[axis]) if far else pt[axis]
    pa, pb = pt[(axis + 1) % 3], pt[(axis + 2) % 3]
    A0, A1 = det["lo"][0] - pa, det["hi"][0] - pa
    B0, B1 = det["lo"][1] - pb, det["hi"][1] - pb

    def f(a, b):
        return math.atan(a * b / (h * math.sqrt(h * h + a * a + b * b)))
    return f(A1, B1) - f(A0, B1) - f(A1, B0) + f(A0, B0)


def solid_angle_visibility(point, det, box):
    """the fraction Omega / 4 pi of isotropically emitted photons that reach the rectangle directly"""
    return solid_angle(point, det, box) / (4.0 * math.pi)
