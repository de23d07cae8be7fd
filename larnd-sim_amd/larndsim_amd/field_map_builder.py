"""Drift-field map builder: the map ``--field_map`` consumes, from a space-charge density and wall potentials of one TPC
(csrc/kernels_fmapbuild.hip; include/ldsim.h states the model).

One TPC is one box in the simulation frame (cm, z the drift coordinate) with a node grid ``dims = (nx, ny, nz)`` whose first and
last nodes lie on the faces; ``n = sign(z_cathode - z_anode)``, ``q = |z - z_anode|``.  kV, kV/cm, source ``s = rho / eps`` in
kV/cm^2.

* Potential: ``E = E0 n z^ - grad psi``; ``laplace psi = -s`` inside, ``psi`` given on the six faces (0: conducting anode and
  cathode, ideally graded cage; anything else: a cage defect).  7-point stencil, ``A psi = b`` with
  ``(A psi)(c) = sum_a (2 psi(c) - psi(c - e_a) - psi(c + e_a)) / h_a^2``.
* Field at the nodes: central differences, one-sided three-point on the faces; ``Ex, Ey, En = E0 - n dpsi/dz, |E|``.
* Paths: an electron moves with ``-mu(|E|, T) E``; by ``s = q_node - q``: ``dx/ds = -Ex/En``, ``dy/ds = -Ey/En``,
  ``dtau/ds = v_drift / (mu(|E|) En) - 1`` with ``tau = v_drift t - s``; trilinear field, classical RK4 in
  ``N = max(1, ceil(q_node / step))`` equal steps.  A positive charge cloud pulls electrons towards it.
* Channels: ``E = |E|`` at the node, ``dx, dy`` end point minus node, ``dz = n tau(q_node)`` (``|z + dz - z_anode| / v_drift`` is
  the path's drift time), ``flags`` = 1 where the end point left the box sideways.

``params`` / ``validate`` / ``box_from_consts``: the build's parameters.  ``source_from_density``, ``cosmic_source``: sources.
``solve`` / ``trace`` / ``build`` / ``build_ms``: the GPU.  ``solve_twin`` (a direct solve by a type-I sine transform, independent
of the iterative method), ``field_twin``, ``trace_twin``, ``build_twin``: numpy, in any float type (``np.longdouble``), no GPU.
"""
import ctypes as C
import math

import numpy as np

MAX_STEPS = 1048576                # include/ldsim.h LDSIM_FIELD_MAP_BUILD_MAX_STEPS
EPS0_F_PER_CM = 8.8541878128e-14   # vacuum permittivity, C / (V cm)
# Literature values, parameters of the model and no claims about a detector: the rate at which cosmic rays leave ion charge in
# liquid argon at the surface, about 2e-10 C/m^3/s (Palestini et al., arXiv:2011.07292 quote 1.6e-10 to 2e-10), and the mobility
# of the positive ions, for which measurements between 8e-4 and 2e-3 cm^2/V/s are in use (ICARUS assumed 1.6e-3).
COSMIC_ION_RATE = 2.0e-16          # C / cm^3 / s
ION_MOBILITY = 1.6e-3              # cm^2 / V / s


class FieldMapBuildError(ValueError):
    pass


# ---- parameters -------------------------------------------------------------------------------------------------------------
def box_from_consts(tpc, pitch=1.0):
    """origin, spacing, dims, z_anode, z_cathode of TPC ``tpc`` of the loaded ``consts``, the node pitch as close to ``pitch`` (cm)
    as a whole number of cells per axis allows: ``n = max(2, round(extent / pitch) + 1)``"""
    from . import consts
    borders = np.asarray(consts.detector.TPC_BORDERS, dtype=np.float64)
    if not 0 <= int(tpc) < len(borders):
        raise FieldMapBuildError(f"tpc: {tpc} outside [0, {len(borders)})")
    if not (math.isfinite(pitch) and pitch > 0):
        raise FieldMapBuildError(f"pitch: a finite node pitch > 0 in cm, got {pitch}")
    b = borders[int(tpc)]
    lo, hi = b.min(axis=1), b.max(axis=1)
    dims = tuple(max(2, int(round((hi[a] - lo[a]) / pitch)) + 1) for a in range(3))
    spacing = tuple(float((hi[a] - lo[a]) / (dims[a] - 1)) for a in range(3))
    return {"origin": tuple(float(v) for v in lo), "spacing": spacing, "dims": dims, "z_anode": float(b[2][0]),
            "z_cathode": float(b[2][1])}


def params(origin, spacing, dims, z_anode, z_cathode, E0=None, temperature=None, mobility=None, tol=1e-12, max_iters=20000,
           step=None, check_every=32):
    """The build's parameters as a dict.  Defaults from the loaded ``consts``: ``E0`` E_FIELD, ``temperature`` TEMPERATURE,
    ``mobility`` ELECTRON_MOBILITY_PARAMS; ``step`` hz / 2."""
    from . import consts
    det = consts.detector
    try:
        origin, spacing, dims = tuple(float(v) for v in origin), tuple(float(v) for v in spacing), tuple(int(v) for v in dims)
    except (TypeError, ValueError) as e:
        raise FieldMapBuildError(f"origin, spacing, dims: three numbers each ({e})")
    if not (len(origin) == len(spacing) == len(dims) == 3):
        raise FieldMapBuildError("origin, spacing, dims: three numbers each")
    mobility = det.ELECTRON_MOBILITY_PARAMS if mobility is None else mobility
    p = {"origin": origin, "spacing": spacing, "dims": dims, "z_anode": float(z_anode), "z_cathode": float(z_cathode),
         "E0": float(det.E_FIELD if E0 is None else E0),
         "temperature": float(det.TEMPERATURE if temperature is None else temperature),
         "mobility": tuple(float(v) for v in mobility), "tol": float(tol), "max_iters": int(max_iters),
         "step": float(spacing[2] / 2 if step is None else step), "check_every": int(check_every)}
    validate(p)
    return p


def validate(p):
    """raises FieldMapBuildError naming the entry"""
    for a, ax in enumerate("xyz"):
        if not (math.isfinite(p["spacing"][a]) and p["spacing"][a] > 0):
            raise FieldMapBuildError(f"spacing: a finite pitch > 0 along {ax}, got {p['spacing'][a]}")
        if not math.isfinite(p["origin"][a]):
            raise FieldMapBuildError(f"origin: a finite position along {ax}, got {p['origin'][a]}")
        if p["dims"][a] < 2:
            raise FieldMapBuildError(f"dims: every dimension >= 2, got {p['dims']}")
    if p["dims"][0] * p["dims"][1] * p["dims"][2] > 2 ** 31 - 1:
        raise FieldMapBuildError(f"dims: {p['dims']} is more than 2^31 - 1 nodes")
    for k, what in (("E0", "field"), ("temperature", "temperature"), ("tol", "tolerance"), ("step", "step")):
        if not (math.isfinite(p[k]) and p[k] > 0):
            raise FieldMapBuildError(f"{k}: a finite {what} > 0, got {p[k]}")
    if len(p["mobility"]) != 6 or not all(math.isfinite(v) for v in p["mobility"]) or p["mobility"][0] == 0:
        raise FieldMapBuildError(f"mobility: six finite parameters, the first other than 0, got {p['mobility']}")
    if not (math.isfinite(p["z_anode"]) and math.isfinite(p["z_cathode"])):
        raise FieldMapBuildError(f"z_anode, z_cathode: finite planes, got {p['z_anode']}, {p['z_cathode']}")
    if p["z_anode"] == p["z_cathode"]:
        raise FieldMapBuildError(f"z_anode: equal to z_cathode ({p['z_anode']}), the drift direction is undefined")
    z_lo, z_hi = p["origin"][2], p["origin"][2] + (p["dims"][2] - 1) * p["spacing"][2]
    slack = 1e-6 * p["spacing"][2]
    if max(abs(min(p["z_anode"], p["z_cathode"]) - z_lo), abs(max(p["z_anode"], p["z_cathode"]) - z_hi)) > slack:
        raise FieldMapBuildError(f"z_anode, z_cathode: ({p['z_anode']}, {p['z_cathode']}) are not the grid's z faces "
                                 f"({z_lo}, {z_hi})")
    if p["max_iters"] < 1:
        raise FieldMapBuildError(f"max_iters: a count >= 1, got {p['max_iters']}")
    if p["check_every"] < 1:
        raise FieldMapBuildError(f"check_every: a count >= 1, got {p['check_every']}")
    if (p["dims"][2] - 1) * p["spacing"][2] / p["step"] > MAX_STEPS:
        raise FieldMapBuildError(f"step: {p['step']} cm makes more than {MAX_STEPS} steps on the longest path")


def _array(p, a, name, dtype=np.float64):
    a = np.asarray(a)
    if a.shape != tuple(p["dims"]):
        raise FieldMapBuildError(f"{name}: shape {a.shape}, the grid is {tuple(p['dims'])}")
    if not np.all(np.isfinite(a)):
        raise FieldMapBuildError(f"{name}: holds a non-finite value")
    return np.ascontiguousarray(a, dtype=dtype)


def _boundary(p, boundary, dtype=np.float64):
    """psi with the face values of ``boundary`` (None: 0) and zeros inside"""
    psi = np.zeros(p["dims"], dtype=dtype)
    if boundary is not None:
        b = _array(p, boundary, "boundary", dtype)
        psi[...] = b
        psi[1:-1, 1:-1, 1:-1] = 0
    return psi


def _pack(p):
    from .abi import LdsimFieldMapBuildParams
    validate(p)
    P = LdsimFieldMapBuildParams()
    P.origin[:], P.spacing[:], P.n[:], P.mobility[:] = p["origin"], p["spacing"], p["dims"], p["mobility"]
    P.z_anode, P.z_cathode, P.e0, P.temperature = p["z_anode"], p["z_cathode"], p["E0"], p["temperature"]
    P.tol, P.step, P.max_iters, P.check_every = p["tol"], p["step"], p["max_iters"], p["check_every"]
    return P


def drift_sign(p):
    return 1.0 if p["z_cathode"] > p["z_anode"] else -1.0


def drift_coordinate(p, dtype=np.float64):
    """q of the nz node planes"""
    ft = np.dtype(dtype).type
    z = ft(p["origin"][2]) + np.arange(p["dims"][2]).astype(dtype) * ft(p["spacing"][2])
    return np.abs(z - ft(p["z_anode"]))


# ---- sources ----------------------------------------------------------------------------------------------------------------
def source_from_density(rho_C_per_cm3, eps_r=1.505):
    """s = rho / (eps_r eps_0) in kV/cm^2 from a charge density in C/cm^3 (eps_r: liquid argon)"""
    return np.asarray(rho_C_per_cm3, dtype=np.float64) / (eps_r * EPS0_F_PER_CM) * 1e-3


def cosmic_source(p, ion_rate=COSMIC_ION_RATE, ion_mobility=ION_MOBILITY, eps_r=1.505):
    """The source of the steady-state, first-order space charge of cosmic rays: ions made at ``ion_rate`` (C/cm^3/s) everywhere
    drift to the cathode at ``ion_mobility`` (cm^2/V/s) times E0, so rho(q) = ion_rate q / (ion_mobility E0).  The ions' effect
    on their own drift is not in it."""
    if not (math.isfinite(ion_rate) and ion_rate >= 0):
        raise FieldMapBuildError(f"ion_rate: a finite rate >= 0 in C/cm^3/s, got {ion_rate}")
    if not (math.isfinite(ion_mobility) and ion_mobility > 0):
        raise FieldMapBuildError(f"ion_mobility: a finite mobility > 0 in cm^2/V/s, got {ion_mobility}")
    v_ion = ion_mobility * p["E0"] * 1e3                  # cm/s (E0 in kV/cm)
    rho = ion_rate * drift_coordinate(p) / v_ion
    return np.ascontiguousarray(np.broadcast_to(source_from_density(rho, eps_r), p["dims"]))


# ---- the GPU ----------------------------------------------------------------------------------------------------------------
def solve(p, source, boundary=None, ctx=None):
    """(psi, iterations, relative residual) by the conjugate-gradient kernels (``ldsim_field_map_solve``)"""
    from . import lib
    P = _pack(p)
    s = _array(p, source, "source")
    psi = _boundary(p, boundary)
    it, res = C.c_int32(), C.c_double()
    ctx = ctx or lib.context(refresh_consts=False)
    lib.check(lib.load().ldsim_field_map_solve(ctx, C.byref(P), lib.ptr(s), lib.ptr(psi), C.byref(it), C.byref(res)))
    return psi, it.value, res.value


def trace(p, psi, ctx=None):
    """{"E", "dx", "dy", "dz", "flags"} of the potential ``psi`` by fb_field_kernel and fb_trace_kernel (``ldsim_field_map_trace``)"""
    from . import lib
    P = _pack(p)
    psi = _array(p, psi, "psi")
    out = {k: np.zeros(p["dims"], dtype=np.float64) for k in ("E", "dx", "dy", "dz")}
    out["flags"] = np.zeros(p["dims"], dtype=np.uint8)
    ctx = ctx or lib.context(refresh_consts=False)
    lib.check(lib.load().ldsim_field_map_trace(ctx, C.byref(P), lib.ptr(psi), lib.ptr(out["E"]), lib.ptr(out["dx"]),
                                               lib.ptr(out["dy"]), lib.ptr(out["dz"]), lib.ptr(out["flags"])))
    return out


def _as_map(p, ch):
    return {"origin": np.asarray(p["origin"], dtype=np.float64), "spacing": np.asarray(p["spacing"], dtype=np.float64),
            "E": ch["E"], "dx": ch["dx"], "dy": ch["dy"], "dz": ch["dz"]}


def build(p, source, boundary=None, ctx=None, info=None):
    """The map of one TPC on the GPU, as the dict ``field_map.validate`` accepts for a TPC.  ``info``: a dict that receives
    ``iterations``, ``residual``, ``flags`` and ``psi``."""
    psi, it, res = solve(p, source, boundary, ctx)
    ch = trace(p, psi, ctx)
    if info is not None:
        info.update(iterations=it, residual=res, flags=ch["flags"], psi=psi)
    return _as_map(p, ch)


def build_ms(ctx=None):
    """HIP-event times (ms) of the last solve, field kernel and trace kernel"""
    from . import lib
    ms = (C.c_double * 3)()
    lib.check(lib.load().ldsim_field_map_build_ms(ctx or lib.context(refresh_consts=False), ms))
    return tuple(ms)


# ---- the numpy restatement --------------------------------------------------------------------------------------------------
def stencil_eigenvalues(p):
    """the eigenvalues of A as three 1-D arrays to be added: 4 / h^2 sin^2(pi m / (2 (n - 1))), m = 1 .. n - 2"""
    return [4.0 / p["spacing"][a] ** 2 * np.sin(np.pi * np.arange(1, p["dims"][a] - 1) / (2.0 * (p["dims"][a] - 1))) ** 2
            for a in range(3)]


def lambda_min(p):
    """the smallest eigenvalue of A (every dimension >= 3)"""
    return float(sum(4.0 / p["spacing"][a] ** 2 * math.sin(math.pi / (2.0 * (p["dims"][a] - 1))) ** 2 for a in range(3)))


def rhs(p, source, boundary=None):
    """b on the interior nodes, shape (nx - 2, ny - 2, nz - 2): the source and the face values moved to the right"""
    s = _array(p, source, "source")
    psi = _boundary(p, boundary)
    b = s[1:-1, 1:-1, 1:-1].copy()
    ih2 = [1.0 / h ** 2 for h in p["spacing"]]
    if b.size:
        b[0, :, :] += psi[0, 1:-1, 1:-1] * ih2[0]
        b[-1, :, :] += psi[-1, 1:-1, 1:-1] * ih2[0]
        b[:, 0, :] += psi[1:-1, 0, 1:-1] * ih2[1]
        b[:, -1, :] += psi[1:-1, -1, 1:-1] * ih2[1]
        b[:, :, 0] += psi[1:-1, 1:-1, 0] * ih2[2]
        b[:, :, -1] += psi[1:-1, 1:-1, -1] * ih2[2]
    return b


def relative_residual(p, source, psi):
    """|b - A psi|_2 / |b|_2 of a potential whose face nodes hold the boundary values (0 when b = 0)"""
    s, psi = _array(p, source, "source"), _array(p, psi, "psi")
    c = psi[1:-1, 1:-1, 1:-1]
    if not c.size:
        return 0.0
    ih2 = [1.0 / h ** 2 for h in p["spacing"]]
    r = s[1:-1, 1:-1, 1:-1] - ((2 * c - psi[:-2, 1:-1, 1:-1] - psi[2:, 1:-1, 1:-1]) * ih2[0]
                                + (2 * c - psi[1:-1, :-2, 1:-1] - psi[1:-1, 2:, 1:-1]) * ih2[1]
                                + (2 * c - psi[1:-1, 1:-1, :-2] - psi[1:-1, 1:-1, 2:]) * ih2[2])
    bound = psi.copy()
    bound[1:-1, 1:-1, 1:-1] = 0
    bn = float(np.sqrt((rhs(p, source, bound) ** 2).sum()))
    return float(np.sqrt((r ** 2).sum())) / bn if bn > 0 else 0.0


def solve_twin(p, source, boundary=None):
    """psi (f64, all nodes) by diagonalising A with the type-I sine transform: a direct solve of the same discrete system"""
    from scipy.fft import dstn, idstn
    validate(p)
    psi = _boundary(p, boundary)
    b = rhs(p, source, boundary)
    if b.size and np.any(b != 0):
        lx, ly, lz = stencil_eigenvalues(p)
        lam = lx[:, None, None] + ly[None, :, None] + lz[None, None, :]
        psi[1:-1, 1:-1, 1:-1] = idstn(dstn(b, type=1) / lam, type=1)
    return psi


def mobility(p, e, dtype=np.float64):
    """mu(E, T) in cm^2/kV/us in the kernel's order of operations (``consts.electron_mobility`` with E sqrt(E) for E^1.5)"""
    ft = np.dtype(dtype).type
    a = [ft(v) for v in p["mobility"]]
    e = np.asarray(e, dtype=dtype)
    r = ft(p["temperature"]) / ft(89)
    tc = ft(1) / (r * np.sqrt(r))
    se, e2 = np.sqrt(e), e * e
    num = ((a[0] + a[1] * e) + a[2] * (e * se)) + a[3] * (e2 * se)
    den = ((ft(1) + (a[1] / a[0]) * e) + a[4] * e2) + a[5] * (e2 * e)
    return ((num / den) * tc) * ft(1e-3)


def v_drift(p, dtype=np.float64):
    return np.dtype(dtype).type(p["E0"]) * mobility(p, p["E0"], dtype)


def _deriv(psi, axis, h, ft):
    n = psi.shape[axis]
    ih = ft(1) / ft(h)

    def sl(s):
        return tuple(s if a == axis else slice(None) for a in range(3))
    d = np.empty_like(psi)
    if n == 2:
        d[...] = (psi[sl(slice(1, 2))] - psi[sl(slice(0, 1))]) * ih
        return d
    hih = ft(0.5) * ih
    d[sl(slice(1, -1))] = (psi[sl(slice(2, None))] - psi[sl(slice(0, -2))]) * hih
    lo, hi = psi[sl(slice(0, 1))], psi[sl(slice(-1, None))]
    d[sl(slice(0, 1))] = (ft(4) * (psi[sl(slice(1, 2))] - lo) - (psi[sl(slice(2, 3))] - lo)) * hih
    d[sl(slice(-1, None))] = ((psi[sl(slice(-3, -2))] - hi) - ft(4) * (psi[sl(slice(-2, -1))] - hi)) * hih
    return d


def field_twin(p, psi, dtype=np.float64):
    """(Ex, Ey, En, |E|) at the nodes, in ``dtype``"""
    validate(p)
    ft = np.dtype(dtype).type
    psi = _array(p, psi, "psi", dtype)
    ex = -_deriv(psi, 0, p["spacing"][0], ft)
    ey = -_deriv(psi, 1, p["spacing"][1], ft)
    en = ft(p["E0"]) - ft(drift_sign(p)) * _deriv(psi, 2, p["spacing"][2], ft)
    em = np.where((ex == 0) & (ey == 0), np.abs(en), np.sqrt((ex * ex + ey * ey) + en * en))
    return ex, ey, en, em


def field_at(p, field, x, y, q, dtype=np.float64):
    """(Ex, Ey, En, |E|) at the points (x, y, z_anode + n q): the trilinear interpolation of the node values ``field`` (the tuple
    ``field_twin`` returns, or ``stack_field`` of it), a + f (b - a) along z, then y, then x, coordinates clamped to the grid"""
    ft = np.dtype(dtype).type
    x, y, q = np.broadcast_arrays(np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(q, dtype=dtype))
    pos = (x, y, ft(p["z_anode"]) + ft(drift_sign(p)) * q)
    nx, ny, nz = p["dims"]
    cell, w = [], []
    for a in range(3):
        u = (pos[a] - ft(p["origin"][a])) * (ft(1) / ft(p["spacing"][a]))
        u = np.minimum(np.maximum(u, ft(0)), ft(p["dims"][a] - 1))
        c = np.minimum(u.astype(np.int64), p["dims"][a] - 2)
        cell.append(c)
        w.append(u - c.astype(dtype))
    base = (cell[0] * ny + cell[1]) * nz + cell[2]
    f = field if isinstance(field, np.ndarray) else stack_field(field)
    w = [v[..., None] for v in w]
    c = [f[base + (((t >> 2) & 1) * ny * nz + ((t >> 1) & 1) * nz + (t & 1))] for t in range(8)]
    c00, c01 = c[0] + w[2] * (c[1] - c[0]), c[2] + w[2] * (c[3] - c[2])
    c10, c11 = c[4] + w[2] * (c[5] - c[4]), c[6] + w[2] * (c[7] - c[6])
    a0, a1 = c00 + w[1] * (c01 - c00), c10 + w[1] * (c11 - c10)
    out = a0 + w[0] * (a1 - a0)
    return out[..., 0], out[..., 1], out[..., 2], out[..., 3]


def stack_field(field):
    """the node records (Ex, Ey, En, |E|) as one array [nodes][4], as the trace kernel reads them"""
    return np.ascontiguousarray(np.stack([np.asarray(ch).reshape(-1) for ch in field], axis=-1))


def path_rhs(p, field, x, y, q, dtype=np.float64):
    """(dx/ds, dy/ds, dtau/ds, En) at (x, y, q), s = q_node - q"""
    ft = np.dtype(dtype).type
    ex, ey, en, em = field_at(p, field, x, y, q, dtype)
    with np.errstate(all="ignore"):
        return -(ex / en), -(ey / en), v_drift(p, dtype) / (mobility(p, em, dtype) * en) - ft(1), en


def trace_twin(p, psi, dtype=np.float64, on_reverse="raise"):
    """{"E", "dx", "dy", "dz", "flags"} by the same RK4 in numpy, in ``dtype``.  The step counts N are those of f64, whatever ``dtype``.  ``on_reverse="mask"`` returns the nodes whose path met En <= 0 as ``reversed`` instead of
    raising FieldMapBuildError."""
    validate(p)
    ft = np.dtype(dtype).type
    nodes = field_twin(p, psi, dtype)
    field = stack_field(nodes)
    nx, ny, nz = p["dims"]
    x0 = (ft(p["origin"][0]) + np.arange(nx).astype(dtype) * ft(p["spacing"][0]))[:, None] + np.zeros((nx, ny), dtype=dtype)
    y0 = (ft(p["origin"][1]) + np.arange(ny).astype(dtype) * ft(p["spacing"][1]))[None, :] + np.zeros((nx, ny), dtype=dtype)
    qs, qs64 = drift_coordinate(p, dtype), drift_coordinate(p)
    out = {k: np.zeros(p["dims"], dtype=dtype) for k in ("dx", "dy", "dz")}
    out["E"] = nodes[3].copy()
    rev = np.zeros(p["dims"], dtype=bool)
    end = np.zeros(p["dims"] + (2,), dtype=dtype)
    for k in range(nz):
        qn = qs[k]
        x, y, tau = x0.copy(), y0.copy(), np.zeros((nx, ny), dtype=dtype)
        if qs64[k] > 0:
            n_steps = int(max(1.0, math.ceil(float(qs64[k]) / p["step"])))
            ds = qn / ft(n_steps)
            hds, ds6 = ft(0.5) * ds, ds / ft(6)
            for s in range(n_steps):
                q0, qh, q1 = qn - ft(s) * ds, qn - (ft(s) + ft(0.5)) * ds, qn - (ft(s) + ft(1)) * ds
                with np.errstate(all="ignore"):
                    k1 = path_rhs(p, field, x, y, q0, dtype)
                    k2 = path_rhs(p, field, x + hds * k1[0], y + hds * k1[1], qh, dtype)
                    k3 = path_rhs(p, field, x + hds * k2[0], y + hds * k2[1], qh, dtype)
                    k4 = path_rhs(p, field, x + ds * k3[0], y + ds * k3[1], q1, dtype)
                    for kk in (k1, k2, k3, k4):
                        rev[:, :, k] |= ~(kk[3] > 0)
                    x = x + ds6 * (((k1[0] + ft(2) * k2[0]) + ft(2) * k3[0]) + k4[0])
                    y = y + ds6 * (((k1[1] + ft(2) * k2[1]) + ft(2) * k3[1]) + k4[1])
                    tau = tau + ds6 * (((k1[2] + ft(2) * k2[2]) + ft(2) * k3[2]) + k4[2])
        out["dx"][:, :, k], out["dy"][:, :, k], out["dz"][:, :, k] = x - x0, y - y0, ft(drift_sign(p)) * tau
        end[:, :, k, 0], end[:, :, k, 1] = x, y
    lo = [ft(p["origin"][a]) for a in range(2)]
    hi = [ft(p["origin"][a]) + ft(p["dims"][a] - 1) * ft(p["spacing"][a]) for a in range(2)]   # the last node's own coordinate
    out["flags"] = ((end[..., 0] < lo[0]) | (end[..., 0] > hi[0]) | (end[..., 1] < lo[1]) | (end[..., 1] > hi[1])).astype(np.uint8)
    if on_reverse == "mask":
        out["reversed"] = rev
    elif rev.any():
        node = int(np.flatnonzero(rev.reshape(-1))[0])
        raise FieldMapBuildError(f"source: field reverses on the path of node {node} "
                                 f"(i, j, k) = {tuple(int(v) for v in np.unravel_index(node, p['dims']))}: En <= 0")
    return out


def build_twin(p, source, boundary=None, dtype=np.float64, info=None):
    """``build`` in numpy: the direct solve, then the field and the paths in ``dtype`` (the channels are returned as f64)"""
    psi = solve_twin(p, source, boundary)
    ch = trace_twin(p, psi, dtype)
    if info is not None:
        info.update(iterations=0, residual=relative_residual(p, source, psi), flags=ch["flags"], psi=psi)
    return _as_map(p, {k: np.ascontiguousarray(ch[k], dtype=np.float64) for k in ("E", "dx", "dy", "dz")})
