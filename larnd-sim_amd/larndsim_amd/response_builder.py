"""Field-response builder: the induction table of a pixelated anode by the Shockley-Ramo theorem (csrc/kernels_respbuild.hip;
include/ldsim.h states the model).

The anode is the plane ``z = 0``.  A pixel is a square pad of side ``pad_size <= PIXEL_PITCH`` centred on its pitch cell; all the
rest of the plane (the other pads, the gaps) is grounded, the cathode is far away and the drift field uniform, so an electron at
transverse offset ``(x, y)`` from the pad centre moves straight down at ``V_DRIFT``.  The pad's weighting potential is the solid
angle it subtends over 2 pi::

    phi(x, y, z) = 1 / (2 pi) sum_{sx = +-1} sum_{sy = +-1} sx sy atan2(X Y, z sqrt(X^2 + Y^2 + z^2)),  X = x + sx a, Y = y + sy a,

``a = pad_size / 2`` (at ``z = 0``: 1 over the pad, 0 off it, 1/2 on an edge, 1/4 on a corner).  The charge induced between two
instants is the difference of phi at the two positions (Ramo), so a table entry -- the tick average of the current per unit
charge -- is exact, without a derivative::

    z_e(m) = V_DRIFT max(0, (arrival_tick + 1/2) dt - (m - 1/2) dt)                   tick edges m = 0 .. K
    phibar(i, j, m) = mean over n_sub x n_sub midpoints x = (i + (p + 1/2) / n_sub) b, y = (j + (q + 1/2) / n_sub) b of phi(x, y, z_e(m))
    R[i, j, k] = (phibar(i, j, k + 1) - phibar(i, j, k)) / dt

in the convention ``detsim.get_closest_waveform`` reads: bin ``i`` stands for ``|x|`` in ``[i b, (i + 1) b)``, tick ``k`` for ``t``
in ``[(k - 1/2) dt, (k + 1/2) dt)``.  The charge reaches the plane at the upper edge of tick ``arrival_tick``; entries after it are
exactly 0, and a bin's entries sum to ``(phibar(z = 0) - phibar(z_e(0))) / dt``: 1 / dt less the start height's potential for a bin
over the pad.  With ``pad_size < PIXEL_PITCH`` the charge that lands on the gaps is lost: field focusing onto the pads is not
modelled.

* ``params`` / ``validate``: the build's parameters, defaults from the loaded ``consts``.
* ``build`` / ``build_ms``: the table on the GPU (``ldsim_response_build``).
* ``weighting_potential``, ``twin``: the numpy restatement of the formulae above, in any float type (``np.longdouble``).
"""
import ctypes as C
import math

import numpy as np

MAX_K, MAX_NSUB = 7679, 16      # include/ldsim.h LDSIM_RESPONSE_BUILD_MAX_K, LDSIM_RESPONSE_BUILD_MAX_NSUB


class ResponseBuildError(ValueError):
    pass


# ---- parameters -------------------------------------------------------------------------------------------------------------
def default_arrival_tick(time_window=None, sampling=None):
    """floor(TIME_WINDOW / RESPONSE_SAMPLING) - 1: ``tracks_current`` looks up 0 < t < TIME_WINDOW only, so a charge slice reads
    ticks 0 .. n or 1 .. n + 1 (n = floor(TIME_WINDOW / dt) - 1) by its sub-tick phase; with the arrival at the edge n + 1/2 both
    sets hold the whole collection"""
    from . import consts
    tw = consts.detector.TIME_WINDOW if time_window is None else time_window
    dt = consts.detector.RESPONSE_SAMPLING if sampling is None else sampling
    return int(math.floor(float(tw) / float(dt) + 1e-9)) - 1


def params(pad_size=None, n_sub=4, shape=None, arrival_tick=None, pitch=None, bin_size=None, v_drift=None, sampling=None,
           time_window=None):
    """The build's parameters as a dict.  Defaults from the loaded ``consts``: ``pitch`` PIXEL_PITCH, ``pad_size`` the pitch,
    ``bin_size`` RESPONSE_BIN_SIZE, ``v_drift`` V_DRIFT, ``sampling`` RESPONSE_SAMPLING, ``shape`` (45, 45, 1950) at a sampling of
    0.1 us and above, else (45, 45, 3800) (the shapes of the reference's files), ``arrival_tick`` ``default_arrival_tick``."""
    from . import consts
    det = consts.detector
    pitch = float(det.PIXEL_PITCH if pitch is None else pitch)
    sampling = float(det.RESPONSE_SAMPLING if sampling is None else sampling)
    if shape is None:
        shape = (45, 45, 1950) if sampling >= 0.1 - 1e-12 else (45, 45, 3800)
    if len(shape) != 3:
        raise ResponseBuildError(f"shape: three counts (I, J, K), got {tuple(shape)!r}")
    if arrival_tick is None:
        if not sampling > 0:
            raise ResponseBuildError(f"sampling: a finite tick > 0 in us, got {sampling}")
        arrival_tick = default_arrival_tick(det.TIME_WINDOW if time_window is None else time_window, sampling)
    p = {"pad_size": pitch if pad_size is None else float(pad_size), "pitch": pitch,
         "bin_size": float(det.RESPONSE_BIN_SIZE if bin_size is None else bin_size),
         "v_drift": float(det.V_DRIFT if v_drift is None else v_drift), "sampling": sampling,
         "n_i": int(shape[0]), "n_j": int(shape[1]), "n_k": int(shape[2]), "n_sub": int(n_sub), "arrival_tick": int(arrival_tick)}
    validate(p)
    return p


def validate(p):
    """raises ResponseBuildError naming the entry"""
    for k, what in (("pitch", "size"), ("bin_size", "size"), ("v_drift", "velocity"), ("sampling", "tick")):
        if not (math.isfinite(p[k]) and p[k] > 0):
            raise ResponseBuildError(f"{k}: a finite {what} > 0, got {p[k]}")
    if not (math.isfinite(p["pad_size"]) and 0 < p["pad_size"] <= p["pitch"]):
        raise ResponseBuildError(f"pad_size: must lie in (0, pitch = {p['pitch']}] cm, got {p['pad_size']}")
    for k in ("n_i", "n_j", "n_k"):
        if p[k] < 1:
            raise ResponseBuildError(f"{k}: a count >= 1, got {p[k]}")
    if p["n_k"] > MAX_K:
        raise ResponseBuildError(f"n_k: {p['n_k']} ticks exceed the kernel's capacity, a row of n_k + 1 tick edges in LDS: "
                                 f"n_k <= {MAX_K}")
    if p["n_i"] * p["n_j"] > 2 ** 31 - 1:
        raise ResponseBuildError(f"n_i, n_j: {p['n_i']} x {p['n_j']} rows exceed one launch (2^31 - 1)")
    if not 1 <= p["n_sub"] <= MAX_NSUB:
        raise ResponseBuildError(f"n_sub: 1 .. {MAX_NSUB} sub-samples per bin and axis, got {p['n_sub']}")
    if not 0 <= p["arrival_tick"] < p["n_k"]:
        raise ResponseBuildError(f"arrival_tick: must lie in [0, n_k = {p['n_k']}), got {p['arrival_tick']}")


def _pack(p):
    from .abi import LdsimResponseBuildParams
    validate(p)
    P = LdsimResponseBuildParams()
    P.pad_size, P.bin_size, P.v_drift, P.sampling = p["pad_size"], p["bin_size"], p["v_drift"], p["sampling"]
    P.n_i, P.n_j, P.n_k, P.n_sub, P.arrival_tick = p["n_i"], p["n_j"], p["n_k"], p["n_sub"], p["arrival_tick"]
    return P


# ---- the GPU build ----------------------------------------------------------------------------------------------------------
def build(p, ctx=None):
    """the table, f64 (n_i, n_j, n_k), from response_build_kernel: what ``lib.set_response`` and the driver's ``--response_file``
    take"""
    from . import lib
    P = _pack(p)
    table = np.zeros((p["n_i"], p["n_j"], p["n_k"]), dtype=np.float64)
    ctx = ctx or lib.context(refresh_consts=False)
    lib.check(lib.load().ldsim_response_build(ctx, C.byref(P), lib.ptr(table)))
    return table


def build_ms(ctx=None):
    """HIP-event time (ms) of the last build's kernel"""
    from . import lib
    ms = C.c_double()
    lib.check(lib.load().ldsim_response_build_ms(ctx or lib.context(refresh_consts=False), C.byref(ms)))
    return ms.value


# ---- the numpy restatement --------------------------------------------------------------------------------------------------
def weighting_potential(x, y, z, pad_size):
    """phi(x, y, z >= 0) of the square pad of side ``pad_size`` centred at the origin of the grounded plane z = 0; broadcasts, in
    the float type of its arguments"""
    x, y, z = np.asarray(x), np.asarray(y), np.asarray(z)
    ft = np.result_type(x, y, z, np.float64)
    x, y, z = x.astype(ft), y.astype(ft), z.astype(ft)
    a = ft.type(pad_size) / 2
    two_pi = 8 * np.arctan(ft.type(1))
    s = 0
    for sx in (-1, 1):
        for sy in (-1, 1):
            X, Y = x + sx * a, y + sy * a
            s = s + (sx * sy) * np.arctan2(X * Y, z * np.sqrt(X * X + Y * Y + z * z))
    return s / two_pi


def edge_heights(p, dtype=np.float64):
    """z_e(m) of the tick edges m = 0 .. n_k, cm"""
    ft = np.dtype(dtype).type
    dt, m = ft(p["sampling"]), np.arange(p["n_k"] + 1).astype(dtype)
    return ft(p["v_drift"]) * np.maximum(ft(0), (ft(p["arrival_tick"]) + ft(0.5)) * dt - (m - ft(0.5)) * dt)


def mean_potential(p, z, dtype=np.float64):
    """phibar(i, j, z) for the heights ``z`` (1-D): the mean of phi over the n_sub x n_sub midpoints of every bin, summed p outer,
    q inner; shape (n_i, n_j, len(z))"""
    ft = np.dtype(dtype).type
    n, b = p["n_sub"], ft(p["bin_size"])
    z = np.asarray(z, dtype=dtype).reshape(1, 1, -1)
    i = np.arange(p["n_i"]).astype(dtype).reshape(-1, 1, 1)
    j = np.arange(p["n_j"]).astype(dtype).reshape(1, -1, 1)
    acc = np.zeros((p["n_i"], p["n_j"], z.shape[-1]), dtype=dtype)
    for s in range(n):
        x = (i + (ft(s) + ft(0.5)) / ft(n)) * b
        for q in range(n):
            y = (j + (ft(q) + ft(0.5)) / ft(n)) * b
            acc += weighting_potential(x, y, z, ft(p["pad_size"]))
    return acc / ft(n * n)


def twin(p, dtype=np.float64):
    """the table from the formulae of the module's docstring in numpy, in ``dtype`` (f64, or ``np.longdouble`` as the more precise
    reference); touches no GPU"""
    validate(p)
    phibar = mean_potential(p, edge_heights(p, dtype), dtype)
    return (phibar[:, :, 1:] - phibar[:, :, :-1]) / np.dtype(dtype).type(p["sampling"])


def bins_over_pad(p):
    """number of bins per axis that lie wholly over the pad"""
    return int(math.floor(0.5 * p["pad_size"] / p["bin_size"] * (1 + 1e-12)))


def collection_only(p):
    """the table of a pad that sees nothing until the charge lands: 1 / dt at ``arrival_tick`` for the bins wholly over the pad, 0
    elsewhere -- the yardstick a built table's collected charge is compared with"""
    t = np.zeros((p["n_i"], p["n_j"], p["n_k"]))
    n = bins_over_pad(p)
    t[:n, :n, p["arrival_tick"]] = 1.0 / p["sampling"]
    return t
