"""SiPM correlated noise of the light leg (``ChargeChain.set_sipm_noise``, ``simulate_pixels.py --sipm_crosstalk`` ...): the
numpy restatement of ``light_sipm_count_kernel`` (csrc/light_wvfm.hip), operation for operation in float64 and taking the draws
as arrays, the analytic moments of what it draws, and the wrapper of the stage call ``ldsim_sipm_stat_fluctuations``.

Per element (idet, itick) of a rate array x [n_det][n_ticks] (PE per us), with tick = LIGHT_TICK_SIZE, from the keyed stream
(stage tag ``rng.TAG_LIGHT_FLUCT``, key ``element_keys``); "Poisson(m, i)" is ``poisson`` on draw i:

    n_p = Poisson(x tick, 0)                                     primaries: the draw of the stage with the noise off
    n_d = Poisson(dark_rate tick, 1)                             dark counts, also where x <= 0
    g_0 = n_p + n_d,  g_{k+1} = Poisson(crosstalk g_k, 2 + k)    prompt cross-talk by generations, until g_k = 0 or k = 31
    N = sum of g_k
    n_ap = Binomial(N, afterpulse)                               ``charge_stats.binomial`` on normal 34 and uniform 35
    after-pulse j lands on tick itick + 1 + floor(-afterpulse_tau log(u_j) / tick),  u_j = uniform 64 + j
    count[idet][t] = N of the element + the after-pulses that landed on it;  output = float32(1 / tick * count)

Draw-index table: 0 primaries | 1 dark counts | 2 .. 33 cross-talk generations 0 .. 31 | 34, 35 after-pulse binomial (normal,
uniform) | 36 .. 63 unused | 64 + j delay of after-pulse j.

Stated simplifications: an after-pulse has full amplitude (no cell recovery), starts no cross-talk and no after-pulse of its own
(first order only), and is dropped when it lands at or beyond n_ticks; dark counts exist only inside the tick window of a
simulated sub-batch (the empty group's waveforms get none); truth slots are untouched (in the reference too they come from the
unfluctuated sums).
"""
import ctypes as C

import numpy as np

from . import charge_stats, lib, rng

MAX_GENERATIONS = 32
DRAW_PRIMARY, DRAW_DARK, DRAW_CASCADE, DRAW_AP_Z, DRAW_AP_U, DRAW_DELAY = 0, 1, 2, 34, 35, 64
N_FIXED_DRAWS = 36           # draws 0 .. 35: everything but the delays
POISSON_NORMAL_MIN = 30.0    # mean from which ``poisson`` truncates a normal
FIELDS = ("crosstalk", "afterpulse", "afterpulse_tau", "dark_rate")
AFTERPULSE_TAU_DEFAULT = 0.1


def params(crosstalk=0.0, afterpulse=0.0, afterpulse_tau=AFTERPULSE_TAU_DEFAULT, dark_rate=0.0):
    """the four constants as the dict the functions below take"""
    return dict(crosstalk=float(crosstalk), afterpulse=float(afterpulse), afterpulse_tau=float(afterpulse_tau),
                dark_rate=float(dark_rate))


def check(p, tick=None):
    """the ranges of ``ldsim_set_sipm_noise``; raises ValueError naming the field"""
    if not 0 <= p["crosstalk"] <= 0.5:
        raise ValueError(f"crosstalk {p['crosstalk']:g} must lie in [0, 0.5]")
    if not 0 <= p["afterpulse"] <= 0.5:
        raise ValueError(f"afterpulse {p['afterpulse']:g} must lie in [0, 0.5]")
    if p["afterpulse"] > 0 and not (np.isfinite(p["afterpulse_tau"]) and p["afterpulse_tau"] > 0):
        raise ValueError(f"afterpulse_tau {p['afterpulse_tau']:g} us must be finite and > 0 when afterpulse > 0")
    if not (np.isfinite(p["dark_rate"]) and p["dark_rate"] >= 0) or (tick is not None and not p["dark_rate"] * tick < 30):
        raise ValueError(f"dark_rate {p['dark_rate']:g} per us must be finite, >= 0 and below 30 per tick")
    return p


def element_keys(call_key, n_det, n_ticks):
    """stream key of every element, [n_det][n_ticks] uint64: key_mix(key_mix(call key, idet), itick)"""
    rows = rng.key_mix(np.uint64(int(call_key) & rng.MASK64), np.arange(n_det, dtype=np.int64))
    return rng.key_mix(rows[:, None], np.arange(n_ticks, dtype=np.int64)[None, :])


def poisson(mean, u, z):
    """``poisson_int32`` (csrc/light_wvfm.hip) per element, from one uniform draw ``u`` and one normal draw ``z`` (float32 as
    the device draws them): mean <= 0 gives 0; mean < 30 is inverted with u (x counts up while u > the running sum s of
    p = exp(-mean), p mean / 1, ..., stopping where s no longer grows); otherwise trunc(z sqrt(mean) + mean) clamped at 0.
    Returns int64."""
    mean, u, z = (np.array(a, dtype=np.float64) for a in np.broadcast_arrays(mean, u, z))
    out = np.zeros(mean.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        big = mean >= POISSON_NORMAL_MIN
        v = np.trunc(z * np.sqrt(mean) + mean)
        out[big] = np.maximum(v[big], 0.0).astype(np.int64)
        inv = np.flatnonzero((mean > 0) & ~big)
        m, ui = mean.flat[inv], u.flat[inv]
        x = np.zeros(len(inv))
        p = np.exp(-m)
        s = p.copy()
        go = ui > s
        while go.any():
            x = np.where(go, x + 1, x)
            p = np.where(go, p * m / np.maximum(x, 1.0), p)
            s_new = np.where(go, s + p, s)
            go = go & (s_new != s) & (ui > s_new)
            s = s_new
    out.flat[inv] = x.astype(np.int64)
    return out


def cascade(g0, crosstalk, uniforms, normals):
    """total progeny N of ``g0`` first avalanches per element under prompt cross-talk: g_{k+1} = Poisson(crosstalk g_k) on draw
    2 + k of ``uniforms`` / ``normals`` [n][>= 34], until no element has a generation left or after 32 generations.  Returns
    (N, generations drawn) as int64."""
    g = np.asarray(g0, dtype=np.int64).ravel().copy()
    un, zn = np.asarray(uniforms).reshape(len(g), -1), np.asarray(normals).reshape(len(g), -1)
    total, gens = g.copy(), np.zeros(len(g), dtype=np.int64)
    for k in range(MAX_GENERATIONS):
        live = g > 0
        if not live.any():
            break
        nxt = poisson(float(crosstalk) * g[live].astype(np.float64), un[live, DRAW_CASCADE + k], zn[live, DRAW_CASCADE + k])
        g = np.zeros_like(g)
        g[live] = nxt
        total += g
        gens += live
    return total, gens


def avalanches(rate, tick, p, uniforms, normals):
    """steps 1-4 without the delays, from draws 0 .. 35: dict of int64 [n_det][n_ticks] ``n_p``, ``n_d``, ``N`` and ``n_ap``"""
    x = np.asarray(rate, dtype=np.float32)
    shape = x.shape
    x = x.astype(np.float64).ravel()
    un, zn = np.asarray(uniforms).reshape(len(x), -1), np.asarray(normals).reshape(len(x), -1)
    if un.shape[1] < N_FIXED_DRAWS or zn.shape[1] < N_FIXED_DRAWS:
        raise ValueError(f"the cascade and the after-pulse binomial read draws 0 .. {N_FIXED_DRAWS - 1} of every stream")
    n_p = np.where(x > 0, poisson(np.where(x > 0, x * tick, 0.0), un[:, DRAW_PRIMARY], zn[:, DRAW_PRIMARY]), 0)
    n_d = poisson(np.full(len(x), p["dark_rate"] * tick), un[:, DRAW_DARK], zn[:, DRAW_DARK])
    N, _ = cascade(n_p + n_d, p["crosstalk"], un, zn)
    n_ap = charge_stats.binomial(N.astype(np.float64), p["afterpulse"], zn[:, DRAW_AP_Z], un[:, DRAW_AP_U]).astype(np.int64)
    return {k: v.reshape(shape) for k, v in dict(n_p=n_p, n_d=n_d, N=N, n_ap=n_ap).items()}


def counts(rate, tick, p, uniforms, normals, detail=False):
    """The kernel's avalanche counts, int64 [n_det][n_ticks], from ``rate`` [n_det][n_ticks] (float32 as the stage reads it),
    the constants ``p`` (``params``) and the draws of every element's stream, ``uniforms`` / ``normals`` [n_det * n_ticks][nd]
    (or [n_det][n_ticks][nd]) with nd >= 36 and, for the delays, nd >= 64 + the largest n_ap (``avalanches`` tells it from the
    first 36).  ``detail``: also the dict of ``avalanches`` with ``dropped`` (after-pulses beyond the row end, per element) and
    ``delay_ticks`` (landing tick - itick of every after-pulse, kept or dropped, as one flat float64 array per element order)."""
    x = np.asarray(rate, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("rate must be [n_det][n_ticks]")
    n_det, n_ticks = x.shape
    a = avalanches(x, tick, p, uniforms, normals)
    un = np.asarray(uniforms).reshape(n_det * n_ticks, -1)
    n_ap = a["n_ap"].ravel()
    need = DRAW_DELAY + int(n_ap.max(initial=0))
    if n_ap.any() and un.shape[1] < need:
        raise ValueError(f"the after-pulse delays read uniform draws up to {need - 1}: {un.shape[1]} given")
    count = a["N"].astype(np.int64).copy()
    dropped = np.zeros(n_det * n_ticks, dtype=np.int64)
    delays = []
    idet, itick = np.divmod(np.arange(n_det * n_ticks), n_ticks)
    tau = p["afterpulse_tau"]
    for j in range(int(n_ap.max(initial=0))):
        e = np.flatnonzero(n_ap > j)
        with np.errstate(all="ignore"):
            d = np.floor(-tau * np.log(un[e, DRAW_DELAY + j].astype(np.float64)) / tick)
        keep = d < (n_ticks - 1 - itick[e]).astype(np.float64)
        np.add.at(count, (idet[e[keep]], itick[e[keep]] + 1 + d[keep].astype(np.int64)), 1)
        np.add.at(dropped, e[~keep], 1)
        delays.append((e, d + 1))
    if not detail:
        return count
    order = np.argsort(np.concatenate([e for e, _ in delays]) if delays else np.zeros(0, dtype=np.int64), kind="stable")
    a["dropped"] = dropped.reshape(n_det, n_ticks)
    a["delay_ticks"] = (np.concatenate([d for _, d in delays]) if delays else np.zeros(0))[order]
    return count, a


def to_rate(count, tick):
    """the stage's conversion: float32(1 / tick * float64(count))"""
    return (1.0 / tick * np.asarray(count, dtype=np.float64)).astype(np.float32)


# ---- analytic moments ------------------------------------------------------------------------------------------------------------
def progeny_mean_variance(mu, crosstalk):
    """mean and variance of the total progeny N of Poisson(mu) primaries (mu < 30: drawn by inversion) under cross-talk
    ``crosstalk`` = lambda, no dark counts or after-pulses: a Poisson number of Borel(lambda) trees, mean mu / (1 - lambda) and
    variance mu / (1 - lambda)^3.  The 32-generation cap changes these by less than lambda^32 of mu."""
    mu, lam = np.asarray(mu, dtype=np.float64), float(crosstalk)
    return mu / (1 - lam), mu / (1 - lam) ** 3


def afterpulse_mean_factor(afterpulse):
    """after-pulses multiply the mean count of a whole, long row by 1 + p, up to what falls off its end"""
    return 1.0 + float(afterpulse)


def mean_delay(afterpulse_tau, tick):
    """mean of (landing tick - itick) tick [us] of an after-pulse that is not cut by the row end: the delay D ~ Exp(tau) lands
    1 + floor(D / tick) ticks later, and E floor(D / tick) = q / (1 - q) with q = exp(-tick / tau), so the mean is
    tick / (1 - q) = tau + tick / 2 + tick^2 / (12 tau) - ..."""
    return tick / -np.expm1(-tick / afterpulse_tau)


# ---- the stage call -------------------------------------------------------------------------------------------------------------
def stat_fluctuations(rate, counts=False, ctx=None):
    """``ldsim_sipm_stat_fluctuations``: the fluctuation stage on ``rate`` [n_det][n_ticks] under the context's current call
    key (rows keyed by their index), with the SiPM noise when ``ChargeChain.set_sipm_noise`` enabled it; keyed mode only.
    Returns the fluctuated float32 rate, with ``counts`` (noise enabled only) also the int32 avalanche counts."""
    x = np.ascontiguousarray(rate, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("rate must be [n_det][n_ticks]")
    out = np.zeros_like(x)
    cnt = np.zeros(x.shape, dtype=np.int32) if counts else None
    lib.check(lib.load().ldsim_sipm_stat_fluctuations(ctx or lib.context(), lib.ptr(x), C.c_int32(x.shape[0]),
                                                     C.c_int32(x.shape[1]), lib.ptr(out), lib.ptr(cnt)))
    return (out, cnt) if counts else out
