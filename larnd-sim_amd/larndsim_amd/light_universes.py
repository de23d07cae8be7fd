"""
Light universes: a batch's light response run again under varied light constants (``ChargeChain.light_universes``,
``ldsim_dev_light_universes`` in include/ldsim.h).

After ``sum_light`` the photon sum of a batch is resident, and everything behind it -- scintillation profile, Poisson
fluctuations, SiPM response, triggers, digitised waveforms -- reads only that array and a handful of constants.  A *variation*
is the set of nine values one universe is run with -- absolute values, not deltas:

``photon_scale``
    multiplies the resident photon sum: light yield, ``W_PH``, ``SCINT_PRESCALE`` and a global efficiency in one number.  It is
    applied to the summed photons (one f4 rounding), not to ``n_photons`` before the f4 sums, so a universe is *not* bit-equal
    to a fresh run under a changed ``W_PH``
``singlet_fraction, tau_s, tau_t``
    ``SINGLET_FRACTION``, ``TAU_S``, ``TAU_T`` of ``consts.light``
``gain_scale``
    multiplies ``LIGHT_GAIN[row]`` (one f64 product per row)
``response_time, oscillation_period``
    ``LIGHT_RESPONSE_TIME``, ``LIGHT_OSCILLATION_PERIOD``; not read under ``SIPM_RESPONSE_MODEL 1``, where a value that differs
    from the configuration's is refused (a knob that does nothing is an error)
``trig_threshold_scale``
    multiplies every group threshold handed to ``light_sim.get_triggers_universe`` (host side)
``noise_scale``
    multiplies the detector-noise spectrum handed to ``light_sim.sim_triggers_universe`` (host side)

Every array of universe ``k`` equals, bit for bit, what ``ChargeChain.light_response`` gives on the scaled photon sum under
``consts.light`` patched to variation ``k`` and the same call key; with keyed streams all universes of a batch see the same random
numbers, so their differences are the constants' effect.  Truth slots are not produced per universe.

This module imports the standard library only (the driver's self-launching parent reads a universes file before numpy is
loaded); the dtypes are made on first use.
"""
import json
import math

MAX_UNIVERSES = 64                   # LDSIM_LIGHT_UNIVERSES_MAX

C_FIELDS = ("photon_scale", "singlet_fraction", "tau_s", "tau_t", "gain_scale", "response_time", "oscillation_period")
HOST_FIELDS = ("trig_threshold_scale", "noise_scale")
FIELDS = C_FIELDS + HOST_FIELDS      # the nine values; the first seven in the order of LdsimLightVariation

# key of a universes file / of variation() -> field: the constants' own names, and four names of this module
KEYS = {"PHOTON_SCALE": "photon_scale", "SINGLET_FRACTION": "singlet_fraction", "TAU_S": "tau_s", "TAU_T": "tau_t",
        "LIGHT_GAIN_SCALE": "gain_scale", "LIGHT_RESPONSE_TIME": "response_time",
        "LIGHT_OSCILLATION_PERIOD": "oscillation_period", "TRIG_THRESHOLD_SCALE": "trig_threshold_scale",
        "NOISE_SCALE": "noise_scale"}
CONST_OF = {"singlet_fraction": "SINGLET_FRACTION", "tau_s": "TAU_S", "tau_t": "TAU_T",
            "response_time": "LIGHT_RESPONSE_TIME", "oscillation_period": "LIGHT_OSCILLATION_PERIOD"}
SCALE_FIELDS = ("photon_scale", "gain_scale", "trig_threshold_scale", "noise_scale")     # nominal 1.0

# fixed columns of dataset light_universe_trig (file_rows adds op_channel i4 [channels of a trigger])
_TRIG_COLUMNS = [("universe", "u2"), ("event_id", "u4"), ("trigger_idx", "i8"), ("start_time", "f8"), ("trigger_type", "i4")]


def __getattr__(name):
    # FILE_UNIVERSE: dataset light_universes of the driver's file (one row per universe); FILE_TRIG: the fixed columns of
    # dataset light_universe_trig
    if name in ("FILE_UNIVERSE", "FILE_TRIG"):
        import numpy as np
        d = {"FILE_UNIVERSE": np.dtype([("name", "S64")] + [(f, "f8") for f in FIELDS]),
             "FILE_TRIG": np.dtype(_TRIG_COLUMNS)}
        globals().update(d)
        return d[name]
    raise AttributeError(name)


def nominal():
    """the variation that changes nothing: the values of ``consts.light``, every scale 1"""
    from . import consts
    v = {f: float(getattr(consts.light, c)) for f, c in CONST_OF.items()}
    v.update({f: 1.0 for f in SCALE_FIELDS})
    return {f: v[f] for f in FIELDS}


def _field_of(key):
    f = KEYS.get(str(key).upper())
    if f is None:
        raise ValueError(f"light universes: unknown key {key!r} (known: {', '.join(KEYS)})")
    return f


def variation(base=None, **changes):
    """``nominal()`` (or ``base``) with ``changes`` applied; keys are the constants' names (``SINGLET_FRACTION``, ``TAU_S``,
    ``TAU_T``, ``LIGHT_RESPONSE_TIME``, ``LIGHT_OSCILLATION_PERIOD``) and ``PHOTON_SCALE``, ``LIGHT_GAIN_SCALE``,
    ``TRIG_THRESHOLD_SCALE``, ``NOISE_SCALE``, in either letter case.  An unknown key is an error."""
    v = dict(nominal() if base is None else base)
    for k, x in changes.items():
        v[_field_of(k)] = x
    return v


def validate(variations, sipm_response_model=None, reference=None):
    """The argument rules of ``ldsim_dev_light_universes`` and of the two host-side fields, with the same key words: ValueError
    for a list that is not 1 to 64 long, a missing or unknown field, a value that is not finite or outside its range.  Under
    ``sipm_response_model`` 1 (None: ``consts.light.SIPM_RESPONSE_MODEL``) ``response_time`` and ``oscillation_period`` must
    equal those of ``reference`` (None: ``nominal()``)."""
    n = len(variations)
    if not (1 <= n <= MAX_UNIVERSES):
        raise ValueError(f"light universes: n = {n} universes, must lie in [1, {MAX_UNIVERSES}]")
    if sipm_response_model is None:
        from . import consts
        sipm_response_model = int(consts.light.SIPM_RESPONSE_MODEL)
    if sipm_response_model == 1 and reference is None:
        reference = nominal()
    rules = {"photon_scale": (lambda x: x > 0, "must be finite and > 0"),
             "singlet_fraction": (lambda x: 0 <= x <= 1, "must be finite and in [0, 1]"),
             "tau_s": (lambda x: x > 0, "must be finite and > 0"),
             "tau_t": (lambda x: x > 0, "must be finite and > 0"),
             "gain_scale": (lambda x: x != 0, "must be finite and != 0"),
             "response_time": (lambda x: x > 0, "must be finite and > 0"),
             "oscillation_period": (lambda x: x > 0, "must be finite and > 0"),
             "trig_threshold_scale": (lambda x: True, "must be finite"),
             "noise_scale": (lambda x: x >= 0, "must be finite and >= 0")}
    for k, v in enumerate(variations):
        missing = [f for f in FIELDS if f not in v]
        extra = [f for f in v if f not in FIELDS]
        if missing or extra:
            raise ValueError(f"light universes: universe {k}: missing fields {missing}, unknown key {extra}")
        for f in FIELDS:
            x = v[f]
            ok, rule = rules[f]
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or not ok(x):
                raise ValueError(f"light universes: universe {k}: {f} = {x!r} {rule}")
        if sipm_response_model == 1:
            for f in ("response_time", "oscillation_period"):
                if float(v[f]) != float(reference[f]):
                    raise ValueError(f"light universes: universe {k}: {f} = {v[f]!r} is not read under SIPM_RESPONSE_MODEL 1 "
                                     f"and differs from the configuration's ({reference[f]!r})")
    return variations


def parse(entries):
    """[(name, changes)] of a decoded universes file: a list of ``{"name": ..., "TAU_S": ..., ...}``; the keys other than
    ``name`` are checked here (unknown keys are an error), the values by ``validate`` once they are applied"""
    if not isinstance(entries, list) or not all(isinstance(e, dict) for e in entries):
        raise ValueError("light universes: the file must hold a JSON list of objects")
    if not (1 <= len(entries) <= MAX_UNIVERSES):
        raise ValueError(f"light universes: n = {len(entries)} universes, must lie in [1, {MAX_UNIVERSES}]")
    out = []
    for k, e in enumerate(entries):
        changes = {key: x for key, x in e.items() if key != "name"}
        for key in changes:
            if str(key).upper() not in KEYS:
                raise ValueError(f"light universes: universe {k}: unknown key {key!r} (known: name, {', '.join(KEYS)})")
        name = str(e.get("name", f"universe{k}"))
        if len(name.encode()) > 64:
            raise ValueError(f"light universes: universe {k}: name longer than 64 bytes")
        out.append((name, changes))
    return out


def read(path):
    """``parse`` of the JSON file ``path`` (standard library only: no constants needed)"""
    with open(path) as f:
        return parse(json.load(f))


def load(path):
    """(names, variations) of the universes file ``path``: every entry is ``nominal()`` (the constants loaded now) with the
    entry's keys applied, validated"""
    entries = read(path)
    names = [n for n, _ in entries]
    vs = [variation(**c) for _, c in entries]
    validate(vs)
    return names, vs


def dump(path, names, variations):
    """write a universes file ``load`` reads back to the same names and variations"""
    key_of = {f: k for k, f in KEYS.items()}
    with open(path, "w") as f:
        json.dump([dict(name=n, **{key_of[k]: v[k] for k in FIELDS}) for n, v in zip(names, variations)], f, indent=1)


def pack(variations):
    """the ctypes array of LdsimLightVariation for validated ``variations`` (the seven device-side fields)"""
    from .abi import LdsimLightVariation
    arr = (LdsimLightVariation * len(variations))()
    for a, v in zip(arr, variations):
        for f in C_FIELDS:
            setattr(a, f, float(v[f]))
    return arr


def unpack(a, base=None):
    """the variation dict of one LdsimLightVariation; the two host-side fields from ``base`` (default 1.0)"""
    v = {f: float(getattr(a, f)) for f in C_FIELDS}
    v.update({f: float(base[f]) if base is not None else 1.0 for f in HOST_FIELDS})
    return v


# ---- the definition in numpy (tests, documentation): what universe k's arrays are, stage by stage ---------------------------------
def conv_ticks():
    """``ceil((LIGHT_WINDOW[1] - LIGHT_WINDOW[0]) / LIGHT_TICK_SIZE)``: the reach of both convolutions in ticks"""
    from . import consts
    light = consts.light
    return int(math.ceil((light.LIGHT_WINDOW[1] - light.LIGHT_WINDOW[0]) / light.LIGHT_TICK_SIZE))


def scaled_input(inc, photon_scale):
    """step 1: ``x_k = (float)((double)inc * photon_scale)``, one rounding"""
    import numpy as np
    return (np.asarray(inc, dtype=np.float32).astype(np.float64) * float(photon_scale)).astype(np.float32)


def scintillation_table(v):
    """``light_sim.scintillation_model(n)`` for n = 0 .. conv_ticks() under the variation's singlet fraction and time constants"""
    from . import consts
    tick, sf, ts, tt = consts.light.LIGHT_TICK_SIZE, float(v["singlet_fraction"]), float(v["tau_s"]), float(v["tau_t"])
    out = []
    for n in range(conv_ticks() + 1):
        p1 = sf * math.exp(-float(n) * tick / ts) * (1 - math.exp(-tick / ts))
        p3 = (1 - sf) * math.exp(-float(n) * tick / tt) * (1 - math.exp(-tick / tt))
        out.append(p1 + p3)
    return out


def response_table(v):
    """``light_sim.sipm_response_model(n)`` for n = 0 .. conv_ticks(): the RLC response under the variation's response time and
    oscillation period (``SIPM_RESPONSE_MODEL 0``), or the interpolated ``IMPULSE_MODEL`` (1)"""
    from . import consts
    light = consts.light
    tick = light.LIGHT_TICK_SIZE
    out = []
    if int(light.SIPM_RESPONSE_MODEL) == 0:
        rt, op = float(v["response_time"]), float(v["oscillation_period"])
        for n in range(conv_ticks() + 1):
            t = float(n) * tick
            x = 1.0 * math.exp(-t / rt) * math.sin(t / op)
            x /= op * (rt * rt)
            x *= op * op + rt * rt
            out.append(x * tick)
        return out
    imp, itick = [float(a) for a in light.IMPULSE_MODEL], light.IMPULSE_TICK_SIZE
    for n in range(conv_ticks() + 1):
        idx = float(n) * tick / itick
        i0 = int(math.floor(idx))
        if i0 < 0 or i0 > len(imp) - 1:
            x = 0.0
        elif float(i0) == idx:
            x = imp[i0]
        elif i0 > len(imp) - 2:
            x = 0.0
        else:
            x = imp[i0] + (imp[i0 + 1] - imp[i0]) * (idx - float(i0))
        out.append(x / (itick / tick))
    return out


def convolve(x, table, gain=None, skip_zero=False):
    """steps 2 and 4 term by term: ``out[d][i]`` takes ``j = max(i - C, 0) .. i`` in ascending order, an f4 store after every
    term; ``skip_zero``: zero samples are skipped (the scintillation stage); ``gain``: the row's f64 gain, multiplied into the
    table entry before the sample (the SiPM stage).  Python loops: for small arrays."""
    import numpy as np
    x = np.asarray(x, dtype=np.float32)
    C = len(table) - 1
    out = np.zeros(x.shape, dtype=np.float32)
    for d in range(x.shape[0]):
        w = [float(t) if gain is None else float(gain[d]) * float(t) for t in table]
        row = [float(a) for a in x[d]]
        for i in range(x.shape[1]):
            acc = np.float32(0.0)
            for j in range(max(i - C, 0), i + 1):
                if skip_zero and row[j] == 0.0:
                    continue
                acc = np.float32(float(acc) + w[i - j] * row[j])
            out[d, i] = acc
    return out


def poisson_counts(scint, uniforms, normals):
    """step 3 on the host: ``calc_stat_fluctuations``' rule (inversion with one f4 uniform below a mean of 30, else a normal
    truncated at zero) for given draws, element by element: ``disc = (float)(1 / tick * count)``; elements <= 0 give 0"""
    import numpy as np
    from . import consts
    tick = consts.light.LIGHT_TICK_SIZE
    x = np.asarray(scint, dtype=np.float32)
    mean = x.astype(np.float64) * tick
    u = np.asarray(uniforms, dtype=np.float32).astype(np.float64)
    z = np.asarray(normals, dtype=np.float32).astype(np.float64)
    count = np.zeros(x.shape, dtype=np.int64)
    low = (x > 0) & (mean < 30)
    p = np.where(low, np.exp(-mean), 0.0)
    s = p.copy()
    todo = low & (u > s)
    k = 0
    while todo.any():
        k += 1
        count[todo] += 1
        p = np.where(todo, p * mean / k, p)
        prev = s
        s = np.where(todo, s + p, s)
        todo = todo & (s != prev) & (u > s)
    high = (x > 0) & ~low
    with np.errstate(invalid="ignore"):
        v = z * np.sqrt(np.where(high, mean, 0.0)) + mean
    count[high] = np.maximum(np.trunc(v[high]).astype(np.int64), 0)
    return (1.0 / tick * count.astype(np.float64)).astype(np.float32)


def universe_rows(names, variations):
    """dataset ``light_universes`` of the driver's file: the name and the nine values of every universe"""
    import numpy as np
    rows = np.zeros(len(variations), dtype=__getattr__("FILE_UNIVERSE"))
    for k, (n, v) in enumerate(zip(names, variations)):
        rows[k]["name"] = str(n).encode()
        for f in FIELDS:
            rows[k][f] = v[f]
    return rows


def file_rows(universe, event_id, start_time, trigger_idx, trigger_type, op_channel):
    """dataset ``light_universe_trig`` rows of one universe's triggers of one (event, TPC group): universe index, event id,
    trigger tick, start time of the tick axis, trigger type and the optical channels of every trigger ([n_trig][channels]);
    row i of the dataset belongs to waveform i of ``light_universe_wvfm``"""
    import numpy as np
    opc = np.asarray(op_channel)
    idx = np.asarray(trigger_idx)
    if opc.ndim != 2 or opc.shape[0] != idx.shape[0]:
        raise ValueError(f"light universes: {idx.shape[0]} triggers, op_channel of shape {opc.shape}")
    rows = np.zeros(idx.shape[0], dtype=np.dtype(_TRIG_COLUMNS + [("op_channel", "i4", (opc.shape[1],))]))
    rows["universe"], rows["event_id"], rows["trigger_idx"] = universe, event_id, idx
    rows["start_time"], rows["trigger_type"], rows["op_channel"] = start_time, trigger_type, opc
    return rows
