"""
FEE universes: a chain launch digitised again under varied front-end constants (``ChargeChain.fee_universes``,
``ldsim_chain_fee_universes`` in include/ldsim.h).

A launch spends its time on the induced currents; the LArPix front end only reads them.  A *variation* is the set of fifteen
front-end values one universe is digitised with -- absolute values, not deltas:

``discrimination_threshold, gain, v_cm, v_ref, v_pedestal, buffer_risetime``
    the constants of the same names in ``consts.detector`` (``DISCRIMINATION_THRESHOLD`` ...)
``reset_noise_charge, uncorrelated_noise_charge, discriminator_noise``
    the three noise charges; a universe with a non-zero one draws from the keyed streams of the launch's pixels
    (``ChargeChain.seed_keyed`` / ``set_batch_keys``; the driver's ``--rng keyed``): all universes of a pixel see the same
    normals and scale them by their own charges
``threshold_table_scale, threshold_table_offset, gain_table_scale``
    with per-pixel tables set (``set_pixel_thresholds`` / ``set_pixel_gains``) the threshold of a pixel is
    ``table[pixel] * scale + offset`` and its gain ``table[pixel] * gain_table_scale``; not read without tables
``adc_hold_delay, adc_busy_delay, reset_cycles``
    integers, in clock cycles

Not varied, because they shape the launch's record or the clock: ``TIME_SAMPLING``, the number of time ticks,
``MAX_ADC_VALUES``, ``MAX_TRACKS_PER_PIXEL``, ``CLOCK_CYCLE``, ``ADC_COUNTS``.

Universe ``k`` of the result equals, bit for bit, a fresh launch under ``consts`` patched to variation ``k``.

This module imports the standard library only (the driver's self-launching parent reads a universes file before numpy is
loaded); the dtypes are made on first use.
"""
import json
import math

MAX_UNIVERSES = 64                   # LDSIM_FEE_UNIVERSES_MAX

FLOAT_FIELDS = ("discrimination_threshold", "gain", "v_cm", "v_ref", "v_pedestal", "buffer_risetime",
                "reset_noise_charge", "uncorrelated_noise_charge", "discriminator_noise",
                "threshold_table_scale", "threshold_table_offset", "gain_table_scale")
INT_FIELDS = ("adc_hold_delay", "adc_busy_delay", "reset_cycles")
FIELDS = FLOAT_FIELDS + INT_FIELDS   # the fifteen values, in the order of LdsimFeeVariation
NOISE_FIELDS = FLOAT_FIELDS[6:9]
TABLE_DEFAULTS = {"threshold_table_scale": 1.0, "threshold_table_offset": 0.0, "gain_table_scale": 1.0}
MAX_TAPS = 62                        # 10 * buffer_risetime / TIME_SAMPLING the kernels hold taps for


def __getattr__(name):
    # FILE_UNIVERSE: dataset fee_universes of the driver's file (one row per universe); FILE_HIT: dataset fee_universe_hits
    if name in ("FILE_UNIVERSE", "FILE_HIT"):
        import numpy as np
        d = {"FILE_UNIVERSE": np.dtype([("index", "u2"), ("name", "S64")] + [(f, "f8") for f in FLOAT_FIELDS]
                                       + [(f, "i4") for f in INT_FIELDS]),
             "FILE_HIT": np.dtype([("universe", "u2"), ("event_id", "u4"), ("pixel_id", "i4"), ("slot", "i4"), ("adc", "i4"),
                                   ("tick", "f8"), ("charge", "f8")])}
        globals().update(d)
        return d[name]
    raise AttributeError(name)


def nominal():
    """the variation that changes nothing: the values of ``consts.detector``, table scales 1, offset 0"""
    from . import consts
    d = consts.detector
    v = {f: float(getattr(d, f.upper())) for f in FLOAT_FIELDS if f not in TABLE_DEFAULTS}
    v.update(TABLE_DEFAULTS)
    v.update({f: int(getattr(d, f.upper())) for f in INT_FIELDS})
    return v


def variation(base=None, **changes):
    """``nominal()`` (or ``base``) with ``changes`` applied; keys are the field names above in either letter case.  An unknown
    key is an error."""
    v = dict(nominal() if base is None else base)
    for k, x in changes.items():
        f = k.lower()
        if f not in FIELDS:
            raise ValueError(f"FEE universes: unknown key {k!r} (known: {', '.join(s.upper() for s in FIELDS)})")
        v[f] = x
    return v


def is_noisy(v):
    return any(float(v[f]) != 0 for f in NOISE_FIELDS)


def validate(variations, time_sampling=None):
    """The argument rules of ``ldsim_chain_fee_universes``, with the same key words: ValueError for a list that is not 1 to 64
    long, a missing or non-finite field, ``v_ref == v_cm``, a negative delay, cycle count or noise charge, a rise time beyond
    the kernel's 62 taps (checked when ``time_sampling`` is given, else against ``consts.detector.TIME_SAMPLING``)."""
    n = len(variations)
    if not (1 <= n <= MAX_UNIVERSES):
        raise ValueError(f"FEE universes: n = {n} universes, must lie in [1, {MAX_UNIVERSES}]")
    if time_sampling is None:
        from . import consts
        time_sampling = consts.detector.TIME_SAMPLING
    for k, v in enumerate(variations):
        missing = [f for f in FIELDS if f not in v]
        extra = [f for f in v if f not in FIELDS]
        if missing or extra:
            raise ValueError(f"FEE universes: universe {k}: missing fields {missing}, unknown key {extra}")
        for f in FLOAT_FIELDS:
            if isinstance(v[f], bool) or not isinstance(v[f], (int, float)) or not math.isfinite(v[f]):
                raise ValueError(f"FEE universes: universe {k}: {f} = {v[f]!r} is not finite")
        for f in INT_FIELDS:
            if isinstance(v[f], bool) or int(v[f]) != v[f] or not (-2 ** 31 <= int(v[f]) < 2 ** 31):
                raise ValueError(f"FEE universes: universe {k}: {f} = {v[f]!r} is not an integer")
        if v["v_ref"] == v["v_cm"]:
            raise ValueError(f"FEE universes: universe {k}: v_ref == v_cm ({v['v_ref']}): the ADC has no range")
        for f in INT_FIELDS:
            if v[f] < 0:
                raise ValueError(f"FEE universes: universe {k}: negative {f} ({v[f]})")
        for f in NOISE_FIELDS:
            if v[f] < 0:
                raise ValueError(f"FEE universes: universe {k}: negative noise charge {f} ({v[f]})")
        if v["buffer_risetime"] > 0 and 10 * v["buffer_risetime"] / time_sampling > MAX_TAPS:
            raise ValueError(f"FEE universes: universe {k}: buffer_risetime {v['buffer_risetime']} exceeds the kernel's "
                             f"{MAX_TAPS} taps at time_sampling {time_sampling}")
    return variations


def parse(entries):
    """[(name, changes)] of a decoded universes file: a list of ``{"name": ..., "DISCRIMINATION_THRESHOLD": ..., ...}``; the
    keys other than ``name`` are checked here (unknown keys are an error), the values by ``validate`` once they are applied"""
    if not isinstance(entries, list) or not all(isinstance(e, dict) for e in entries):
        raise ValueError("FEE universes: the file must hold a JSON list of objects")
    if not (1 <= len(entries) <= MAX_UNIVERSES):
        raise ValueError(f"FEE universes: n = {len(entries)} universes, must lie in [1, {MAX_UNIVERSES}]")
    out = []
    for k, e in enumerate(entries):
        changes = {key: x for key, x in e.items() if key != "name"}
        for key in changes:
            if key.lower() not in FIELDS:
                raise ValueError(f"FEE universes: universe {k}: unknown key {key!r} (known: name, "
                                 f"{', '.join(s.upper() for s in FIELDS)})")
        name = str(e.get("name", f"universe{k}"))
        if len(name.encode()) > 64:
            raise ValueError(f"FEE universes: universe {k}: name longer than 64 bytes")
        out.append((name, changes))
    return out


def read(path):
    """``parse`` of the JSON file ``path`` (standard library only: no constants needed)"""
    with open(path) as f:
        return parse(json.load(f))


def changes_noisy(changes):
    """True / False when the changes alone decide whether the universe has noise (a noise charge set non-zero / all three set
    to zero); None when it depends on the constants' own charges"""
    low = {k.lower(): x for k, x in changes.items()}
    given = [low[f] for f in NOISE_FIELDS if f in low]
    if any(isinstance(x, (int, float)) and x != 0 for x in given):
        return True
    return False if len(given) == len(NOISE_FIELDS) else None


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
    with open(path, "w") as f:
        json.dump([dict(name=n, **{k.upper(): v[k] for k in FIELDS}) for n, v in zip(names, variations)], f, indent=1)


def pack(variations):
    """the ctypes array of LdsimFeeVariation for validated ``variations``"""
    from .abi import LdsimFeeVariation
    arr = (LdsimFeeVariation * len(variations))()
    for a, v in zip(arr, variations):
        for f in FLOAT_FIELDS:
            setattr(a, f, float(v[f]))
        for f in INT_FIELDS:
            setattr(a, f, int(v[f]))
        a.pad = 0
    return arr


def unpack(a):
    """the variation dict of one LdsimFeeVariation"""
    v = {f: float(getattr(a, f)) for f in FLOAT_FIELDS}
    v.update({f: int(getattr(a, f)) for f in INT_FIELDS})
    return v


def universe_rows(names, variations):
    """dataset ``fee_universes`` of the driver's file: index, name and the fifteen values of every universe"""
    import numpy as np
    rows = np.zeros(len(variations), dtype=__getattr__("FILE_UNIVERSE"))
    for k, (n, v) in enumerate(zip(names, variations)):
        rows[k]["index"] = k
        rows[k]["name"] = str(n).encode()
        for f in FIELDS:
            rows[k][f] = v[f]
    return rows


def file_rows(universes, event_of_batch):
    """dataset ``fee_universe_hits`` rows of one launch from ``ChargeChain.fee_universes()``'s list: per universe its compact
    hit rows (``hit_rows``: batch, pixel, adc, slot, tick; ``hit_charge``), universe after universe; events from the rows' batch
    ids, like ``pixel_truth.file_rows``"""
    import numpy as np
    ev = np.asarray(event_of_batch, dtype=np.int64)
    parts = []
    for k, u in enumerate(universes):
        hr, q = u["hit_rows"], np.asarray(u["hit_charge"], dtype=np.float64)
        if len(hr) != len(q):
            raise ValueError(f"universe {k}: {len(hr)} hit rows, {len(q)} charges")
        rows = np.zeros(len(hr), dtype=__getattr__("FILE_HIT"))
        rows["universe"] = k
        rows["event_id"] = ev[hr["batch"].astype(np.int64)]
        rows["pixel_id"], rows["slot"], rows["adc"], rows["tick"] = hr["pixel"], hr["slot"], hr["adc"], hr["tick"]
        rows["charge"] = q
        parts.append(rows)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=__getattr__("FILE_HIT"))
