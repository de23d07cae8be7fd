"""
Charge universes: a chain launch re-weighted for recombination and electron lifetime (``ChargeChain.universes``,
``ldsim_chain_universes`` in include/ldsim.h).

Charge enters the induced current as one linear factor per segment, and neither the pair list nor the time windows read it.  A
universe that only changes how many electrons a segment delivers is therefore the launch's current rows, each multiplied by one
number per segment, summed and scanned again.  A *variation* holds the seven values one universe is re-weighted with --
absolute values, not deltas:

``electron_lifetime, w_ion``
    ``consts.detector.ELECTRON_LIFETIME`` and ``consts.physics.W_ION``
``box_alpha, box_beta, birks_ab, birks_kb``
    the parameters of the two recombination models (``consts.physics.BOX_ALPHA`` ... ``BIRKS_kb``)
``recomb_mode``
    1 = box, 2 = Birks (``consts.physics.BOX`` / ``BIRKS``, the mode of ``quench_drift``); a universe may switch the model

The weight of a segment is not "nominal times a smooth factor": ``n_electrons`` is stored twice by the quench/drift, after the
recombination and after the lifetime factor, each time rounded to the column's type (a ``uint32`` in the reference's dtype).
The weights are formed from replayed, stored values: ``w = n_k / n_res`` (``segment_weights``), which is what a fresh launch
under the universe's constants reads.

Not varied: ``E_FIELD`` and ``V_DRIFT`` (they set the drift times, where the rows sit on the time axis), the diffusion constants
(the rows' shapes), ``LAR_DENSITY`` (redundant with ``BIRKS_kb`` and ``BOX_BETA``), ``W_PH`` and the light leg (``n_photons`` is
not re-weighted).

This module imports the standard library only, like ``fee_universes``; numpy is loaded by the functions that need it.
"""
import json
import math

from . import fee_universes as _fu
from .fee_universes import MAX_UNIVERSES, file_rows  # noqa: F401  (file_rows: the rows of dataset charge_universe_hits)

FLOAT_FIELDS = ("electron_lifetime", "w_ion", "box_alpha", "box_beta", "birks_ab", "birks_kb")
INT_FIELDS = ("recomb_mode",)
FIELDS = FLOAT_FIELDS + INT_FIELDS   # the seven values, in the order of LdsimChargeVariation
BOX, BIRKS = 1, 2
MODELS = {"box": BOX, "birks": BIRKS}
# the keys of a universes file, and where the constants hold their nominal values
FILE_KEYS = {"ELECTRON_LIFETIME": "electron_lifetime", "W_ION": "w_ion", "BOX_ALPHA": "box_alpha", "BOX_BETA": "box_beta",
             "BIRKS_AB": "birks_ab", "BIRKS_KB": "birks_kb", "RECOMB_MODEL": "recomb_mode"}
_CONSTS = {"electron_lifetime": ("detector", "ELECTRON_LIFETIME"), "w_ion": ("physics", "W_ION"),
           "box_alpha": ("physics", "BOX_ALPHA"), "box_beta": ("physics", "BOX_BETA"), "birks_ab": ("physics", "BIRKS_Ab"),
           "birks_kb": ("physics", "BIRKS_kb")}


def __getattr__(name):
    # FILE_UNIVERSE: dataset charge_universes of the driver's file (one row per universe: the seven charge values, then the
    # fifteen front-end values); FILE_HIT: dataset charge_universe_hits (fee_universes.FILE_HIT)
    if name == "FILE_HIT":
        return _fu.__getattr__("FILE_HIT")
    if name == "FILE_UNIVERSE":
        import numpy as np
        d = np.dtype([("index", "u2"), ("name", "S64")] + [(f, "f8") for f in FLOAT_FIELDS] + [(f, "i4") for f in INT_FIELDS]
                     + [(f, "f8") for f in _fu.FLOAT_FIELDS] + [(f, "i4") for f in _fu.INT_FIELDS])
        globals()["FILE_UNIVERSE"] = d
        return d
    raise AttributeError(name)


def nominal(mode=BIRKS):
    """the variation that changes nothing of a ``quench_drift(mode)``: the values of ``consts`` and the mode"""
    from . import consts
    v = {f: float(getattr(getattr(consts, ns), n)) for f, (ns, n) in _CONSTS.items()}
    v["recomb_mode"] = int(mode)
    return v


def variation(base=None, **changes):
    """``nominal()`` (or ``base``) with ``changes`` applied; keys are the field names above or a file's keys, in either letter
    case; ``recomb_model="box"`` / ``"birks"`` sets ``recomb_mode``.  An unknown key is an error."""
    v = dict(nominal() if base is None else base)
    for k, x in changes.items():
        f = FILE_KEYS.get(k.upper(), k.lower())
        if f not in FIELDS:
            raise ValueError(f"charge universes: unknown key {k!r} (known: {', '.join(FILE_KEYS)})")
        if f == "recomb_mode" and isinstance(x, str):
            if x.lower() not in MODELS:
                raise ValueError(f"charge universes: RECOMB_MODEL {x!r} must be \"box\" or \"birks\"")
            x = MODELS[x.lower()]
        v[f] = x
    return v


def validate(variations):
    """The argument rules of ``ldsim_chain_universes``, with the same key words: ValueError for a list that is not 1 to 64 long,
    a missing or non-finite field, ``electron_lifetime`` or ``w_ion`` not above 0, a ``recomb_mode`` other than 1 or 2."""
    n = len(variations)
    if not (1 <= n <= MAX_UNIVERSES):
        raise ValueError(f"charge universes: n = {n} universes, must lie in [1, {MAX_UNIVERSES}]")
    for k, v in enumerate(variations):
        missing = [f for f in FIELDS if f not in v]
        extra = [f for f in v if f not in FIELDS]
        if missing or extra:
            raise ValueError(f"charge universes: universe {k}: missing fields {missing}, unknown key {extra}")
        for f in FLOAT_FIELDS:
            if isinstance(v[f], bool) or not isinstance(v[f], (int, float)) or not math.isfinite(v[f]):
                raise ValueError(f"charge universes: universe {k}: {f} = {v[f]!r} is not finite")
        for f in ("electron_lifetime", "w_ion"):
            if not v[f] > 0:
                raise ValueError(f"charge universes: universe {k}: {f} {v[f]} must be > 0")
        m = v["recomb_mode"]
        if isinstance(m, bool) or not isinstance(m, int) or m not in (BOX, BIRKS):
            raise ValueError(f"charge universes: universe {k}: recomb_mode {m!r} must be 1 (box) or 2 (Birks)")
    return variations


def parse(entries):
    """[(name, charge changes, FEE changes)] of a decoded universes file: a list of ``{"name": ..., "ELECTRON_LIFETIME": ...,
    "RECOMB_MODEL": "box", "GAIN": ..., ...}``.  The keys other than ``name`` are a charge key (``FILE_KEYS``) or a key of
    ``fee_universes.FIELDS``, so one file holds combined universes; unknown keys are an error, the values are checked by
    ``validate`` once they are applied."""
    if not isinstance(entries, list) or not all(isinstance(e, dict) for e in entries):
        raise ValueError("charge universes: the file must hold a JSON list of objects")
    if not (1 <= len(entries) <= MAX_UNIVERSES):
        raise ValueError(f"charge universes: n = {len(entries)} universes, must lie in [1, {MAX_UNIVERSES}]")
    out = []
    for k, e in enumerate(entries):
        charge, fee = {}, {}
        for key, x in e.items():
            if key == "name":
                continue
            if key.upper() in FILE_KEYS:
                if key.upper() == "RECOMB_MODEL" and not (isinstance(x, str) and x.lower() in MODELS):
                    raise ValueError(f"charge universes: universe {k}: RECOMB_MODEL {x!r} must be \"box\" or \"birks\"")
                charge[key] = x
            elif key.lower() in _fu.FIELDS:
                fee[key] = x
            else:
                raise ValueError(f"charge universes: universe {k}: unknown key {key!r} (known: name, {', '.join(FILE_KEYS)}, "
                                 f"{', '.join(s.upper() for s in _fu.FIELDS)})")
        name = str(e.get("name", f"universe{k}"))
        if len(name.encode()) > 64:
            raise ValueError(f"charge universes: universe {k}: name longer than 64 bytes")
        out.append((name, charge, fee))
    return out


def read(path):
    """``parse`` of the JSON file ``path`` (standard library only: no constants needed)"""
    with open(path) as f:
        return parse(json.load(f))


def load(path, mode=BIRKS):
    """(names, charge variations, FEE variations) of the universes file ``path``: every entry is ``nominal(mode)`` and
    ``fee_universes.nominal()`` (the constants loaded now) with the entry's keys applied, validated"""
    entries = read(path)
    names = [n for n, _, _ in entries]
    cs = [variation(nominal(mode), **c) for _, c, _ in entries]
    fs = [_fu.variation(**f) for _, _, f in entries]
    validate(cs)
    _fu.validate(fs)
    return names, cs, fs


def pack(variations):
    """the ctypes array of LdsimChargeVariation for validated ``variations``"""
    from .abi import LdsimChargeVariation
    arr = (LdsimChargeVariation * len(variations))()
    for a, v in zip(arr, variations):
        for f in FLOAT_FIELDS:
            setattr(a, f, float(v[f]))
        a.recomb_mode = int(v["recomb_mode"])
        a.pad = 0
    return arr


def unpack(a):
    """the variation dict of one LdsimChargeVariation"""
    v = {f: float(getattr(a, f)) for f in FLOAT_FIELDS}
    v["recomb_mode"] = int(a.recomb_mode)
    return v


def universe_rows(names, charge, fee):
    """dataset ``charge_universes`` of the driver's file: index, name, the seven charge values and the fifteen front-end values
    of every universe"""
    import numpy as np
    rows = np.zeros(len(charge), dtype=__getattr__("FILE_UNIVERSE"))
    for k, (n, c, f) in enumerate(zip(names, charge, fee)):
        rows[k]["index"] = k
        rows[k]["name"] = str(n).encode()
        for x in FIELDS:
            rows[k][x] = c[x]
        for x in _fu.FIELDS:
            rows[k][x] = f[x]
    return rows


# ---- the numpy twins of the two definitions ---------------------------------------------------------------------------------
def narrow_store(x, dtype):
    """a f64 array as the segment store holds it after a store into a column of ``dtype``: rounded to f4, truncated towards zero
    for the integer types, unchanged for f8"""
    import numpy as np
    dtype = np.dtype(dtype)
    x = np.asarray(x, dtype=np.float64)
    if dtype == np.float64:
        return x.copy()
    if dtype.kind in "iu":
        return np.trunc(x).astype(dtype).astype(np.float64)
    return x.astype(dtype).astype(np.float64)


def replay(v, dE, dEdx, e_field, drift_distance, in_tpc, dtype, lar_density, v_drift):
    """``n_electrons`` as ``quench_drift`` stores it under variation ``v``, operation for operation: the recombination factor at
    ``e_field`` (a number, or one per segment with a field map), the store, and for the segments ``in_tpc`` the lifetime factor
    over ``drift_distance`` (|z - z_anode| of the drift coordinate the drift used) and the store again.  ``dtype``: the dtype of
    the ``n_electrons`` column."""
    import numpy as np
    dE, dEdx = np.asarray(dE, dtype=np.float64), np.asarray(dEdx, dtype=np.float64)
    e = np.broadcast_to(np.asarray(e_field, dtype=np.float64), dE.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        if v["recomb_mode"] == BOX:
            csi = v["box_beta"] * dEdx / (e * lar_density)
            r = np.log(v["box_alpha"] + csi) / csi
            recomb = np.where(r > 0, r, 0.0)
        elif v["recomb_mode"] == BIRKS:
            recomb = v["birks_ab"] / (1 + v["birks_kb"] * dEdx / (e * lar_density))
        else:
            raise ValueError("Invalid recombination mode: must be 'physics.BOX' or 'physics.BIRKS'")
    if np.isnan(recomb).any():
        raise RuntimeError("Invalid recombination value")
    n_q = narrow_store(recomb * dE / v["w_ion"], dtype)
    drift_time = np.asarray(drift_distance, dtype=np.float64) / v_drift
    n_d = narrow_store(n_q * np.exp(-drift_time / v["electron_lifetime"]), dtype)
    return np.where(np.asarray(in_tpc, dtype=bool), n_d, n_q)


def segment_weights(v, n_res, dE, dEdx, e_field, drift_distance, in_tpc, dtype, lar_density, v_drift, simulated=None):
    """(w f64 [n], n_k [n], n_unweightable) of variation ``v``: ``n_k = replay(...)``, ``w = n_k / n_res`` in f64; where
    ``n_res == 0`` the weight is 0, and the segment is counted when ``n_k != 0``.  Segments outside every TPC (``in_tpc`` False)
    and segments that are not ``simulated`` (``batch < 0``) have no pairs: weight 1, not counted."""
    import numpy as np
    n_res = np.asarray(n_res, dtype=np.float64)
    n_k = replay(v, dE, dEdx, e_field, drift_distance, in_tpc, dtype, lar_density, v_drift)
    live = np.asarray(in_tpc, dtype=bool)
    if simulated is not None:
        live = live & np.asarray(simulated, dtype=bool)
    w = np.ones(n_res.shape)
    zero = n_res == 0
    ok = live & ~zero
    w[ok] = n_k[ok] / n_res[ok]
    w[live & zero] = 0.0
    return w, n_k, int((live & zero & (n_k != 0)).sum())


def weighted_sums(pixels, weights, n_ticks):
    """S f64 [len(pixels)][n_ticks]: ``pixels`` holds per pixel its slots in slot order, each ``(segment, start, w0, w1, row)``
    -- the segment's index into ``weights``, the tick of the row's element 0 on the pixel's axis, the ticks [w0, w1) of the row
    that were written, the f32 row.  ``S[t] += weights[segment] * float64(row[t - start])`` over the window clipped to the row
    and to [0, n_ticks), every product rounded before it is added."""
    import numpy as np
    weights = np.asarray(weights, dtype=np.float64)
    S = np.zeros((len(pixels), n_ticks))
    for p, slots in enumerate(pixels):
        for seg, start, w0, w1, row in slots:
            row = np.asarray(row)
            lo = max(start + max(w0, 0), 0)
            hi = min(start + min(w1, len(row)), n_ticks)
            if hi > lo:
                S[p, lo:hi] += weights[seg] * row[lo - start:hi - start].astype(np.float64)
    return S
