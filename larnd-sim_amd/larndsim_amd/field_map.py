"""
Drift-field maps: per TPC, a regular 3D grid in the simulation frame (TPC_BORDERS after
``swap_coordinates``, cm, z = drift coordinate) with up to four channels -- ``E`` (kV/cm, replaces the module's e_field in
the recombination), ``dx`` / ``dy`` (where the charge starting at a node reaches the anode, cm) and ``dz`` (shift of the
equivalent drift coordinate, cm).  A channel left out is uniform (E = e_field, offsets 0); a TPC without a map drifts as
before.

File format (``.npz``): for every TPC id i that has a map, ``tpc{i}_origin`` and ``tpc{i}_spacing`` (3 floats each: the
position of node (0, 0, 0) and the node pitch along x, y, z) and any of ``tpc{i}_E``, ``tpc{i}_dx``, ``tpc{i}_dy``,
``tpc{i}_dz`` (C-order [nx][ny][nz], every dimension >= 2, one shape for all channels of a TPC).
"""
import re

import numpy as np

CHANNELS = ("E", "dx", "dy", "dz")
_KEY = re.compile(r"^tpc(\d+)_(origin|spacing|E|dx|dy|dz)$")


def validate(maps, n_tpc):
    """{tpc: {"origin", "spacing", channel: array}} -> the same with float64 C-contiguous arrays; ValueError on anything
    the library would refuse (and on a map without a channel)."""
    out = {}
    for tpc, m in maps.items():
        tpc = int(tpc)
        if not 0 <= tpc < n_tpc:
            raise ValueError(f"field map: TPC {tpc} outside [0, {n_tpc})")
        unknown = set(m) - {"origin", "spacing", *CHANNELS}
        if unknown:
            raise ValueError(f"field map of TPC {tpc}: unknown entries {sorted(unknown)}")
        v = {}
        for k in ("origin", "spacing"):
            if k not in m:
                raise ValueError(f"field map of TPC {tpc}: no {k}")
            a = np.asarray(m[k], dtype=np.float64)
            if a.shape != (3,) or not np.all(np.isfinite(a)):
                raise ValueError(f"field map of TPC {tpc}: {k} must be 3 finite numbers, got {m[k]!r}")
            v[k] = np.ascontiguousarray(a)
        if not np.all(v["spacing"] > 0):
            raise ValueError(f"field map of TPC {tpc}: spacing must be > 0, got {v['spacing'].tolist()}")
        shape = None
        for ch in CHANNELS:
            if ch not in m or m[ch] is None:
                continue
            a = np.ascontiguousarray(m[ch], dtype=np.float64)
            if a.ndim != 3 or min(a.shape) < 2:
                raise ValueError(f"field map of TPC {tpc}: {ch} must be [nx][ny][nz] with every dimension >= 2, got shape "
                                 f"{a.shape}")
            if shape is not None and a.shape != shape:
                raise ValueError(f"field map of TPC {tpc}: {ch} has shape {a.shape}, another channel {shape}")
            shape = a.shape
            if not np.all(np.isfinite(a)):
                raise ValueError(f"field map of TPC {tpc}: {ch} holds a non-finite value")
            if ch == "E" and not np.all(a > 0):
                raise ValueError(f"field map of TPC {tpc}: E must be > 0 everywhere (min {a.min()})")
            v[ch] = a
        if shape is None:
            raise ValueError(f"field map of TPC {tpc}: none of the channels {CHANNELS}")
        out[tpc] = v
    return out


def load(path, n_tpc):
    """the validated maps of an ``.npz`` file (format above); ``n_tpc`` = len(TPC_BORDERS) of the configuration"""
    maps = {}
    with np.load(path, allow_pickle=False) as f:
        for key in f.files:
            mt = _KEY.match(key)
            if not mt:
                raise ValueError(f"field map {path}: unexpected key {key!r} (tpc<i>_origin / _spacing / _E / _dx / _dy / _dz)")
            maps.setdefault(int(mt.group(1)), {})[mt.group(2)] = f[key]
    return validate(maps, n_tpc)


def save(path, maps):
    """write ``maps`` ({tpc: {"origin", "spacing", channel: array}}) in the format ``load`` reads"""
    np.savez(path, **{f"tpc{int(t)}_{k}": np.asarray(a) for t, m in maps.items() for k, a in m.items() if a is not None})
