"""
Pixel charge truth: the induced charge per unique pixel and per (pixel, track) of a chain launch
(``ChargeChain.pixel_truth``, ``ldsim_chain_pixel_truth`` in include/ldsim.h).

The reference has no such output: its results end in hits, and its backtracking fractions are normalised per hit.
Per unique-pixel row ``u`` of ``ChargeChain.download()``, in the unit of ``adc_list`` (electrons), ``dt = TIME_SAMPLING``:

``q_track[u][k]``
    ``dt * sum_t wf_k[t]`` over the ticks the pixel sum takes from slot ``k``'s f32 current row: the row's written window
    ``[w0, w1)`` placed at the slot's start tick on the pixel's time axis and clipped to ``[0, N_t)``, accumulated in f64.
    Slots are the filled entries of ``track_pixel_map[u]``, in that order; the others hold 0.
``q_induced[u]``
    ``dt * sum_t S[t]``, ``S`` the pixel's summed waveform: f64, the slots' rows added in slot order.
``q_abs[u]``
    ``dt * sum_t |S[t]|``.  A pixel that only saw induction has ``q_induced ~ 0`` and ``q_abs > 0``.
``n_hits[u]``, ``q_hits[u]``
    the pixel's hits and ``sum_{h < n_hits} adc_list[u][h]`` (slot 0 up), read from the launch's own results.  With FEE
    noise on, ``q_hits`` includes the noise charges the hits were read out with; the three values above never do.

``restate`` below is that definition in numpy for one pixel: the CPU tests run it on hand-made rows, the GPU tests feed it
the oracle's currents.
"""
import numpy as np

# rows of the compact form (LdsimPixelTruthRow / LdsimPixelTruthTrack of include/ldsim.h)
PIXEL_ROW = np.dtype([("row", "i4"), ("pixel_id", "i4"), ("batch", "i4"), ("n_hits", "i4"), ("n_tracks", "i4"), ("pad", "i4"),
                      ("q_hits", "f8"), ("q_induced", "f8"), ("q_abs", "f8")])
TRACK_ENTRY = np.dtype([("segment", "i8"), ("q", "f8")])
assert PIXEL_ROW.itemsize == 48 and TRACK_ENTRY.itemsize == 16

# datasets of the driver's output file (cli/simulate_pixels.py --pixel_truth)
FILE_PIXEL = np.dtype([("event_id", "u4"), ("pixel_id", "i4"), ("n_hits", "i4"), ("q_hits", "f8"), ("q_induced", "f8"),
                       ("q_abs", "f8"), ("track_begin", "i8"), ("track_count", "i4")])
FILE_TRACK = np.dtype([("segment_id", "i8"), ("q", "f8")])


def hits_of(adc_list):
    """(n_hits [U], q_hits [U]) of ``adc_list`` [U][A]: the filled slots come first; summed slot 0 up, like the device"""
    adc = np.asarray(adc_list, dtype=np.float64).reshape(len(adc_list), -1)
    n_hits = (adc != 0).sum(axis=1).astype(np.int32)
    run = np.concatenate([np.zeros((adc.shape[0], 1)), np.cumsum(adc, axis=1)], axis=1)      # (sequential per row)
    return n_hits, run[np.arange(adc.shape[0]), n_hits]


def restate(rows, starts, windows, dt, n_ticks, adc=None):
    """The five per-pixel values of one pixel.

    rows     [n_slots][T] current rows of the pixel's slots, slot order (any float dtype; read as f32 like the device's)
    starts   [n_slots]    tick of each row's element 0 on the pixel's time axis
    windows  [n_slots][2] the elements [w0, w1) of each row that count (a row written in full: (0, T))
    dt                    TIME_SAMPLING
    n_ticks               N_t, the length of the pixel's time axis
    adc      [A] or None  the pixel's ``adc_list`` row (None: no hits)

    Returns dict(q_track [n_slots], q_induced, q_abs, n_hits, q_hits)."""
    rows = np.asarray(rows, dtype=np.float32).astype(np.float64)
    rows = rows.reshape(len(starts), -1) if len(starts) else np.zeros((0, 0))
    S = np.zeros(int(n_ticks))
    q_track = np.zeros(len(starts))
    for k, (st, (w0, w1)) in enumerate(zip(starts, windows)):
        st, w0, w1 = int(st), max(int(w0), 0), min(int(w1), rows.shape[1])
        lo, hi = max(st + w0, 0), min(st + w1, int(n_ticks))
        if hi <= lo:
            continue
        part = rows[k, lo - st:hi - st]
        q_track[k] = dt * part.sum()
        S[lo:hi] += part                                    # (slots in slot order)
    n_hits, q_hits = (np.zeros(1, np.int32), np.zeros(1)) if adc is None else hits_of(np.asarray(adc)[None, :])
    return dict(q_track=q_track, q_induced=dt * S.sum(), q_abs=dt * np.abs(S).sum(), n_hits=int(n_hits[0]),
                q_hits=float(q_hits[0]))


def tracks_of(rows, entries):
    """(begin, count) of every pixel row's entries in ``entries``: they lie pixel after pixel"""
    count = rows["n_tracks"].astype(np.int64)
    begin = np.cumsum(count) - count
    if len(entries) != int(count.sum()):
        raise ValueError(f"{len(entries)} track entries, the pixel rows count {int(count.sum())}")
    return begin, count


def file_rows(pt, event_of_batch, first_segment_of_batch, segment_ids, track_base=0):
    """(pixel_truth rows, pixel_truth_tracks rows) of the driver's file from ``ChargeChain.pixel_truth()``'s compact form:
    events from the rows' batch ids, track slots mapped to the file's segment ids (a batch's slots count its segments from its
    first one, like ``packets.compact_to_rows``), ``track_begin`` = ``track_base`` + the row's first entry."""
    px, tr = pt["pixels"], pt["tracks"]
    begin, count = tracks_of(px, tr)
    batch = px["batch"].astype(np.int64)
    rows = np.zeros(len(px), dtype=FILE_PIXEL)
    rows["event_id"] = np.asarray(event_of_batch, dtype=np.int64)[batch]
    for k in ("pixel_id", "n_hits", "q_hits", "q_induced", "q_abs"):
        rows[k] = px[k]
    rows["track_begin"] = int(track_base) + begin
    rows["track_count"] = count
    entries = np.zeros(len(tr), dtype=FILE_TRACK)
    seg_idx = np.repeat(np.asarray(first_segment_of_batch, dtype=np.int64)[batch], count) + tr["segment"]
    entries["segment_id"] = np.asarray(segment_ids, dtype=np.int64)[seg_idx]
    entries["q"] = tr["q"]
    return rows, entries
