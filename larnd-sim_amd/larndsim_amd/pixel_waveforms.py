"""
Pixel current waveforms: the summed induced current ``S[t]`` of every unique pixel of a chain launch, zero-suppressed into
spans (``ChargeChain.pixel_waveforms``, ``ldsim_chain_pixel_waveforms`` in include/ldsim.h).

The reference has no such output.  Per unique-pixel row ``u`` of ``ChargeChain.download()``, on the pixel's time axis
``[0, N_t)`` (tick ``t`` is the time ``t * TIME_SAMPLING`` on the axis ``adc_ticks_list`` uses):

``S[t]``
    f64: the f32 current rows of the pixel's slots added in slot order, each over its written window placed at the slot's
    start tick and clipped to ``[0, N_t)`` -- the sum of ``pixel_truth.restate``, so ``dt * sum(S) = q_induced``.  It holds no
    FEE noise; ticks outside every window are 0.
active ticks
    ``A = {t : |S[t]| > min_abs_current}``: strict, in f64 (0: the ticks with ``S != 0``).
    The device compares the unrounded f64 ``S``; the samples it returns are rounded to f32.  A threshold equal to a returned
    sample therefore excludes that tick only when its ``S`` is exactly an f32 (a sum of one slot); a sum of several slots that
    rounding moved down still exceeds it.
kept ticks
    ``K = {t in [0, N_t) : some a in A has |t - a| <= pad_ticks}``, ``0 <= pad_ticks <= 64``.
spans
    the maximal runs of consecutive ticks of ``K``; a span's samples are ``(float)S[t]`` of its ticks in rising ``t``.
order
    span rows by ``(u, t_begin)``, the samples of all spans concatenated in that order.

The functions below are that definition in numpy: the CPU tests run them on hand-made arrays, the GPU tests apply them to the
device's own dense ``S``.
"""
import numpy as np

MAX_PAD_TICKS = 64

# rows of the compact form (LdsimPixelWaveSpan of include/ldsim.h)
SPAN_ROW = np.dtype([("row", "i4"), ("pixel_id", "i4"), ("batch", "i4"), ("t_begin", "i4"), ("n_samples", "i4"), ("pad", "i4"),
                     ("sample_begin", "i8")])
assert SPAN_ROW.itemsize == 32

# dataset pixel_waveforms of the driver's output file (cli/simulate_pixels.py --pixel_waveforms); pixel_waveform_samples is f4
FILE_SPAN = np.dtype([("event_id", "u4"), ("pixel_id", "i4"), ("t_begin", "i4"), ("n_samples", "i4"), ("sample_begin", "i8")])


def check_args(min_abs_current, pad_ticks):
    """the argument rules of ``ldsim_chain_pixel_waveforms``"""
    if not (0 <= float(min_abs_current) < float("inf")):
        raise ValueError(f"min_abs_current {min_abs_current!r} must be finite and >= 0")
    if int(pad_ticks) != pad_ticks or not (0 <= int(pad_ticks) <= MAX_PAD_TICKS):
        raise ValueError(f"pad_ticks {pad_ticks!r} must be an integer in [0, {MAX_PAD_TICKS}]")


def kept_of(S, min_abs_current=0.0, pad_ticks=0):
    """bool, the shape of ``S`` ([N_t] or [n][N_t]): the kept ticks (along the last axis)"""
    check_args(min_abs_current, pad_ticks)
    S = np.asarray(S)
    n, pad = S.shape[-1], int(pad_ticks)
    active = np.abs(S.astype(np.float64)) > float(min_abs_current)
    before = np.concatenate([np.zeros(S.shape[:-1] + (1,), dtype=np.int64), np.cumsum(active, axis=-1)], axis=-1)
    t = np.arange(n)                                             # active ticks in [t - pad, t + pad], clipped to the axis
    return before[..., np.minimum(t + pad + 1, n)] - before[..., np.maximum(t - pad, 0)] > 0


def _runs(kept):
    """(row, t_begin, n) of the runs of True along the last axis of ``kept`` [n][N_t], ordered by (row, t_begin)"""
    k = np.zeros((kept.shape[0], kept.shape[1] + 2), dtype=np.int8)
    k[:, 1:-1] = kept
    d = np.diff(k, axis=1)
    row, begin = np.nonzero(d == 1)                              # (row-major: the i-th begin and the i-th end are one run's)
    _, end = np.nonzero(d == -1)
    return row, begin.astype(np.int64), (end - begin).astype(np.int64)


def spans_of(S, min_abs_current=0.0, pad_ticks=0):
    """(t_begin [n_spans], n_samples [n_spans]) of one pixel's ``S`` [N_t], in rising ``t_begin``"""
    _, begin, n = _runs(kept_of(np.asarray(S).ravel(), min_abs_current, pad_ticks)[None, :])
    return begin, n


def compact_of(S_dense, rows_meta, min_abs_current=0.0, pad_ticks=0, hits_only=False):
    """The compact form of dense rows ``S_dense`` [n][N_t].  ``rows_meta``: per dense row its ``row`` (u), ``pixel_id`` and
    ``batch`` (and ``n_hits`` when ``hits_only``), as a dict of arrays [n] or a structured array.  Returns
    ``dict(spans= SPAN_ROW rows, samples= f32, n_ticks=)``."""
    S_dense = np.asarray(S_dense)
    S_dense = S_dense.reshape(len(S_dense), -1)
    kept = kept_of(S_dense, min_abs_current, pad_ticks)
    if hits_only:
        kept &= (np.asarray(rows_meta["n_hits"]) > 0)[:, None]
    i, begin, n = _runs(kept)
    spans = np.zeros(len(i), dtype=SPAN_ROW)
    for k in ("row", "pixel_id", "batch"):
        spans[k] = np.asarray(rows_meta[k])[i]
    spans["t_begin"], spans["n_samples"] = begin, n
    spans["sample_begin"] = np.cumsum(n) - n
    return dict(spans=spans, samples=S_dense[kept].astype(np.float32), n_ticks=int(S_dense.shape[1]))


def expand(spans, samples, U, n_ticks):
    """dense f32 [U][n_ticks] of a compact form: the samples at their ticks, 0 elsewhere"""
    out = np.zeros((int(U), int(n_ticks)), dtype=np.float32)
    samples = np.asarray(samples, dtype=np.float32)
    for s in spans:
        b, n, t = int(s["sample_begin"]), int(s["n_samples"]), int(s["t_begin"])
        if t < 0 or n < 0 or t + n > n_ticks or b < 0 or b + n > len(samples):
            raise ValueError(f"span {s} does not fit {n_ticks} ticks and {len(samples)} samples")
        out[int(s["row"]), t:t + n] = samples[b:b + n]
    return out


def file_rows(pw, event_of_batch, sample_base=0):
    """(pixel_waveforms rows, pixel_waveform_samples) of the driver's file from ``ChargeChain.pixel_waveforms()``'s compact
    form: events from the rows' batch ids, like ``pixel_truth.file_rows``; ``sample_begin`` = ``sample_base`` + the span's
    first sample (counted over the whole file)."""
    sp, sam = pw["spans"], np.asarray(pw["samples"], dtype=np.float32)
    if len(sam) != int(sp["n_samples"].astype(np.int64).sum()):
        raise ValueError(f"{len(sam)} samples, the span rows count {int(sp['n_samples'].astype(np.int64).sum())}")
    rows = np.zeros(len(sp), dtype=FILE_SPAN)
    rows["event_id"] = np.asarray(event_of_batch, dtype=np.int64)[sp["batch"].astype(np.int64)]
    for k in ("pixel_id", "t_begin", "n_samples"):
        rows[k] = sp[k]
    rows["sample_begin"] = int(sample_base) + sp["sample_begin"]
    return rows, sam
