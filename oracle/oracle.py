"""
TEST INFRASTRUCTURE ONLY -- ctypes wrapper of oracle/libldsim_oracle.so.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module;
the product package (larndsim_amd) never does.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_HERE)
if os.path.join(_REPO, "larnd-sim_amd") not in sys.path:
    sys.path.insert(0, os.path.join(_REPO, "larnd-sim_amd"))

from larndsim_amd import consts  # noqa: E402
from larndsim_amd.abi import LdsimConsts, pack_consts  # noqa: E402
from larndsim_amd.layout import FIELDS, store_codes  # noqa: E402

_lib = None


def oracle_dtype():
    """All-f8 mirror of the hot-path fields (+ i4 pixel_plane): the flat record the C oracle works on."""
    return np.dtype([(n, 'f8') for n in FIELDS[:-1]] + [('pixel_plane', 'i4'), ('_pad', 'i4')])


def to_oracle(tracks):
    """Structured array of any layout -> flat f8 oracle records."""
    out = np.zeros(tracks.shape[0], dtype=oracle_dtype())
    for n in FIELDS:
        if n in tracks.dtype.names:
            out[n] = tracks[n]
    return out


def from_oracle(orec, tracks, fields=None):
    """Copy (already narrowed) oracle fields back into a structured array."""
    for n in (fields or FIELDS):
        if n in tracks.dtype.names:
            tracks[n] = orec[n]
    return tracks


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(_HERE, "libldsim_oracle.so")
        if not os.path.exists(path):
            build()
        _lib = C.CDLL(path)
    return _lib


def _p(a, t=None):
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)


def _consts(noise_zero=True):
    return pack_consts(noise_zero=noise_zero)


def quench(tracks, mode):
    o = to_oracle(tracks)
    codes, _ = store_codes(tracks.dtype)
    c = _consts()
    rc = lib().o_quench(_p(o), C.c_int64(len(o)), C.byref(c), C.c_int(mode), _p(codes))
    if rc == -1:
        raise ValueError("Invalid recombination mode: must be 'physics.BOX' or 'physics.BIRKS'")
    if rc == -2:
        raise RuntimeError("Invalid recombination value")
    from_oracle(o, tracks, ["n_electrons", "n_photons"])
    return tracks


def drift(tracks):
    o = to_oracle(tracks)
    codes, _ = store_codes(tracks.dtype)
    c = _consts()
    lib().o_drift(_p(o), C.c_int64(len(o)), C.byref(c), _p(codes))
    from_oracle(o, tracks, ["pixel_plane", "n_electrons", "long_diff", "tran_diff", "t", "t_start", "t_end"])
    return tracks


def max_pixels(tracks):
    o = to_oracle(tracks)
    c = _consts()
    n = C.c_int64(0)
    lib().o_max_pixels(_p(o), C.c_int64(len(o)), C.byref(c), C.byref(n))
    return n.value


def get_pixels(tracks, max_active, P, radius):
    o = to_oracle(tracks)
    c = _consts()
    n = len(o)
    active = np.full((n, max_active), -1, dtype=np.int32)
    neigh = np.full((n, P), -1, dtype=np.int32)
    nrad = np.full((n, P), -1, dtype=np.int32)
    nlist = np.zeros(n)
    lib().o_get_pixels(_p(o), C.c_int64(n), C.byref(c), C.c_int(radius), _p(active), C.c_int64(max_active),
                       _p(neigh), _p(nrad), C.c_int64(P), _p(nlist))
    return active, neigh, nrad, nlist


def time_intervals(tracks):
    o = to_oracle(tracks)
    c = _consts()
    starts = np.empty(len(o))
    tmax = C.c_int64(0)
    lib().o_time_intervals(_p(o), C.c_int64(len(o)), C.byref(c), _p(starts), C.byref(tmax))
    return starts, tmax.value


def tracks_current(tracks, pixels, T, response):
    o = to_oracle(tracks)
    c = _consts()
    S, P = pixels.shape
    pixels = np.ascontiguousarray(pixels, dtype=np.int32)
    response = np.ascontiguousarray(response, dtype=np.float64)
    signals = np.zeros((S, P, T), dtype=np.float32)
    lib().o_tracks_current(_p(signals), _p(pixels), _p(o), C.c_int64(S), C.c_int64(P), C.c_int64(T), _p(response),
                           C.c_int64(response.shape[0]), C.c_int64(response.shape[1]), C.c_int64(response.shape[2]),
                           C.byref(c))
    return signals


def rho(point, q, start, sigmas, segment):
    f = lib().o_rho
    f.restype = C.c_double
    s = np.asarray(start, dtype=np.float64); g = np.asarray(sigmas, dtype=np.float64)
    sg = np.asarray(segment, dtype=np.float64)
    return f(C.c_double(point[0]), C.c_double(point[1]), C.c_double(point[2]), C.c_double(q), _p(s), _p(g), _p(sg))


def unique_pixels(neigh):
    u = np.unique(neigh.ravel())
    return u[u != -1].astype(np.int32)


def pixel_index_map(neigh, unique_pix):
    """cli/simulate_pixels.py:1019-1026 restated with searchsorted (unique_pix is sorted)."""
    idx = np.searchsorted(unique_pix, neigh)
    idx = np.clip(idx, 0, max(len(unique_pix) - 1, 0))
    ok = (neigh >= 0) & (len(unique_pix) > 0)
    ok &= unique_pix[idx] == neigh if len(unique_pix) else False
    return np.where(ok, idx, -1).astype(np.int64)


def track_pixel_map(unique_pix, neigh, nrad, max_distance, M):
    U = len(unique_pix)
    S, P = neigh.shape
    m = np.full((U, M), -1, dtype=np.int64)
    lib().o_track_pixel_map(_p(m), _p(np.ascontiguousarray(unique_pix, dtype=np.int32)), C.c_int64(U),
                            _p(np.ascontiguousarray(neigh, dtype=np.int32)),
                            _p(np.ascontiguousarray(nrad, dtype=np.int32)), C.c_int64(S), C.c_int64(P),
                            C.c_int(max_distance), C.c_int64(M))
    return m


def sum_pixel_signals(signals, track_starts, pim, tpm, U, want_tracks=True):
    c = _consts()
    S, P, T = signals.shape
    NT = c.n_time_ticks
    M = tpm.shape[1]
    ps = np.zeros((U, NT))
    pts = np.zeros((U, NT, M)) if want_tracks else None
    ovf = np.zeros(U)
    lib().o_sum_pixel_signals(_p(ps), _p(np.ascontiguousarray(signals)), _p(np.ascontiguousarray(track_starts)),
                              _p(np.ascontiguousarray(pim, dtype=np.int64)),
                              _p(np.ascontiguousarray(tpm, dtype=np.int64)), _p(pts), _p(ovf), C.c_int64(S),
                              C.c_int64(P), C.c_int64(T), C.c_int64(NT), C.c_int64(M), C.byref(c))
    return ps, pts, ovf


def tracks_current_mc(tracks, pixels, T, response, rng_states):
    """o_tracks_current_mc: signals f32 [S][P][T]; rng_states (RNG_DTYPE, S*P entries) are stepped once."""
    o = to_oracle(tracks)
    c = _consts(noise_zero=False)
    S, P = pixels.shape
    sig = np.zeros((S, P, T), dtype=np.float32)
    resp = np.ascontiguousarray(response, dtype=np.float64)
    pix = np.ascontiguousarray(pixels, dtype=np.int32)
    assert rng_states.dtype == RNG_DTYPE and len(rng_states) >= S * P
    lib().o_tracks_current_mc(_p(sig), _p(pix), _p(o), C.c_int64(S), C.c_int64(P), C.c_int64(T), _p(resp),
                              C.c_int64(resp.shape[0]), C.c_int64(resp.shape[1]), C.c_int64(resp.shape[2]), C.byref(c),
                              _p(rng_states))
    return sig


def _mc_outputs(S, P, T, want):
    sig = np.zeros((S, P, T), dtype=np.float32)
    out = {"signals": sig}
    if want:
        out.update(signals64=np.zeros((S, P, T)), n_draws=np.zeros((S, P, T), dtype=np.int32), margin=np.zeros((S, P, T)))
    return out


def tracks_current_mc_detail(tracks, pixels, T, response, rng_states):
    """``tracks_current_mc`` (same streams, same bits in ``signals``, the states stepped once) with what the loop knows besides:
    dict(signals f32, signals64 the unrounded sums, n_draws i4 the normals each (segment, pixel, tick) drew, margin f8: the
    smallest move of one of its draws that changes a decision -- an edge of the time window, a reach cut, a half-integer of the
    roundings for i, j, k -- in spacings of float32 at that draw's Box-Muller radius; +inf where nothing was decided)."""
    o = to_oracle(tracks)
    c = _consts(noise_zero=False)
    S, P = pixels.shape
    out = _mc_outputs(S, P, T, True)
    resp = np.ascontiguousarray(response, dtype=np.float64)
    pix = np.ascontiguousarray(pixels, dtype=np.int32)
    assert rng_states.dtype == RNG_DTYPE and len(rng_states) >= S * P
    lib().o_tracks_current_mc_ex(_p(out["signals"]), _p(out["signals64"]), _p(out["n_draws"]), _p(out["margin"]), _p(pix), _p(o),
                                 C.c_int64(S), C.c_int64(P), C.c_int64(T), _p(resp), C.c_int64(resp.shape[0]),
                                 C.c_int64(resp.shape[1]), C.c_int64(resp.shape[2]), C.byref(c), _p(rng_states))
    return out


def tracks_current_mc_normals(tracks, pixels, T, response, normals, radii=None):
    """The loop of ``tracks_current_mc`` on supplied normals: draw d of entry (itrk, ipix, it) is ``normals[itrk, ipix, it, d]``
    (f32 [S][P][T][D]; D at least the largest count an entry needs, else ValueError).  ``radii``: the Box-Muller radius of
    each normal, for the margin (None: the margin takes the spacing at |normal|, which is not above the radius's).  Returns
    the dict of ``tracks_current_mc_detail``."""
    o = to_oracle(tracks)
    c = _consts(noise_zero=False)
    S, P = pixels.shape
    nrm = np.ascontiguousarray(normals, dtype=np.float32)
    assert nrm.shape[:3] == (S, P, T), (nrm.shape, (S, P, T))
    rad = None if radii is None else np.ascontiguousarray(radii, dtype=np.float32)
    assert rad is None or rad.shape == nrm.shape
    out = _mc_outputs(S, P, T, True)
    resp = np.ascontiguousarray(response, dtype=np.float64)
    pix = np.ascontiguousarray(pixels, dtype=np.int32)
    rc = lib().o_tracks_current_mc_normals(_p(out["signals"]), _p(out["signals64"]), _p(out["n_draws"]), _p(out["margin"]),
                                           _p(pix), _p(o), C.c_int64(S), C.c_int64(P), C.c_int64(T), _p(resp),
                                           C.c_int64(resp.shape[0]), C.c_int64(resp.shape[1]), C.c_int64(resp.shape[2]),
                                           C.byref(c), _p(nrm), _p(rad), C.c_int64(nrm.shape[3]))
    if rc:
        raise ValueError(f"tracks_current_mc_normals: an entry needs more than the {nrm.shape[3]} normals supplied per entry")
    return out


def mc_stream_normals(rng_states, S, P, T, D, segments=None, count=None, want_radii=False):
    """The normals ``tracks_current_mc`` draws in table mode among S segments, as arrays for the segments ``(begin, end)``
    (None: all): draws 0 .. D-1 (``count`` i4 [n][P][T]: only the first count[entry]; the rest stay 0) of the stream of every
    (itrk, ipix, it) -- ``mc_stream_words(states[itrk + S*ipix], it)`` then the xoroshiro128p Box-Muller normals.
    f32 [n][P][T][D], with the radii when asked.  The states are not stepped."""
    assert rng_states.dtype == RNG_DTYPE and len(rng_states) >= S * P
    b, e = (0, S) if segments is None else segments
    nrm = np.zeros((e - b, P, T, D), dtype=np.float32)
    rad = np.zeros((e - b, P, T, D), dtype=np.float32) if want_radii else None
    cnt = None if count is None else np.ascontiguousarray(count, dtype=np.int32)
    assert cnt is None or cnt.shape == (e - b, P, T)
    lib().o_mc_table_normals(_p(rng_states), C.c_int64(S), C.c_int64(P), C.c_int64(T), C.c_int64(b), C.c_int64(e), C.c_int64(D),
                             _p(cnt), _p(nrm), _p(rad))
    return (nrm, rad) if want_radii else nrm


RNG_DTYPE =np.dtype([("s0", "<u8"), ("s1", "<u8")])     # numba.cuda.random.xoroshiro128p_dtype


def rng_create_states(n, seed):
    """numba.cuda.random.create_xoroshiro128p_states(n, seed) restated (oracle/ldsim_oracle.c: unpinned)."""
    st = np.zeros(n, dtype=RNG_DTYPE)
    lib().o_rng_create_states(_p(st), C.c_int64(n), C.c_uint64(int(seed) & (2 ** 64 - 1)))
    return st


def rng_normals(states, index, count):
    """`count` successive xoroshiro128p_normal_float32(states, index) draws (advances states[index])."""
    out = np.zeros(count, dtype=np.float32)
    ptr = C.c_void_p(states.ctypes.data + int(index) * RNG_DTYPE.itemsize)
    lib().o_rng_normals_fill(ptr, C.c_int64(int(count)), _p(out))
    return out


def get_adc_values(pixels_signals, pixels_tracks_signals, time_ticks, thresholds, time_padding=0.0,
                   want_fractions=True, rng_states=None):
    """rng_states = None: noise terms 0.  Else the xoroshiro128p states (RNG_DTYPE, one per pixel, advanced in place) and the
    noise charges of ``consts.detector`` as they stand."""
    c = _consts()
    if rng_states is not None:
        c = _consts(noise_zero=False)
        U, NT = pixels_signals.shape
        A = c.max_adc_values
        M = pixels_tracks_signals.shape[2] if pixels_tracks_signals is not None else c.max_tracks_per_pixel
        adc = np.zeros((U, A)); ticks = np.zeros((U, A))
        frac = np.zeros((U, A, M)) if (want_fractions and pixels_tracks_signals is not None) else None
        assert rng_states.dtype == RNG_DTYPE and len(rng_states) >= U
        lib().o_get_adc_values_rng(_p(np.ascontiguousarray(pixels_signals)), _p(pixels_tracks_signals),
                                   _p(np.ascontiguousarray(time_ticks)), C.c_int64(len(time_ticks)), _p(adc), _p(ticks),
                                   C.c_double(time_padding), _p(frac),
                                   _p(np.ascontiguousarray(thresholds, dtype=np.float64)), C.c_int64(U), C.c_int64(NT),
                                   C.c_int64(M), C.byref(c), _p(rng_states))
        return adc, ticks, frac
    U, NT = pixels_signals.shape
    A = c.max_adc_values
    M = pixels_tracks_signals.shape[2] if pixels_tracks_signals is not None else c.max_tracks_per_pixel
    adc = np.zeros((U, A)); ticks = np.zeros((U, A))
    frac = np.zeros((U, A, M)) if (want_fractions and pixels_tracks_signals is not None) else None
    lib().o_get_adc_values(_p(np.ascontiguousarray(pixels_signals)),
                           _p(pixels_tracks_signals), _p(np.ascontiguousarray(time_ticks)),
                           C.c_int64(len(time_ticks)), _p(adc), _p(ticks), C.c_double(time_padding), _p(frac),
                           _p(np.ascontiguousarray(thresholds, dtype=np.float64)), C.c_int64(U), C.c_int64(NT),
                           C.c_int64(M), C.byref(c))
    return adc, ticks, frac


def digitize(integral, gain=None):
    c = _consts()
    integral = np.ascontiguousarray(integral, dtype=np.float64)
    out = np.empty_like(integral)
    g = None if gain is None else np.ascontiguousarray(np.broadcast_to(gain, integral.shape), dtype=np.float64)
    lib().o_digitize(_p(integral), C.c_int64(integral.size), _p(g), _p(out), C.byref(c))
    return out


def light_incidence(tracks, lut, n_out=None, init=None):
    """``init``: (n_photons_det, t0_det, voxel) the call writes into, like the reference into its caller's arrays (rows of
    segments outside every TPC, and t0_det in trigger mode 1, keep what they hold); default zeros."""
    o = to_oracle(tracks)
    c = _consts()
    n = len(o)
    n_out = c.n_op_channel if n_out is None else n_out
    vis = np.ascontiguousarray(lut['vis'], dtype=np.float32)
    t0 = np.ascontiguousarray(lut['t0'], dtype=np.float32)
    nx, ny, nz, ndet = lut.shape
    eff = np.ascontiguousarray(consts.light.OP_CHANNEL_EFFICIENCY, dtype=np.float64)
    c2t = np.ascontiguousarray(consts.light.OP_CHANNEL_TO_TPC, dtype=np.int32)
    nph = np.zeros((n, n_out), dtype=np.float32); t0d = np.zeros((n, n_out), dtype=np.float32)
    vox = np.zeros((n, 3), dtype=np.int32)
    if init is not None:
        nph, t0d, vox = (np.array(a, dtype=d, order='C') for a, d in zip(init, (np.float32, np.float32, np.int32)))
        assert nph.shape == (n, n_out) and t0d.shape == (n, n_out) and vox.shape == (n, 3)
    lib().o_light_incidence(_p(o), C.c_int64(n), _p(vis), _p(t0), C.c_int(nx), C.c_int(ny), C.c_int(nz),
                            C.c_int(ndet), _p(eff), _p(c2t), C.c_int(n_out), _p(nph), _p(t0d), _p(vox), C.byref(c))
    return nph, t0d, vox


def sum_light_signals(tracks, voxel, track_id, n_photons_det, op_channel, lut, start_time, n_ticks,
                      sorted_indices, max_truth=0, init=None):
    """``init``: (light_sample_inc, true ids, true photons) the sum adds into, like the reference into its caller's arrays;
    default zeros and -1."""
    o = to_oracle(tracks)
    c = _consts()
    n = len(o)
    nx, ny, nz, ndet = lut.shape
    nprof = lut['time_dist'].shape[-1]
    t0_avg = np.ascontiguousarray(lut['t0_avg'], dtype=np.float32)
    td = np.ascontiguousarray(lut['time_dist'], dtype=np.float32)
    n_det = len(op_channel)
    out = np.zeros((n_det, n_ticks), dtype=np.float32)
    tid = np.full((n_det, n_ticks, max(max_truth, 1)), -1, dtype=np.int64)
    tph = np.zeros((n_det, n_ticks, max(max_truth, 1)))
    if init is not None:
        out = np.array(init[0], dtype=np.float32, order='C')
        assert out.shape == (n_det, n_ticks)
        if max_truth:
            tid, tph = np.array(init[1], dtype=np.int64, order='C'), np.array(init[2], dtype=np.float64, order='C')
            assert tid.shape == tph.shape == (n_det, n_ticks, max_truth)
    lib().o_sum_light_signals(_p(o), C.c_int64(n), _p(np.ascontiguousarray(voxel, dtype=np.int32)),
                              _p(np.ascontiguousarray(track_id, dtype=np.int64)),
                              _p(np.ascontiguousarray(n_photons_det, dtype=np.float32)),
                              C.c_int(n_photons_det.shape[1]), _p(np.ascontiguousarray(op_channel, dtype=np.int32)),
                              C.c_int(n_det), _p(t0_avg), _p(td), C.c_int(nx), C.c_int(ny), C.c_int(nz),
                              C.c_int(ndet), C.c_int(nprof), C.c_double(start_time),
                              _p(np.ascontiguousarray(sorted_indices, dtype=np.int32)), C.c_int64(n_ticks), _p(out),
                              _p(tid), _p(tph), C.c_int(max_truth), C.byref(c))
    return out, tid[:, :, :max_truth], tph[:, :, :max_truth]


def _light_truth(tid, tph, D, T):
    if tid is None or tid.shape[-1] == 0:
        return 0, None, None
    return tid.shape[-1], np.ascontiguousarray(tid, dtype=np.int64), np.ascontiguousarray(tph, dtype=np.float64)


def scintillation_effect(light_sample_inc, true_id=None, true_photons=None):
    """light_sim.calc_scintillation_effect: returns (scint f4[D][T], true ids i8, true photons f8)."""
    c = _consts()
    inc = np.ascontiguousarray(light_sample_inc, dtype=np.float32)
    D, T = inc.shape
    Mt, tid, tph = _light_truth(true_id, true_photons, D, T)
    out = np.zeros((D, T), dtype=np.float32)
    otid = np.full((D, T, Mt), -1, dtype=np.int64); otph = np.zeros((D, T, Mt))
    lib().o_scintillation_effect(_p(inc), _p(tid), _p(tph), C.c_int32(D), C.c_int32(T), C.c_int32(Mt), _p(out),
                                 _p(otid) if Mt else None, _p(otph) if Mt else None, C.byref(c))
    return out, otid, otph


def light_detector_response(light_sample_inc, light_gain, impulse_model, true_id=None, true_photons=None):
    """light_sim.calc_light_detector_response: returns (response f4[D][T], true ids i8, true photons f8)."""
    c = _consts()
    inc = np.ascontiguousarray(light_sample_inc, dtype=np.float32)
    D, T = inc.shape
    Mt, tid, tph = _light_truth(true_id, true_photons, D, T)
    gain = np.ascontiguousarray(light_gain, dtype=np.float64)
    imp = np.ascontiguousarray(impulse_model, dtype=np.float64)
    assert gain.shape[0] >= D
    out = np.zeros((D, T), dtype=np.float32)
    otid = np.full((D, T, Mt), -1, dtype=np.int64); otph = np.zeros((D, T, Mt))
    lib().o_light_detector_response(_p(inc), _p(tid), _p(tph), C.c_int32(D), C.c_int32(T), C.c_int32(Mt), _p(gain), _p(imp),
                                    C.c_int32(imp.shape[0]), _p(out), _p(otid) if Mt else None, _p(otph) if Mt else None,
                                    C.byref(c))
    return out, otid, otph



# ---- light: fluctuations, triggers, noise, digitisation (light_sim.py:186-238, 339-619) -------------------------------------
def stat_fluctuations(light_sample_inc, rng_states):
    """light_sim.calc_stat_fluctuations: element (idet, itick) draws from rng_states[idet*ntick + itick] (advanced in place)."""
    c = _consts()
    inc = np.ascontiguousarray(light_sample_inc, dtype=np.float32)
    assert rng_states.dtype == RNG_DTYPE and len(rng_states) >= inc.size
    out = np.zeros(inc.shape, dtype=np.float32)
    lib().o_stat_fluctuations(_p(inc), C.c_int64(inc.size), _p(rng_states), _p(out), C.byref(c))
    return out


def get_triggers(signal, group_threshold, op_channel_idx, i_subbatch):
    """light_sim.get_triggers (:339-443): (trigger tick indices, op channels per trigger, trigger type).
    The group sum keeps the array's f4 (rows added in order), the padded copy and the sample mean are f8, and the
    threshold loop keeps the reference's bookkeeping (the slice offset of the third and later triggers of a module is the
    absolute tick of the previous trigger, not the relative one -- :404-411 -- so those indices come out the way the
    reference computes them, not where the waveform crosses)."""
    light, detector = consts.light, consts.detector
    signal = np.asarray(signal)
    op_channel_idx = np.asarray(op_channel_idx)
    nd, nt = signal.shape
    per = light.OP_CHANNEL_PER_TRIG
    ng = nd // per
    gsum = signal.reshape(ng, per, nt).sum(axis=1, keepdims=True)
    sf = round(light.LIGHT_DIGIT_SAMPLE_SPACING / light.LIGHT_TICK_SIZE)
    padding = sf - nt % sf
    if padding > 0:
        gsum = np.concatenate((gsum, np.zeros((ng, 1, padding))), axis=-1)
    blocks = gsum.reshape(-1, 1, gsum.shape[-1] // sf, sf).mean(axis=-1, keepdims=True)
    flat = np.broadcast_to(blocks, blocks.shape[:3] + (sf,)).reshape(-1, 1, nt + padding)
    flat = flat[..., :(-padding if padding > 0 else nt)]
    above = np.broadcast_to(flat < np.asarray(group_threshold)[:, None, None], (ng, per, nt)).reshape(nd, nt)
    digit_ticks = int(np.ceil((light.LIGHT_TRIG_WINDOW[1] + light.LIGHT_TRIG_WINDOW[0]) / light.LIGHT_TICK_SIZE))
    tpcs = np.unique(light.OP_CHANNEL_TO_TPC[op_channel_idx])
    mods = np.unique([detector.TPC_TO_MODULE[int(t)] for t in tpcs])
    trig, chans, types = [], [], []
    if light.LIGHT_TRIG_MODE == 0:
        for mod in mods:
            mod_channels = light.TPC_TO_OP_CHANNEL[detector.MODULE_TO_TPCS[mod]].ravel()
            rows = np.isin(op_channel_idx, mod_channels)
            hot = np.any(above[rows], axis=0)
            last = 0
            while np.any(hot):
                nxt = int(np.flatnonzero(hot)[0]) + last
                trig.append(nxt); types.append(0); chans.append(mod_channels)
                hot = hot[nxt + digit_ticks:]
                last = nxt + digit_ticks
    elif light.LIGHT_TRIG_MODE == 1 and i_subbatch == 0:
        trig.append(0); chans.append(op_channel_idx); types.append(1)
    if trig:
        return np.array(trig), np.array(chans), np.array(types)
    return np.empty((0,), dtype=int), np.empty((0, len(op_channel_idx)), dtype=int), np.empty((0,), dtype=int)


def gen_light_detector_noise(shape, light_det_noise, phases):
    """light_sim.gen_light_detector_noise (:445-478) with the uniform random phases handed in (`phases`, shape
    (shape[0], shape[1]//2 + 1), what cp.random.uniform(size=noise_spectrum.shape) returns there)."""
    light = consts.light
    if not shape[0]:
        return np.empty(shape)
    light_det_noise = np.asarray(light_det_noise, dtype=np.float64)
    noise_freq = np.fft.rfftfreq((light_det_noise.shape[-1] - 1) * 2, d=light.LIGHT_DET_NOISE_SAMPLE_SPACING)
    desired_freq = np.fft.rfftfreq(shape[-1], d=light.LIGHT_TICK_SIZE)
    bin_size = np.diff(desired_freq).mean()
    spec = np.zeros((shape[0], desired_freq.shape[0]))
    for idet in range(shape[0]):
        spec[idet] = np.interp(desired_freq, noise_freq, light_det_noise[idet], left=0, right=0)
    spec *= np.sqrt(np.diff(noise_freq, axis=-1).mean() / bin_size) * light.LIGHT_DIGIT_SAMPLE_SPACING / light.LIGHT_TICK_SIZE
    noise = spec * np.exp(2j * np.pi * np.asarray(phases))
    scale = 2 ** (16 - light.LIGHT_NBIT)
    if shape[1] < 2:
        noise = np.round(np.real(noise)) * scale
    else:
        noise = np.round(np.fft.irfft(noise, axis=-1)) * scale
    if noise.shape[1] < shape[1]:
        noise = np.concatenate([noise, np.zeros((noise.shape[0], shape[1] - noise.shape[1]))], axis=-1)
    return noise[:, :shape[1]]


def sim_triggers(signal, signal_op_channel_idx, signal_true_track_id, signal_true_photons, trigger_idx, op_channel_idx,
                 digit_samples, light_det_noise, phases_signal=None, phases_missing=None):
    """light_sim.sim_triggers (:545-619).  phases_* = the uniform numbers of the two gen_light_detector_noise calls (None =
    zero spectrum expected).  Returns (digit_signal f8, true ids i8, true photons f8)."""
    light = consts.light
    c = _consts()
    signal = np.asarray(signal)
    sop = np.asarray(signal_op_channel_idx).astype(np.int64)
    tid = np.asarray(signal_true_track_id, dtype=np.int64)
    tph = np.asarray(signal_true_photons, dtype=np.float64)
    trigger_idx = np.asarray(trigger_idx).astype(np.int64)
    op_channel_idx = np.asarray(op_channel_idx).astype(np.int64)
    Mt = tid.shape[-1]
    ntrig, ndm = trigger_idx.shape[0], op_channel_idx.shape[-1]
    digit = np.zeros((ntrig, ndm, digit_samples))
    dtid = np.full((ntrig, ndm, digit_samples, Mt), -1, dtype=np.int64)
    dtph = np.zeros((ntrig, ndm, digit_samples, Mt))
    if ntrig == 0:
        return digit, dtid, dtph
    padded = trigger_idx.copy()
    pre = int(np.ceil(light.LIGHT_TRIG_WINDOW[0] / light.LIGHT_TICK_SIZE))
    if trigger_idx.min() - pre < 0:
        n0 = int(pre - trigger_idx.min())
        signal = np.concatenate([np.zeros((signal.shape[0], n0)), signal], axis=-1)
        tid = np.concatenate([np.full((tid.shape[0], n0, Mt), -1, dtype=np.int64), tid], axis=1)
        tph = np.concatenate([np.zeros((tph.shape[0], n0, Mt)), tph], axis=1)
        padded += n0
    post = int(np.ceil(light.LIGHT_TRIG_WINDOW[1] / light.LIGHT_TICK_SIZE))
    if post + padded.max() > signal.shape[1]:
        n1 = int(post + padded.max() - signal.shape[1])
        signal = np.concatenate([signal, np.zeros((signal.shape[0], n1))], axis=-1)
        tid = np.concatenate([tid, np.full((tid.shape[0], n1, Mt), -1, dtype=np.int64)], axis=1)
        tph = np.concatenate([tph, np.zeros((tph.shape[0], n1, Mt))], axis=1)
    noise_tab = np.asarray(light_det_noise, dtype=np.float64)
    if phases_signal is None:
        assert not np.any(noise_tab[sop]), "phases needed for a non-zero noise spectrum"
        phases_signal = np.zeros((signal.shape[0], signal.shape[1] // 2 + 1))
    signal = signal.copy()
    signal += gen_light_detector_noise(signal.shape, noise_tab[sop], phases_signal)     # f4 += f8 rounds to f4 if still f4
    absent = ~np.isin(op_channel_idx, sop)
    if np.any(absent):
        missing = np.unique(op_channel_idx[absent])
        if phases_missing is None:
            assert not np.any(noise_tab[missing])
            phases_missing = np.zeros((missing.shape[0], signal.shape[1] // 2 + 1))
        signal = np.concatenate([signal, gen_light_detector_noise((missing.shape[0], signal.shape[1]), noise_tab[missing],
                                                                  phases_missing)], axis=0)
        sop = np.concatenate([sop, missing])
        tid = np.concatenate([tid, np.full((missing.shape[0],) + tid.shape[1:], -1, dtype=np.int64)], axis=0)
        tph = np.concatenate([tph, np.zeros((missing.shape[0],) + tph.shape[1:])], axis=0)
        order = np.argsort(sop)
        signal, sop, tid, tph = signal[order], sop[order], tid[order], tph[order]
    # the dtype digitize_signal sees: f4 only if nothing was padded (:578, :589) and no f8 noise rows were appended (:601)
    sig_is_f4 = signal.dtype == np.float32
    sig = np.ascontiguousarray(signal, dtype=np.float64)
    tid = np.ascontiguousarray(tid); tph = np.ascontiguousarray(tph); sop = np.ascontiguousarray(sop)
    top = np.ascontiguousarray(np.broadcast_to(op_channel_idx, (ntrig, ndm)) if op_channel_idx.ndim == 1 else op_channel_idx)
    lib().o_digitize_signal(_p(sig), C.c_int(int(sig_is_f4)), _p(sop), C.c_int64(sig.shape[0]), C.c_int64(sig.shape[1]),
                            _p(top), C.c_int64(ntrig), C.c_int64(ndm), _p(tid), _p(tph), C.c_int32(Mt),
                            C.c_int64(digit_samples), _p(digit), _p(dtid), _p(dtph), C.byref(c))
    scale = 2 ** (16 - light.LIGHT_NBIT)
    digit = np.round(digit / scale) * scale
    return digit, dtid, dtph
