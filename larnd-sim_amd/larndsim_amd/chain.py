"""
Device-resident charge chain: segments stay in HBM from quench to ADC.

Replaces the body of the reference's batch loop (cli/simulate_pixels.py:917-1105: max_pixels ->
get_pixels -> unique -> time_intervals -> tracks_current -> pixel_index_map -> get_track_pixel_map2 ->
sum_pixel_signals -> get_adc_values -> digitize) for any number of (event, TPC-group) batches per call.
"""
import ctypes as C

import numpy as np

from . import consts, lib
from .abi import LdsimChainStats, LdsimSipmNoise
from .layout import make_layout


class ChargeChain:
    def __init__(self, response=None, device=None):
        lib.claim_chain(self)
        self.ctx = lib.context(device=device, noise_zero=False)
        self._generation = lib.consts_generation()
        self.n = 0
        if response is not None:
            lib.set_response(response, self.ctx)
        self.clear_field_map()          # the ctx is process-wide: a fresh chain starts with the uniform field
        self.set_charge_statistics(False)                         # ... and with mean-value charge
        self.set_sipm_noise(enable=False)                         # ... and with the plain Poisson light fluctuations

    def set_field_map(self, maps):
        """Drift-field maps (``field_map``: {tpc: {"origin", "spacing", "E" / "dx" / "dy" / "dz"}}, or the path of an .npz),
        replacing any set before.  Takes effect at the next ``quench_drift``; the charge chain then reads the anode view,
        the light leg and ``download_segments`` the true positions."""
        from . import field_map
        n_tpc = len(consts.detector.TPC_BORDERS)
        maps = field_map.load(maps, n_tpc) if isinstance(maps, (str, bytes)) or hasattr(maps, "__fspath__") \
            else field_map.validate(maps, n_tpc)
        L = lib.load()
        lib.check(L.ldsim_clear_field_maps(self.ctx))
        for tpc, m in sorted(maps.items()):
            shape = np.array(next(m[ch] for ch in field_map.CHANNELS if ch in m).shape, dtype=np.int64)
            lib.check(L.ldsim_set_field_map(self.ctx, C.c_int32(tpc), lib.ptr(shape), lib.ptr(m["origin"]),
                                            lib.ptr(m["spacing"]), *(lib.ptr(m.get(ch)) for ch in field_map.CHANNELS)))
        self.field_maps = maps

    def clear_field_map(self):
        """back to the uniform field (upload or reset, then quench_drift, before the next run)"""
        lib.check(lib.load().ldsim_clear_field_maps(self.ctx))
        self.field_maps = {}

    def download_anode_view(self):
        """[9][n] f64: the positions the charge stages read after a mapped ``quench_drift`` (x_start, y_start, z_start,
        x_end, y_end, z_end, x, y, z)"""
        out = np.empty((9, self.n), dtype=np.float64)
        lib.check(lib.load().ldsim_dev_anode_view_download(self.ctx, lib.ptr(out)))
        return out

    def set_charge_statistics(self, enable=True, fano=0.107):
        """Charge statistics (``charge_stats``): the next ``quench_drift`` counts ion pairs (Fano factor ``fano``) and draws
        recombination and attachment as binomials from keyed streams, instead of writing mean values.  Needs ``seed_keyed`` and
        ``set_batch_keys`` before ``quench_drift``; ``run`` refuses until ``quench_drift`` has run under the new setting."""
        lib.check(lib.load().ldsim_set_charge_statistics(self.ctx, C.c_int32(int(bool(enable))), C.c_double(float(fano))))

    def charge_statistics(self):
        """(enabled, Fano factor) as the context holds them"""
        on, f = C.c_int32(), C.c_double()
        lib.check(lib.load().ldsim_get_charge_statistics(self.ctx, C.byref(on), C.byref(f)))
        return bool(on.value), f.value

    def set_sipm_noise(self, crosstalk=0.0, afterpulse=0.0, afterpulse_tau=0.1, dark_rate=0.0, enable=True):
        """SiPM correlated noise (``sipm_noise``) in the fluctuation stage of ``light_response`` and ``light_universes``: prompt
        cross-talk (``crosstalk`` secondary avalanches per avalanche, 0 .. 0.5), after-pulses (probability ``afterpulse`` per
        avalanche, 0 .. 0.5, mean delay ``afterpulse_tau`` us) and dark counts (``dark_rate`` per us and detector row).  Needs
        ``seed_keyed``; ``enable=False`` switches it off and keeps the context's values."""
        v = LdsimSipmNoise(float(crosstalk), float(afterpulse), float(afterpulse_tau), float(dark_rate))
        lib.check(lib.load().ldsim_set_sipm_noise(self.ctx, C.c_int32(int(bool(enable))), C.byref(v) if enable else None))

    def sipm_noise(self):
        """(enabled, {crosstalk, afterpulse, afterpulse_tau, dark_rate}) as the context holds them"""
        on, v = C.c_int32(), LdsimSipmNoise()
        lib.check(lib.load().ldsim_get_sipm_noise(self.ctx, C.byref(on), C.byref(v)))
        return bool(on.value), {f: getattr(v, f) for f, _ in LdsimSipmNoise._fields_}

    def seed_rng(self, seed, n_states=1024 * 256):
        """``create_xoroshiro128p_states(1024*256, seed=rand_seed)`` of the driver (cli/simulate_pixels.py:396): needed before
        ``run`` when a FEE noise charge is non-zero.  Row u of a launch draws from state u of the table."""
        from . import rng
        self.rng_states = rng.create_xoroshiro128p_states(n_states, seed, self.ctx)
        return self.rng_states

    def extend_rng(self, n_states, seed):
        """``maybe_create_rng_states(n, seed, rng_states)`` (cli/simulate_pixels.py:92-104) on the ctx's table."""
        lib.check(lib.load().ldsim_rng_extend(self.ctx, C.c_int64(int(n_states)), C.c_uint64(int(seed) & (2 ** 64 - 1))))

    def seed_keyed(self, seed):
        """Keyed random mode (csrc/rng.h): drop the table; every draw becomes a function of (seed, stage, identity of what is
        simulated, draw index).  A run then needs ``set_batch_keys`` after each ``upload`` and ``set_rng_key`` before the light
        calls of a sub-batch.  ``seed_rng`` switches back to table mode."""
        lib.check(lib.load().ldsim_rng_keyed_seed(self.ctx, C.c_uint64(int(seed) & (2 ** 64 - 1))))

    def set_batch_keys(self, table, i_mod):
        """keyed mode: the keys of the uploaded batches, from their identities in ``batching.assign_batches``' table"""
        from . import rng
        keys = np.ascontiguousarray(rng.batch_keys(table, i_mod), dtype=np.uint64)
        lib.check(lib.load().ldsim_chain_set_batch_keys(self.ctx, lib.ptr(keys), C.c_int64(len(keys))))

    def set_rng_key(self, key):
        """keyed mode: identity key (rng.call_key) of the light response / trigger / noise calls that follow"""
        lib.check(lib.load().ldsim_rng_set_call_key(self.ctx, C.c_uint64(int(key) & (2 ** 64 - 1))))

    def _check_constants(self):
        """The ctx is process-wide and this object froze its constants at construction: refuse to compute once anything
        (another ChargeChain, a stage call after ``consts`` was reloaded) has frozen different ones."""
        if lib.consts_generation() != self._generation:
            raise lib.LdsimError("the detector constants frozen in the GPU context changed since this ChargeChain was "
                                 "created: create a new ChargeChain (and upload again) after loading another configuration")

    def refresh_constants(self):
        """Adopt the constants currently in ``consts`` for this chain (e.g. after changing DISCRIMINATION_THRESHOLD),
        keeping the resident segments.  What was derived under the old constants is the caller's business: drifted
        segments are not recomputed, and pixel tables of another geometry make the next run fail (LDSIM_ESTATE)."""
        self.ctx = lib.context(noise_zero=False)
        self._generation = lib.consts_generation()

    def upload(self, tracks, batch_id=None):
        """H2D + unpack into the SoA segment store. ``batch_id``: int32 per segment, non-decreasing, <0 = skip."""
        self._check_constants()
        lay = make_layout(tracks.dtype)
        self._layout = lay
        b = None if batch_id is None else np.ascontiguousarray(batch_id, dtype=np.int32)
        tr = np.ascontiguousarray(tracks)
        lib.check(lib.load().ldsim_segments_upload(self.ctx, lib.ptr(tr), C.c_int64(tr.shape[0]), C.byref(lay),
                                                   lib.ptr(b)))
        self.n = tr.shape[0]

    def reset(self):
        """Re-unpack the resident records (undo quench/drift) without another H2D copy."""
        lib.check(lib.load().ldsim_segments_reset(self.ctx))

    def synchronize(self):
        lib.check(lib.load().ldsim_synchronize(self.ctx))

    def quench_drift(self, mode=None):
        self._check_constants()
        mode = consts.physics.BIRKS if mode is None else mode
        lib.check(lib.load().ldsim_dev_quench_drift(self.ctx, C.c_int32(int(mode))))

    def download_segments(self, tracks):
        lay = make_layout(tracks.dtype)
        lib.check(lib.load().ldsim_segments_download(self.ctx, lib.ptr(tracks), C.c_int64(tracks.shape[0]),
                                                     C.byref(lay)))
        return tracks

    def run(self, seg_begin=0, seg_end=None, want_fractions=False):
        self._check_constants()
        seg_end = self.n if seg_end is None else seg_end
        st = LdsimChainStats()
        lib.check(lib.load().ldsim_charge_chain(self.ctx, C.c_int64(seg_begin), C.c_int64(seg_end),
                                                C.c_int32(int(want_fractions)), C.byref(st)))
        self.stats = st
        self._want_fractions = bool(want_fractions)
        return st

    def run_async(self, seg_begin=0, seg_end=None, want_fractions=False):
        """``run`` on a worker thread: the C call blocks (a chain launch reads sizes back from the device five times) but releases
        the interpreter, so the caller can do host work that does not enter the ctx meanwhile -- the bundled driver builds the
        previous launch's packets (``ldsim_packets_build`` takes no ctx).  ``wait()`` joins and returns the launch's statistics.
        Any other call into the ctx before ``wait()`` is refused by the library (LDSIM_ESTATE: a ctx serves one thread at a time)."""
        import threading
        if getattr(self, "_worker", None) is not None:
            raise lib.LdsimError("a chain launch is already in flight: wait() first")
        box = {}

        def work():
            try:
                box["st"] = self.run(seg_begin, seg_end, want_fractions)
            except BaseException as e:          # handed to wait()
                box["err"] = e
        self._worker = (threading.Thread(target=work, name="ldsim-chain-launch"), box)
        self._worker[0].start()

    def wait(self):
        """Join the launch started by ``run_async`` and return its statistics (or raise what it raised)."""
        w = getattr(self, "_worker", None)
        if w is None:
            raise lib.LdsimError("no chain launch in flight")
        w[0].join()
        self._worker = None
        if "err" in w[1]:
            raise w[1]["err"]
        return w[1]["st"]

    def set_pixel_thresholds(self, keys, values, default):
        """Per-pixel discrimination thresholds of the fused chain: ``pixel_thresholds_lut[unique_pix]`` of the reference
        driver (cli/simulate_pixels.py:1079-1084).  Call after the constants are loaded."""
        self._set_table("ldsim_set_pixel_thresholds", keys, values, default)

    def set_pixel_gains(self, keys, values, default):
        """Per-pixel gains for the digitisation: ``pixel_gains_lut[unique_pix]`` (cli/simulate_pixels.py:1097-1100)."""
        self._set_table("ldsim_set_pixel_gains", keys, values, default)

    def clear_pixel_tables(self):
        """Back to DISCRIMINATION_THRESHOLD * e and GAIN * mV / e for every pixel."""
        lib.check(lib.load().ldsim_clear_pixel_tables(self.ctx))

    def _set_table(self, fn, keys, values, default):
        k = np.ascontiguousarray(keys, dtype=np.int32).ravel()
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        if k.shape != v.shape:
            raise ValueError("keys and values differ in length")
        self._check_constants()   # the table is dense over the pixel geometry this chain was created under
        lib.check(getattr(lib.load(), fn)(self.ctx, lib.ptr(k), lib.ptr(v), C.c_int64(k.size), C.c_double(float(default))))

    def kernel_ms(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        lib.check(lib.load().ldsim_chain_kernel_ms(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        w, m, f = C.c_double(), C.c_double(), C.c_double()
        lib.check(lib.load().ldsim_chain_kernel_ms_detail(self.ctx, C.byref(w), C.byref(m), C.byref(f)))
        return dict(current_ms=a.value, adc_ms=b.value, total_ms=c.value, weights_ms=w.value, mac_ms=m.value,
                    fallback_ms=f.value)

    def _pinned(self, name, shape, dtype):
        """view of a page-locked buffer kept per output (grown when too small); valid until the next pinned download"""
        n = int(np.prod(shape))
        pool = self.__dict__.setdefault("_pinned_pool", {})
        buf = pool.get(name)
        if buf is None or buf.size < n or buf.dtype != np.dtype(dtype):
            buf = pool[name] = lib.pinned_array((max(n + n // 4, 1),), dtype)
        return buf[:n].reshape(shape)

    def download(self, fractions=None, pinned=False):
        """Per-unique-(batch, pixel) results of the last run(), reference dtypes.  ``pinned``: the arrays are views of
        page-locked buffers owned by the chain (PCIe-rate copies, no 1 GB allocation per call); they are overwritten by the
        next pinned download."""
        U = int(self.stats.n_unique)
        A, M = consts.sim.MAX_ADC_VALUES, consts.sim.MAX_TRACKS_PER_PIXEL
        want_fr = fractions if fractions is not None else self._want_fractions
        if pinned:
            out = dict(unique_pix=self._pinned("unique_pix", (U,), np.int32), batch=self._pinned("batch", (U,), np.int32),
                       adc_list=self._pinned("adc_list", (U, A), np.float64),
                       adc_ticks_list=self._pinned("adc_ticks_list", (U, A), np.float64),
                       adc_digit=self._pinned("adc_digit", (U, A), np.float64),
                       track_pixel_map=self._pinned("track_pixel_map", (U, M), np.int64))
            fr = self._pinned("current_fractions", (U, A, M), np.float64) if want_fr else None
        else:
            out = dict(unique_pix=np.zeros(U, dtype=np.int32), batch=np.zeros(U, dtype=np.int32),
                       adc_list=np.zeros((U, A)), adc_ticks_list=np.zeros((U, A)), adc_digit=np.zeros((U, A)),
                       track_pixel_map=np.full((U, M), -1, dtype=np.int64))
            fr = np.zeros((U, A, M)) if want_fr else None
        if fr is not None:
            out['current_fractions'] = fr
        lib.check(lib.load().ldsim_chain_download(self.ctx, C.c_int64(U), lib.ptr(out['unique_pix']),
                                                  lib.ptr(out['batch']), lib.ptr(out['adc_list']),
                                                  lib.ptr(out['adc_ticks_list']), lib.ptr(out['adc_digit']),
                                                  lib.ptr(out['track_pixel_map']), lib.ptr(fr)))
        return out

    def build_compact(self):
        """``ldsim_chain_compact_build`` of the last run() in HBM: (hit pixels, hits, track entries, fraction entries)"""
        sizes = (C.c_int64 * 4)()
        lib.check(lib.load().ldsim_chain_compact_build(self.ctx, sizes))
        return tuple(int(v) for v in sizes)

    def download_compact(self):
        """The last run()'s results in compact form (``ldsim_chain_compact_build`` / ``_download``): what the exporter reads --
        hit pixels, their hits and the fractions of the track slots they have -- gathered on the device first: a few MB over
        PCIe instead of 13 KB per unique pixel.  ``expand_compact`` turns it into the dense rows of the hit pixels."""
        from .comm import HIT_ROW
        n_hp, n_hits, n_trk, n_frac = self.build_compact()
        out = dict(hit_pixels=np.zeros((n_hp, 5), dtype=np.int32), track_segments=np.zeros(n_trk, dtype=np.int64),
                   hit_rows=np.zeros(n_hits, dtype=HIT_ROW), hit_charge=np.zeros(n_hits), fractions=np.zeros(n_frac),
                   has_fractions=bool(self._want_fractions))
        lib.check(lib.load().ldsim_chain_compact_download(self.ctx, lib.ptr(out["hit_pixels"]), lib.ptr(out["track_segments"]),
                                                          lib.ptr(out["hit_rows"]), lib.ptr(out["hit_charge"]),
                                                          lib.ptr(out["fractions"])))
        return out

    def pixel_truth(self, min_abs_charge=0.0, dense=False):
        """Pixel charge truth of the last run() (``pixel_truth``, ``ldsim_chain_pixel_truth``): the induced charge per unique
        pixel and per (pixel, track), reduced on the device from what the launch left in HBM.  Returns
        ``dict(pixels=, tracks=)``: structured rows (``pixel_truth.PIXEL_ROW``: row, pixel_id, batch, n_hits, n_tracks, q_hits,
        q_induced, q_abs) of the pixels that hold a hit or saw ``q_abs >= min_abs_charge`` electrons (0 keeps every unique
        pixel), in row order, and their track entries (``pixel_truth.TRACK_ENTRY``: segment as in ``track_pixel_map``, q),
        pixel after pixel.  ``dense=True``: ``dict(q_induced [U], q_abs [U], q_track [U][M])`` in the row order of
        ``download()`` instead.  ``q_hits`` includes the FEE noise charges when noise is on; the other values never do.
        Raises ``LdsimError`` (LDSIM_ESTATE) once anything (upload, reset, quench_drift, a host-array stage call) may have
        rewritten the launch's buffers: ``run()`` again."""
        from . import pixel_truth as pt
        self._check_constants()
        L = lib.load()
        sizes = (C.c_int64 * 2)()
        lib.check(L.ldsim_chain_pixel_truth(self.ctx, C.c_double(float(min_abs_charge)), sizes))
        if dense:
            U, M = int(self.stats.n_unique), consts.sim.MAX_TRACKS_PER_PIXEL
            out = dict(q_induced=np.zeros(U), q_abs=np.zeros(U), q_track=np.zeros((U, M)))
            lib.check(L.ldsim_chain_pixel_truth_dense_download(self.ctx, C.c_int64(U), lib.ptr(out["q_induced"]),
                                                               lib.ptr(out["q_abs"]), lib.ptr(out["q_track"])))
            return out
        out = dict(pixels=np.zeros(int(sizes[0]), dtype=pt.PIXEL_ROW), tracks=np.zeros(int(sizes[1]), dtype=pt.TRACK_ENTRY))
        lib.check(L.ldsim_chain_pixel_truth_download(self.ctx, lib.ptr(out["pixels"]), lib.ptr(out["tracks"])))
        return out

    def pixel_truth_row_samples(self):
        """current samples the pixel-truth pass sums for the last run() (``ldsim_chain_pixel_truth_row_samples``, timing tools):
        the bytes it reads from the current rows are four times that"""
        n = C.c_int64()
        lib.check(lib.load().ldsim_chain_pixel_truth_row_samples(self.ctx, C.byref(n)))
        return int(n.value)

    def pixel_waveforms(self, min_abs_current=0.0, pad_ticks=0, hits_only=False, dense=False, rows=None):
        """Pixel current waveforms of the last run() (``pixel_waveforms``, ``ldsim_chain_pixel_waveforms``): the summed induced
        current ``S[t]`` of every unique pixel, zero-suppressed on the device.  A tick is active when ``|S[t]| >
        min_abs_current`` (strict, f64), kept when an active tick lies within ``pad_ticks`` (0..64) of it; the spans are the
        runs of kept ticks.  ``hits_only``: only pixels that hold a hit.  Returns ``dict(spans=, samples=, n_ticks=)``:
        structured rows (``pixel_waveforms.SPAN_ROW``: row, pixel_id, batch, t_begin, n_samples, sample_begin) ordered by
        (row, t_begin), and the f32 samples of all spans in that order.  ``dense=True``: ``S`` f32 [len(rows)][N_t] of the
        row range ``rows`` (a ``range`` or ``(begin, end)``; None: every row) instead, zeros included -- the test and debugging
        form.  ``S`` never holds FEE noise.  Raises ``LdsimError`` (LDSIM_ESTATE) under the rules of ``pixel_truth``."""
        from . import pixel_waveforms as pw
        self._check_constants()
        L = lib.load()
        if dense:
            U = int(self.stats.n_unique)
            if rows is None:
                b, e = 0, U
            elif isinstance(rows, range):
                if rows.step != 1:
                    raise ValueError("pixel_waveforms: rows must be a contiguous range")
                b, e = rows.start, max(rows.stop, rows.start)
            else:
                b, e = rows
            n_t = len(consts.detector.TIME_TICKS)                    # (N_t of the constants _check_constants holds the ctx to)
            S = np.zeros((max(int(e) - int(b), 0), n_t), dtype=np.float32)
            lib.check(L.ldsim_chain_pixel_waveforms_dense(self.ctx, C.c_int64(int(b)), C.c_int64(int(e)), lib.ptr(S)))
            return S
        if rows is not None:
            raise ValueError("pixel_waveforms: rows selects the rows of dense=True")
        sizes = (C.c_int64 * 3)()
        lib.check(L.ldsim_chain_pixel_waveforms(self.ctx, C.c_double(float(min_abs_current)), C.c_int32(int(pad_ticks)),
                                                C.c_int32(1 if hits_only else 0), sizes))
        out = dict(spans=np.zeros(int(sizes[0]), dtype=pw.SPAN_ROW), samples=np.zeros(int(sizes[1]), dtype=np.float32),
                   n_ticks=int(sizes[2]))
        lib.check(L.ldsim_chain_pixel_waveforms_download(self.ctx, lib.ptr(out["spans"]), lib.ptr(out["samples"])))
        return out

    def pixel_waveforms_ms(self):
        """HIP-event times (count kernel, fill kernel) of the last ``pixel_waveforms`` pass in ms (timing tools)"""
        a, b = C.c_double(), C.c_double()
        lib.check(lib.load().ldsim_chain_pixel_waveforms_ms(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def fee_universes(self, variations, dense=False):
        """FEE universes of the last run() (``fee_universes``, ``ldsim_chain_fee_universes``): the launch digitised again under
        each of ``variations`` (1 to 64 dicts of ``fee_universes.variation``: absolute values of threshold, gain, pedestal /
        V_ref / V_cm, rise time, hold / busy / reset timing, the three noise charges, the pixel tables' scales and offset), from
        the currents the launch left in HBM.  Returns one dict per universe: ``hit_rows`` (``comm.HIT_ROW``: batch, pixel, adc,
        slot, tick -- the rows of ``download_compact()``), ``hit_charge`` and ``n_hits``; with ``dense=True`` also ``adc_list``,
        ``adc_ticks_list``, ``adc_digit`` [U][A] and ``hit_count`` [U] in the row order of ``download()``.  Universe k equals,
        bit for bit, a fresh run under ``consts`` patched to variation k.  A universe with a non-zero noise charge needs
        ``seed_keyed`` and ``set_batch_keys``.  Backtracking fractions and ``track_pixel_map`` are not produced per universe.
        Raises ``ValueError`` for variations ``fee_universes.validate`` refuses and ``LdsimError`` (LDSIM_ESTATE) under the rules
        of ``pixel_truth``."""
        from . import fee_universes as fu
        self._check_constants()
        variations = list(variations)
        fu.validate(variations)
        L = lib.load()
        n = len(variations)
        arr = fu.pack(variations)
        n_hits = (C.c_int64 * n)()
        lib.check(L.ldsim_chain_fee_universes(self.ctx, arr, C.c_int32(n), n_hits))
        return self._universe_results(n, n_hits, dense)

    def fee_universes_ms(self):
        """HIP-event time of the last ``fee_universes`` pass's scan kernel in ms (timing tools)"""
        a = C.c_double()
        lib.check(lib.load().ldsim_chain_fee_universes_ms(self.ctx, C.byref(a)))
        return a.value

    def fee_variation_nominal(self):
        """the variation of the constants frozen in the context (``ldsim_fee_variation_nominal``)"""
        from . import fee_universes as fu
        from .abi import LdsimFeeVariation
        v = LdsimFeeVariation()
        lib.check(lib.load().ldsim_fee_variation_nominal(self.ctx, C.byref(v)))
        return fu.unpack(v)

    def universes(self, fee=None, charge=None, dense=False):
        """Universes of the last run() (``charge_universes``, ``ldsim_chain_universes``): universe k is the launch re-weighted
        for the charge variation ``charge[k]`` (dicts of ``charge_universes.variation``: absolute values of the electron
        lifetime, W_ion, the box and Birks parameters, the recombination model) and digitised under the FEE variation
        ``fee[k]`` (``fee_universes.variation``).  ``fee=None``: the nominal front end for every universe; ``charge=None``: the
        call is ``fee_universes(fee)``.  Returns the list ``fee_universes`` returns; with ``charge`` every dict also holds
        ``weights`` (f64 per segment of the launch's range: ``n_k / n_res``, what the replayed quench/drift stores over what
        is resident) and ``n_unweightable`` (segments with no resident charge that the universe gives some).  Needs a plain
        ``quench_drift`` (no charge statistics) since the upload.  Raises ``ValueError`` for variations the two ``validate``
        refuse and ``LdsimError`` (LDSIM_ESTATE) under the rules of ``fee_universes``."""
        from . import charge_universes as cu
        from . import fee_universes as fu
        if charge is None:
            if fee is None:
                raise ValueError("universes: give fee variations, charge variations or both")
            return self.fee_universes(fee, dense=dense)
        self._check_constants()
        charge = list(charge)
        cu.validate(charge)
        n = len(charge)
        c_arr, f_arr = cu.pack(charge), None
        if fee is not None:
            fee = list(fee)
            if len(fee) != n:
                raise ValueError(f"universes: {len(fee)} FEE variations for {n} charge variations")
            fu.validate(fee)
            f_arr = fu.pack(fee)
        L = lib.load()
        n_hits = (C.c_int64 * n)()
        lib.check(L.ldsim_chain_universes(self.ctx, f_arr, c_arr, C.c_int32(n), n_hits))
        out = self._universe_results(n, n_hits, dense)
        for k, u in enumerate(out):
            u["weights"], u["n_unweightable"] = self.universe_weights(k)
        return out

    def _universe_results(self, n, n_hits, dense):
        from .comm import HIT_ROW
        L = lib.load()
        U, A = int(self.stats.n_unique), consts.sim.MAX_ADC_VALUES
        out = []
        for k in range(n):
            u = dict(n_hits=int(n_hits[k]), hit_rows=np.zeros(int(n_hits[k]), dtype=HIT_ROW), hit_charge=np.zeros(int(n_hits[k])))
            lib.check(L.ldsim_chain_fee_universe_hits_download(self.ctx, C.c_int32(k), lib.ptr(u["hit_rows"]),
                                                               lib.ptr(u["hit_charge"])))
            if dense:
                u.update(adc_list=np.zeros((U, A)), adc_ticks_list=np.zeros((U, A)), adc_digit=np.zeros((U, A)),
                         hit_count=np.zeros(U, dtype=np.int32))
                lib.check(L.ldsim_chain_fee_universe_download(self.ctx, C.c_int32(k), C.c_int64(U), lib.ptr(u["adc_list"]),
                                                              lib.ptr(u["adc_ticks_list"]), lib.ptr(u["adc_digit"]),
                                                              lib.ptr(u["hit_count"])))
            out.append(u)
        return out

    def universe_weights(self, k):
        """(weights f64 [segments of the launch's range], n_unweightable) of universe ``k`` of the last ``universes`` pass"""
        n_seg = int(self.stats.n_segments)
        w, nu = np.zeros(n_seg), C.c_int64()
        lib.check(lib.load().ldsim_chain_universe_weights_download(self.ctx, C.c_int32(int(k)), lib.ptr(w), C.c_int64(n_seg),
                                                                   C.byref(nu)))
        return w, int(nu.value)

    def universe_waveforms(self, k, rows=None):
        """``S_k`` f64 [len(rows)][N_t] of universe ``k`` of the last ``universes`` pass, formed by the device code its scan read
        (``ldsim_chain_universe_waveforms_dense``; tests and tools).  ``rows``: ``(begin, end)``, None: every row."""
        U = int(self.stats.n_unique)
        b, e = (0, U) if rows is None else rows
        S = np.zeros((max(int(e) - int(b), 0), len(consts.detector.TIME_TICKS)))
        lib.check(lib.load().ldsim_chain_universe_waveforms_dense(self.ctx, C.c_int32(int(k)), C.c_int64(int(b)), C.c_int64(int(e)),
                                                                  lib.ptr(S)))
        return S

    def universes_weights_ms(self):
        """HIP-event time of the last ``universes`` pass's weights kernel in ms (timing tools)"""
        a = C.c_double()
        lib.check(lib.load().ldsim_chain_universes_weights_ms(self.ctx, C.byref(a)))
        return a.value

    def charge_variation_nominal(self):
        """the charge variation of the constants frozen in the context and the mode of the last ``quench_drift``
        (``ldsim_charge_variation_nominal``)"""
        from . import charge_universes as cu
        from .abi import LdsimChargeVariation
        v = LdsimChargeVariation()
        lib.check(lib.load().ldsim_charge_variation_nominal(self.ctx, C.byref(v)))
        return cu.unpack(v)

    def download_async(self, fractions=None):
        """Start copying the results of the last run() to page-locked host arrays on the library's copy stream and return them
        at once (``ldsim_chain_download_async``): the next ``run()`` overlaps with the transfer.  The arrays hold the rows
        after ``wait_download()``; two sets of host buffers alternate, so the arrays of one call stay valid until the call
        after the next one."""
        U = int(self.stats.n_unique)
        A, M = consts.sim.MAX_ADC_VALUES, consts.sim.MAX_TRACKS_PER_PIXEL
        want_fr = fractions if fractions is not None else self._want_fractions
        slot = self.__dict__["_async_slot"] = 1 - self.__dict__.get("_async_slot", 1)
        tag = f"@{slot}"
        out = dict(unique_pix=self._pinned("unique_pix" + tag, (U,), np.int32), batch=self._pinned("batch" + tag, (U,), np.int32),
                   adc_list=self._pinned("adc_list" + tag, (U, A), np.float64),
                   adc_ticks_list=self._pinned("adc_ticks_list" + tag, (U, A), np.float64),
                   adc_digit=self._pinned("adc_digit" + tag, (U, A), np.float64),
                   track_pixel_map=self._pinned("track_pixel_map" + tag, (U, M), np.int64))
        fr = self._pinned("current_fractions" + tag, (U, A, M), np.float64) if want_fr else None
        if fr is not None:
            out['current_fractions'] = fr
        lib.check(lib.load().ldsim_chain_download_async(self.ctx, C.c_int64(U), lib.ptr(out['unique_pix']),
                                                        lib.ptr(out['batch']), lib.ptr(out['adc_list']),
                                                        lib.ptr(out['adc_ticks_list']), lib.ptr(out['adc_digit']),
                                                        lib.ptr(out['track_pixel_map']), lib.ptr(fr)))
        return out

    def wait_download(self):
        """Block until the transfer started by ``download_async`` has landed."""
        lib.check(lib.load().ldsim_chain_download_wait(self.ctx))

    # ---- device-resident light leg (cli/simulate_pixels.py:749-797, 1120-1153) ------------------------------------------------
    def light_incidence(self, lut=None, n_out=None):
        """``lightLUT.calculate_light_incidence`` over all resident segments (after ``quench_drift``); the arrays stay in
        HBM.  ``lut``: the structured LUT (uploaded unless already resident); ``n_out``: output channels, default all.
        Under the context option ``lib.set_option("light_lut_interp", 1)`` the visibility is interpolated trilinearly between
        voxel centres (``lightLUT.interpolated_light_incidence`` is the numpy twin); the voxel output stays the nearest one."""
        self._check_constants()
        lib.set_light(lut, self.ctx)
        n_out = consts.light.N_OP_CHANNEL if n_out is None else n_out
        lib.check(lib.load().ldsim_dev_light_incidence(self.ctx, C.c_int32(int(n_out))))
        self._light_n_out = int(n_out)

    def download_light_incidence(self, seg_begin=0, seg_end=None):
        """(light_sim_dat rows, track_light_voxel rows) of resident segments [seg_begin, seg_end) in the reference's dtypes
        (cli/simulate_pixels.py:760-763); ``segment_id`` is left 0 -- the driver fills it from its own ids."""
        seg_end = self.n if seg_end is None else seg_end
        n = seg_end - seg_begin
        nph = np.zeros((n, self._light_n_out), dtype=np.float32)
        t0 = np.zeros((n, self._light_n_out), dtype=np.float32) if consts.light.LIGHT_TRIG_MODE == 0 else None
        vox = np.zeros((n, 3), dtype=np.int32)
        lib.check(lib.load().ldsim_dev_light_incidence_download(self.ctx, C.c_int64(seg_begin), C.c_int64(seg_end),
                                                                lib.ptr(nph), lib.ptr(t0), lib.ptr(vox)))
        inc = np.zeros((n, self._light_n_out), dtype=[('segment_id', 'u4'), ('n_photons_det', 'f4'), ('t0_det', 'f4')])
        inc['n_photons_det'] = nph
        if t0 is not None:
            inc['t0_det'] = t0
        return inc, vox

    def light_nticks(self, seg_begin, seg_end):
        """``light_sim.get_nticks`` (larndsim/light_sim.py:24-41) for the resident rows of one batch: same expressions, with
        the min / max of ``t0_det`` reduced on the device."""
        light = consts.light
        if light.LIGHT_TRIG_MODE == 0:
            lo, hi, any_ = C.c_float(), C.c_float(), C.c_int32()
            lib.check(lib.load().ldsim_dev_light_t0_range(self.ctx, C.c_int64(seg_begin), C.c_int64(seg_end), C.byref(lo),
                                                          C.byref(hi), C.byref(any_)))
            if any_.value:
                start_time = np.float32(lo.value) - light.LIGHT_WINDOW[0]
                end_time = np.float32(hi.value) + light.LIGHT_WINDOW[1]
                return int(np.ceil((end_time - start_time) / light.LIGHT_TICK_SIZE)), start_time
        return int((light.LIGHT_WINDOW[1] + light.LIGHT_WINDOW[0]) / light.LIGHT_TICK_SIZE), 0

    def sum_light(self, seg_begin, seg_end, op_channel, segment_track_id=None, max_truth=None, max_ticks=int(5e4)):
        """``light_sim.sum_light_signals`` for the batch [seg_begin, seg_end) on the resident incidence arrays
        (cli/simulate_pixels.py:1120-1153).  Returns (n_ticks, start_time); fetch the arrays with ``download_light``."""
        self._check_constants()
        mt = consts.sim.MAX_MC_TRUTH_IDS if max_truth is None else max_truth
        if not mt and consts.light.LIGHT_TRIG_MODE != 0:
            # The driver's loop over hundreds of small batches without truth slots (ndlar): the library call returns with its two
            # kernels in flight, so what the loop costs is this wrapper -- the channel array's pointer and the call's fixed
            # arguments are kept from the last call with the same array object (7.5 -> 2.5 us per call)
            fast = self.__dict__.get("_sum_light_fast")
            lw = consts.light.LIGHT_WINDOW
            key = (max_ticks, lw[0], lw[1], consts.light.LIGHT_TICK_SIZE)
            if fast is None or fast[0] is not op_channel or fast[1] != key:
                n_ticks, t_start = self.light_nticks(seg_begin, seg_end)       # (trigger mode 1: the same for every batch)
                n_ticks = min(n_ticks, max_ticks)
                opc = np.ascontiguousarray(op_channel, dtype=np.int32)
                f = lib.load().ldsim_dev_sum_light
                fast = (op_channel, key, opc, f, lib.ptr(opc), C.c_int32(opc.shape[0]), C.c_int32(0),
                        C.c_double(float(t_start)), C.c_int32(int(n_ticks)), int(n_ticks), t_start,
                        (opc.shape[0], int(n_ticks), 0))
                if opc is op_channel:          # (a converted copy would not follow in-place changes of the caller's array)
                    self._sum_light_fast = fast
            rc = fast[3](self.ctx, C.c_int64(seg_begin), C.c_int64(seg_end), fast[4], fast[5], None, fast[6], fast[7], fast[8])
            if rc:
                lib.check(rc)
            self._light_shape = fast[11]
            lib.set_light_shape_tuple(fast[11])
            return fast[9], fast[10]
        n_ticks, t_start = self.light_nticks(seg_begin, seg_end)
        n_ticks = min(n_ticks, max_ticks)
        opc = np.ascontiguousarray(op_channel, dtype=np.int32)
        tid = None
        if mt:
            tid = (np.arange(seg_begin, seg_end, dtype=np.int64) if segment_track_id is None
                   else np.ascontiguousarray(segment_track_id, dtype=np.int64))
            if tid.shape[0] != seg_end - seg_begin:
                raise ValueError("segment_track_id must have one entry per segment of the range")
        lib.check(lib.load().ldsim_dev_sum_light(self.ctx, C.c_int64(seg_begin), C.c_int64(seg_end), lib.ptr(opc),
                                                 C.c_int32(opc.shape[0]), lib.ptr(tid), C.c_int32(int(mt)),
                                                 C.c_double(float(t_start)), C.c_int32(int(n_ticks))))
        self._light_shape = (opc.shape[0], int(n_ticks), int(mt))
        lib.set_light_shape(self._light_shape)
        return n_ticks, t_start

    def light_response(self, fluctuate=True):
        """``calc_scintillation_effect`` -> ``calc_stat_fluctuations`` (if ``fluctuate``; needs ``seed_rng``) ->
        ``calc_light_detector_response`` on the photon sum of the last ``sum_light``, in HBM
        (cli/simulate_pixels.py:1159-1180).  ``light_sim.get_triggers(None, ...)`` / ``light_sim.sim_triggers(.., None, ..)``
        then work on the resident result; ``download_light_response`` fetches it."""
        self._check_constants()
        light = consts.light
        nd = self._light_shape[0]
        gain = np.ascontiguousarray(light.LIGHT_GAIN, dtype=np.float64)
        if gain.shape[0] < nd:
            raise IndexError(f"LIGHT_GAIN has {gain.shape[0]} entries, the photon sum has {nd} rows")
        imp = np.ascontiguousarray(light.IMPULSE_MODEL, dtype=np.float64)
        lib.check(lib.load().ldsim_dev_light_response(self.ctx, lib.ptr(gain), lib.ptr(imp), C.c_int32(imp.shape[0]),
                                                      C.c_int32(int(bool(fluctuate)))))

    def download_light_response(self, stages=False, truth=True):
        """response f4 [n_det][n_ticks] (+ true ids i8, true photons f8); with ``stages`` also the scintillation and the
        fluctuated arrays: (scint, disc, response, ids, photons)."""
        nd, nt, mt = self._light_shape
        resp = np.zeros((nd, nt), dtype=np.float32)
        sc = np.zeros((nd, nt), dtype=np.float32) if stages else None
        di = np.zeros((nd, nt), dtype=np.float32) if stages else None
        tid = np.full((nd, nt, mt if truth else 0), -1, dtype=np.int64)
        tph = np.zeros((nd, nt, mt if truth else 0))
        lib.check(lib.load().ldsim_dev_light_response_download(
            self.ctx, lib.ptr(sc), lib.ptr(di), lib.ptr(resp), lib.ptr(tid) if (mt and truth) else None,
            lib.ptr(tph) if (mt and truth) else None))
        return (sc, di, resp, tid, tph) if stages else (resp, tid, tph)

    def light_response_ms(self):
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        lib.check(lib.load().ldsim_light_response_ms(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return {"scintillation": a.value, "fluctuations": b.value, "detector_response": c.value}

    # ---- light universes (light_universes.py, ldsim_dev_light_universes) ---------------------------------------------------------
    def light_variation_nominal(self):
        """the light variation of the constants frozen in the context (``ldsim_light_variation_nominal``)"""
        from . import light_universes as lu
        from .abi import LdsimLightVariation
        v = LdsimLightVariation()
        lib.check(lib.load().ldsim_light_variation_nominal(self.ctx, C.byref(v)))
        return lu.unpack(v)

    def light_universes(self, variations, fluctuate=True, keep_stages=False):
        """Light universes of the last ``sum_light`` (``light_universes``, ``ldsim_dev_light_universes``): the batch's
        scintillation profile, Poisson fluctuations (if ``fluctuate``; needs ``seed_keyed`` and the call key of ``set_rng_key``)
        and detector response run again under each of ``variations`` (1 to 64 dicts of ``light_universes.variation``), in HBM.
        Universes with equal constants share their stages; tables that share an input go through one multi-table kernel.
        ``light_sim.get_triggers_universe`` / ``sim_triggers_universe`` then work on universe ``k``'s response and
        ``download_light_universe`` fetches it (its scintillation and fluctuated arrays only with ``keep_stages``).  The
        launch's own ``light_response`` result is left as it was.  Every array of universe k equals, bit for bit, a
        ``light_response`` on the scaled photon sum under ``consts.light`` patched to variation k and the same call key.
        ``trig_threshold_scale`` and ``noise_scale`` are not used here: they scale arguments of the two ``light_sim`` calls.
        Raises ``ValueError`` for variations ``light_universes.validate`` refuses and ``LdsimError`` (LDSIM_ESTATE) without a
        resident photon sum, or with ``fluctuate`` in table mode."""
        from . import light_universes as lu
        self._check_constants()
        variations = list(variations)
        lu.validate(variations)
        light = consts.light
        nd = self._light_shape[0]
        gain = np.ascontiguousarray(light.LIGHT_GAIN, dtype=np.float64)
        if gain.shape[0] < nd:
            raise IndexError(f"LIGHT_GAIN has {gain.shape[0]} entries, the photon sum has {nd} rows")
        imp = np.ascontiguousarray(light.IMPULSE_MODEL, dtype=np.float64)
        arr = lu.pack(variations)
        lib.check(lib.load().ldsim_dev_light_universes(self.ctx, arr, C.c_int32(len(variations)), lib.ptr(gain), lib.ptr(imp),
                                                       C.c_int32(imp.shape[0]), C.c_int32(int(bool(fluctuate))),
                                                       C.c_int32(int(bool(keep_stages)))))
        self._light_universes_shape = self._light_shape[:2]

    def download_light_universe(self, k, stages=False):
        """response f4 [n_det][n_ticks] of universe ``k`` of the last ``light_universes``; with ``stages`` (kept by
        ``keep_stages=True``): (scint, disc, response), disc being scint when the pass ran without fluctuations"""
        nd, nt = self.__dict__.get("_light_universes_shape", self._light_shape[:2])
        resp = np.zeros((nd, nt), dtype=np.float32)
        sc = np.zeros((nd, nt), dtype=np.float32) if stages else None
        di = np.zeros((nd, nt), dtype=np.float32) if stages else None
        lib.check(lib.load().ldsim_dev_light_universe_download(self.ctx, C.c_int32(int(k)), lib.ptr(sc), lib.ptr(di),
                                                               lib.ptr(resp)))
        return (sc, di, resp) if stages else resp

    def light_universes_ms(self):
        """HIP-event times of the three stages summed over the last ``light_universes`` pass in ms (timing tools)"""
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        lib.check(lib.load().ldsim_light_universes_ms(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return {"scintillation": a.value, "fluctuations": b.value, "detector_response": c.value}

    def download_light(self, truth=True):
        """(light_sample_inc f4 [n_det][n_ticks], true_track_id i8 [..][max_truth], true_photons f8 [..][max_truth])."""
        nd, nt, mt = self._light_shape
        out = np.zeros((nd, nt), dtype=np.float32)
        want = bool(mt and truth)          # (the truth arrays are GBs at 50 slots: only made when asked for)
        tid = np.full((nd, nt, mt if want else 0), -1, dtype=np.int64)
        tph = np.zeros((nd, nt, mt if want else 0))
        lib.check(lib.load().ldsim_dev_light_download(self.ctx, lib.ptr(out), lib.ptr(tid) if want else None,
                                                      lib.ptr(tph) if want else None))
        return out, tid, tph

    def light_kernel_ms(self):
        a, b = C.c_double(), C.c_double()
        lib.check(lib.load().ldsim_light_kernel_ms(self.ctx, C.byref(a), C.byref(b)))
        return dict(incidence_ms=a.value, sum_ms=b.value)

    def compact_hits(self):
        """(device pointer, n_rows, row_bytes) of the compact hit list of the last run()."""
        p, n, rb = C.c_void_p(), C.c_int64(), C.c_int32()
        lib.check(lib.load().ldsim_chain_compact_hits(self.ctx, C.byref(p), C.byref(n), C.byref(rb)))
        return p.value, n.value, rb.value


def expand_compact(c, lead_rows=False):
    """Dense rows of the hit pixels from ``ChargeChain.download_compact()``: the arrays ``download()`` returns, restricted to
    the unique pixels that hold a hit (``row`` = their index in the full arrays): ``unique_pix``, ``batch``, ``adc_list``,
    ``first_of_batch`` (the pixel is row 0 of its batch in the full arrays: the exporter's clock-rollover bookkeeping looks at the
    first row it is handed), ``adc_ticks_list``, ``adc_digit`` [n][A] (slots past a pixel's last hit: charge 0, tick 0, the pedestal code -- what the dense
    arrays hold there), ``track_pixel_map`` [n][M] (-1 pad) and ``current_fractions`` [n][A][M] (written slots only: the dense
    array's un-normalised residue in the slot after the last hit, fee.py:572-573, is not part of the result).

    ``lead_rows``: a batch whose first unique pixel holds no hit keeps that hit-less row in front of its hit pixels (no charge, no
    track) -- the reference's exporter keeps its clock-rollover state in row 0 of what it is handed (fee.py:164-183, 267-277), and
    the driver counts the batches of an export from what it is handed, so a batch without any hit still shows up as its first row.
    The compact form carries the first row of every batch (0 hits) since round 4; for input without it the row is inserted here
    (the pixel id of the row after it, ``row`` -1)."""
    from . import packets
    A, M = consts.sim.MAX_ADC_VALUES, consts.sim.MAX_TRACKS_PER_PIXEL
    hp = c["hit_pixels"]
    if not lead_rows and len(hp) and (hp[:, 3] == 0).any():          # (hit-less first rows carry no hits, slots or fractions)
        hp = hp[hp[:, 3] > 0]
    n0 = hp.shape[0]
    nh, nt = hp[:, 3].astype(np.int64), (hp[:, 4] & 255).astype(np.int64)
    first = (hp[:, 4] & 256) != 0
    ped = float(packets._digitize0())                   # fee.digitize(0): what an unwritten slot digitises to
    pos = np.arange(n0)                                 # output row of hit pixel i
    n = n0
    if lead_rows and n0:
        need = np.r_[True, hp[1:, 2] != hp[:-1, 2]] & ~first          # batches that start with a hit-less pixel
        pos = pos + np.cumsum(need)
        n = n0 + int(need.sum())
    out = dict(row=np.full(n, -1, dtype=hp.dtype), first_of_batch=np.ones(n, dtype=bool), unique_pix=np.zeros(n, dtype=hp.dtype),
               batch=np.zeros(n, dtype=hp.dtype), adc_list=np.zeros((n, A)),
               adc_ticks_list=np.zeros((n, A)), adc_digit=np.full((n, A), ped), track_pixel_map=np.full((n, M), -1, dtype=np.int64))
    out["row"][pos] = hp[:, 0]
    out["first_of_batch"][pos] = first
    out["unique_pix"][pos] = hp[:, 1]
    out["batch"][pos] = hp[:, 2]
    if n != n0:
        lead = pos[need] - 1
        out["unique_pix"][lead] = hp[need, 1]
        out["batch"][lead] = hp[need, 2]
    # hits: pixel after pixel, slot 0 up
    pix_of_hit = np.repeat(pos, nh)
    slot = c["hit_rows"]["slot"].astype(np.int64)
    out["adc_list"][pix_of_hit, slot] = c["hit_charge"]
    out["adc_ticks_list"][pix_of_hit, slot] = c["hit_rows"]["tick"]
    out["adc_digit"][pix_of_hit, slot] = c["hit_rows"]["adc"]
    # track slots: pixel after pixel
    pix_of_trk = np.repeat(pos, nt)
    m_of_trk = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
    out["track_pixel_map"][pix_of_trk, m_of_trk] = c["track_segments"]
    if c.get("has_fractions"):
        fr = np.zeros((n, A, M))
        per_hit = np.repeat(nt, nh)                                 # fraction entries of every hit
        h_of_f = np.repeat(np.arange(len(pix_of_hit)), per_hit)
        m_of_f = np.arange(int(per_hit.sum())) - np.repeat(np.cumsum(per_hit) - per_hit, per_hit)
        fr[pix_of_hit[h_of_f], slot[h_of_f], m_of_f] = c["fractions"]
        out["current_fractions"] = fr
    return out
