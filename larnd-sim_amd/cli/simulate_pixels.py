#!/usr/bin/env python3
"""
simulate_pixels.py -- command-line driver keeping the reference's flag surface (cli/simulate_pixels.py:124-145, run through
`fire` there; argparse here).

input checks -> configuration resolution (larndsim_amd.config, the reference's get_config rules) -> segment preparation
(segment_id / n_photons / t0 columns, spill-time reset, x<->z swap) -> active-volume selection -> batching ->
quench + drift -> [light incidence; per batch: photon sum -> scintillation profile -> Poisson fluctuations -> SiPM response ->
triggers -> digitised waveforms with detector noise] -> charge chain with FEE noise -> LArPix packets + mc_packets_assn per
batch -> output file (HDF5 when h5py is importable, else .npz with the same dataset names) with the updated segments,
light_dat, light_trig, light_wvfm, light_wvfm_mc_assn and the truth datasets of the input passed through.

Module-to-module variation (--mod2mod_variation or a keyword with MOD2MOD_VARIATION, e.g. `2x2`): the driver's module loop --
per-module constants, pixel layout, response, light LUT, thresholds and gains; per-module light datasets merged at the end.

The per-module pointer lists (--pixel_layout_id, --response_id, --light_lut_id, --pixel_thresholds_id, --pixel_gains_id: module m
uses file ids[m] of the corresponding file list) default to the keyword's <X>_ID entries.

Several GPUs (--n_gpus N): whole events sharded over N processes, one per GPU; rank 0 gathers the others' results and writes
the one output file ("Multi-GPU driver").

Not built (the flag is accepted and reported): memory logging (--save_memory).
"""
import argparse
import os
import pickle
from math import ceil
import sys
import warnings
from time import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from larndsim_amd import launch  # noqa: E402  (standard library only)

IGNORED = ("save_memory",)
ID_FLAGS = ("pixel_layout_id", "response_id", "light_lut_id", "pixel_thresholds_id", "pixel_gains_id")


def _parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input_filename", required=True)
    ap.add_argument("--output_filename", required=True)
    ap.add_argument("--config", default="module0")
    ap.add_argument("--config_root", default=None, help="larnd-sim tree holding config/config.yaml and the YAML families "
                                                        "(default: $LARNDSIM_ROOT, else the built-in snapshot keywords)")
    tf = lambda s: s.lower() in ("1", "true", "yes")                # noqa: E731
    ap.add_argument("--mod2mod_variation", type=tf, default=None,
                    help="per-module pixel layouts / responses / light LUTs / thresholds / gains (comma-separated lists), "
                         "default: the keyword's MOD2MOD_VARIATION")
    ap.add_argument("--light_simulated", type=tf, default=None)
    for k in ("pixel_layout", "detector_properties", "simulation_properties", "response_file", "light_lut_filename",
              "light_det_noise_filename", "bad_channels", "pixel_thresholds_file", "pixel_gains_file", *IGNORED):
        ap.add_argument("--" + k, default=None)
    for k in ID_FLAGS:
        ap.add_argument("--" + k, default=None, help="module variation: per-module index into the corresponding file list, "
                                                      "e.g. 0,0,1,0 (default: the keyword's entry)")
    ap.add_argument("--n_events", type=int, default=None)
    ap.add_argument("--rand_seed", type=int, default=None)
    ap.add_argument("--tracks_current_mc", action="store_true",
                    help="induced currents from tracks_current_mc like the reference driver (default: tracks_current)")
    ap.add_argument("--raw_arrays", action="store_true", help="also store the per-pixel arrays (raw/...) and light_sample_inc")
    ap.add_argument("--numba_f32", default="auto", choices=["auto", "0", "1"],
                    help="evaluate the sub-expressions Numba types as float32 for f4 record fields in single precision like the "
                         "reference (1), all in double (0), or by the input records' dtype (auto, default); unpinned restatement")
    ap.add_argument("--n_gpus", type=int, default=None,
                    help="shard the events over N GPUs, one process each (started here, or by a launcher that sets WORLD_SIZE=N); "
                         "rank 0 writes the one output file.  Deterministic stages give the one-GPU result at any N.  With --rng "
                         "table the random stages (FEE noise, light fluctuations and noise) depend on N: rank r seeds its table with "
                         "rand_seed + r, and the reference's history-dependent RNG chain is not replayed across ranks; with --rng "
                         "keyed they do not depend on N")
    ap.add_argument("--force_dist", action="store_true", help="with --n_gpus 1: run the multi-GPU (RCCL) path with one rank")
    ap.add_argument("--rng", default="table", choices=["table", "keyed"],
                    help="random streams: table (default; the restated numba xoroshiro128p table, advanced in place) or keyed "
                         "(every draw a function of the seed and the identity of what is simulated: the same file at any "
                         "--n_gpus, --chunk_segments or event subset)")
    ap.add_argument("--field_map", default=None,
                    help="drift-field maps (.npz, larndsim_amd/field_map.py): per TPC the local field of the recombination and "
                         "the displacement / drift-time shift of the charge on its way to the anode (default: uniform field)")
    ap.add_argument("--charge_statistics", action="store_true",
                    help="count the charge: Fano-smeared ion pairs, binomial recombination and electron attachment drawn from "
                         "keyed streams (larndsim_amd/charge_stats.py) instead of mean values; needs --rng keyed")
    ap.add_argument("--fano_factor", type=float, default=None,
                    help="Fano factor of the ion-pair count under --charge_statistics (default 0.107)")
    ap.add_argument("--sipm_crosstalk", type=float, default=None,
                    help="SiPM correlated noise in the light fluctuations (larndsim_amd/sipm_noise.py; any --sipm_* flag enables "
                         "it; needs --rng keyed): mean number of prompt cross-talk avalanches per avalanche, 0 .. 0.5 (default 0)")
    ap.add_argument("--sipm_afterpulse", type=float, default=None,
                    help="SiPM noise: probability of one after-pulse per avalanche, 0 .. 0.5 (default 0)")
    ap.add_argument("--sipm_afterpulse_tau", type=float, default=None,
                    help="SiPM noise: mean delay of an after-pulse [us] (default 0.1)")
    ap.add_argument("--sipm_dark_rate", type=float, default=None,
                    help="SiPM noise: dark counts per us and light detector inside a simulated sub-batch's window (default 0)")
    ap.add_argument("--pixel_truth", action="store_true",
                    help="also store the true induced charge per pixel and per (pixel, segment) of every chain launch "
                         "(datasets pixel_truth and pixel_truth_tracks, larndsim_amd/pixel_truth.py); one GPU only")
    ap.add_argument("--pixel_truth_min_charge", type=float, default=None,
                    help="under --pixel_truth: pixels without a hit are stored when they saw at least this much |charge| "
                         "[electrons] (default 0: every pixel a segment reached)")
    ap.add_argument("--pixel_waveforms", action="store_true",
                    help="also store the summed induced current of every pixel of every chain launch, zero-suppressed into "
                         "spans (datasets pixel_waveforms and pixel_waveform_samples, larndsim_amd/pixel_waveforms.py); one "
                         "GPU only")
    ap.add_argument("--pixel_waveforms_threshold", type=float, default=None,
                    help="under --pixel_waveforms: a tick is active when |current| exceeds this (default 0: every non-zero tick)")
    ap.add_argument("--pixel_waveforms_pad", type=int, default=None,
                    help="under --pixel_waveforms: ticks kept on either side of an active tick, 0..64 (default 0)")
    ap.add_argument("--pixel_waveforms_hits_only", action="store_true",
                    help="under --pixel_waveforms: only the pixels that hold a hit")
    ap.add_argument("--fee_universes", default=None, metavar="FILE.json",
                    help="also digitise every chain launch again under each universe of FILE.json, a list of {\"name\": ..., "
                         "\"DISCRIMINATION_THRESHOLD\": ..., ...}: front-end constants by their names in the detector properties "
                         "(threshold, gain, V_CM / V_REF / V_PEDESTAL, BUFFER_RISETIME, ADC_HOLD_DELAY / ADC_BUSY_DELAY / "
                         "RESET_CYCLES, the three noise charges, THRESHOLD_TABLE_SCALE / _OFFSET and GAIN_TABLE_SCALE for the pixel "
                         "tables), the others as configured (datasets fee_universes and fee_universe_hits, "
                         "larndsim_amd/fee_universes.py); hits only: LArPix packets per universe are out of scope; universes with "
                         "noise need --rng keyed; one GPU only")
    ap.add_argument("--charge_universes", default=None, metavar="FILE.json",
                    help="also re-weight every chain launch for each universe of FILE.json, a list of {\"name\": ..., "
                         "\"ELECTRON_LIFETIME\": ..., ...}: charge constants (ELECTRON_LIFETIME, W_ION, BOX_ALPHA, BOX_BETA, BIRKS_AB, "
                         "BIRKS_KB, RECOMB_MODEL \"box\" or \"birks\") and any key of --fee_universes, so one file holds combined "
                         "universes; the others as configured (datasets charge_universes and charge_universe_hits, "
                         "larndsim_amd/charge_universes.py); hits only; a separate pass beside --fee_universes; not with "
                         "--charge_statistics or --tracks_current_mc; universes with noise need --rng keyed; one GPU only")
    ap.add_argument("--light_universes", default=None, metavar="FILE.json",
                    help="also run the light response of every sub-batch again under each universe of FILE.json, a list of "
                         "{\"name\": ..., \"TAU_S\": ..., ...}: light constants by their names (SINGLET_FRACTION, TAU_S, TAU_T, "
                         "LIGHT_RESPONSE_TIME, LIGHT_OSCILLATION_PERIOD) and PHOTON_SCALE, LIGHT_GAIN_SCALE, TRIG_THRESHOLD_SCALE, "
                         "NOISE_SCALE, the others as configured (datasets light_universes, light_universe_trig and "
                         "light_universe_wvfm, larndsim_amd/light_universes.py); all universes of a batch see the same random "
                         "numbers; no truth slots per universe; needs --rng keyed and simulated light; not with module variation; "
                         "one GPU only")
    ap.add_argument("--light_lut_interpolation", default="nearest", choices=list(LIGHT_LUT_INTERPOLATION),
                    help="visibility of a segment from the light LUT: nearest (default; the voxel that holds the segment, like "
                         "the reference) or trilinear (interpolated between the eight voxel centres around it: no step in the "
                         "light yield at voxel faces; the time profile still comes from the nearest voxel)")
    ap.add_argument("--chunk_segments", type=int, default=50000,
                    help="segments per chain launch (whole batches, at least this many; default 50000)")
    return ap


LIGHT_LUT_INTERPOLATION = {"nearest": 0, "trilinear": 1}          # --light_lut_interpolation -> context option light_lut_interp

FEE_UNIVERSES_NEED_KEYED = ("--fee_universes: universe {} has a non-zero noise charge, and its normals come from the keyed "
                            "streams of the launch's pixels: give --rng keyed as well")

CHARGE_UNIVERSES_NEED_KEYED = ("--charge_universes: universe {} has a non-zero noise charge, and its normals come from the keyed "
                               "streams of the launch's pixels: give --rng keyed as well")
CHARGE_UNIVERSES_NO_STATISTICS = ("--charge_universes is not available with --charge_statistics: binomial draws are not linear in "
                                  "the constants, the launch cannot be re-weighted")
CHARGE_UNIVERSES_NO_MC = ("--charge_universes is not available with --tracks_current_mc: its currents are sampled, not the rows "
                          "that are re-weighted")

LIGHT_UNIVERSES_NEED_KEYED = ("--light_universes draws every universe's fluctuations and noise from the keyed streams of the "
                              "batch, so that all universes see the same random numbers: give --rng keyed as well")
LIGHT_UNIVERSES_NO_MULTI_GPU = "--light_universes is not available with --n_gpus > 1 (its rows are not gathered over the ranks)"
LIGHT_UNIVERSES_NO_MODVAR = ("--light_universes is not available with module variation (a run with it writes per-module waveform "
                             "datasets and merges them)")
LIGHT_UNIVERSES_NEED_LIGHT = "--light_universes varies the light simulation, and light is not simulated in this run"

CHARGE_STATISTICS_NEEDS_KEYED = ("--charge_statistics draws from keyed random streams (one per segment, whatever the "
                                 "chunking or rank count): give --rng keyed as well")
SIPM_NOISE_NEEDS_KEYED = ("--sipm_crosstalk, --sipm_afterpulse, --sipm_afterpulse_tau and --sipm_dark_rate draw from keyed random "
                          "streams (one per light detector and tick, whatever the chunking or rank count): give --rng keyed as "
                          "well")


def sipm_noise_of(crosstalk, afterpulse, afterpulse_tau, dark_rate):
    """the four constants of the SiPM noise from the --sipm_* options (None where one is absent: its default), or None when
    none is given (the feature stays off); ValueError names a flag out of range"""
    if crosstalk is None and afterpulse is None and afterpulse_tau is None and dark_rate is None:
        return None
    # (standard library only: the parent of --n_gpus N parses the options too.  The ranges are ldsim_set_sipm_noise's; the bound
    # of the dark rate that depends on LIGHT_TICK_SIZE is left to it)
    p = dict(crosstalk=float(crosstalk or 0.0), afterpulse=float(afterpulse or 0.0),
             afterpulse_tau=0.1 if afterpulse_tau is None else float(afterpulse_tau), dark_rate=float(dark_rate or 0.0))
    for name in ("crosstalk", "afterpulse"):
        if not 0 <= p[name] <= 0.5:
            raise ValueError(f"--sipm_{name} {p[name]:g} must lie in [0, 0.5]")
    if p["afterpulse"] > 0 and not 0 < p["afterpulse_tau"] < float("inf"):
        raise ValueError(f"--sipm_afterpulse_tau {p['afterpulse_tau']:g} us must be finite and > 0 when --sipm_afterpulse > 0")
    if not 0 <= p["dark_rate"] < float("inf"):
        raise ValueError(f"--sipm_dark_rate {p['dark_rate']:g} per us must be finite and >= 0")
    return p


def _parse_args(argv=None):
    """the parsed options, after the checks that need more than one of them"""
    ap = _parser()
    a = ap.parse_args(argv)
    if a.fano_factor is not None and not a.charge_statistics:
        ap.error("--fano_factor sets the Fano factor of --charge_statistics: give --charge_statistics as well")
    if a.charge_statistics and a.rng != "keyed":
        ap.error(CHARGE_STATISTICS_NEEDS_KEYED)
    if a.fano_factor is not None and not (0 <= a.fano_factor < float("inf")):
        ap.error("--fano_factor must be finite and >= 0")
    try:
        sipm = sipm_noise_of(a.sipm_crosstalk, a.sipm_afterpulse, a.sipm_afterpulse_tau, a.sipm_dark_rate)
    except ValueError as e:
        ap.error(str(e))
    if sipm is not None and a.rng != "keyed":
        ap.error(SIPM_NOISE_NEEDS_KEYED)
    if a.pixel_truth_min_charge is not None and not a.pixel_truth:
        ap.error("--pixel_truth_min_charge sets the selection of --pixel_truth: give --pixel_truth as well")
    if a.pixel_truth_min_charge is not None and not (0 <= a.pixel_truth_min_charge < float("inf")):
        ap.error("--pixel_truth_min_charge must be finite and >= 0")
    for flag, given in (("--pixel_waveforms_threshold", a.pixel_waveforms_threshold is not None),
                        ("--pixel_waveforms_pad", a.pixel_waveforms_pad is not None),
                        ("--pixel_waveforms_hits_only", a.pixel_waveforms_hits_only)):
        if given and not a.pixel_waveforms:
            ap.error(f"{flag} sets the selection of --pixel_waveforms: give --pixel_waveforms as well")
    if a.pixel_waveforms_threshold is not None and not (0 <= a.pixel_waveforms_threshold < float("inf")):
        ap.error("--pixel_waveforms_threshold must be finite and >= 0")
    if a.pixel_waveforms_pad is not None and not (0 <= a.pixel_waveforms_pad <= 64):
        ap.error("--pixel_waveforms_pad must lie in [0, 64]")
    if a.fee_universes is not None:
        # (what the file alone decides; a universe that inherits the configuration's noise charges is checked once they are loaded)
        from larndsim_amd import fee_universes as lfu  # (standard library only)
        try:
            entries = lfu.read(a.fee_universes)
        except (OSError, ValueError) as e:
            ap.error(f"--fee_universes {a.fee_universes}: {e}")
        for k, (name, changes) in enumerate(entries):
            if lfu.changes_noisy(changes) and a.rng != "keyed":
                ap.error(FEE_UNIVERSES_NEED_KEYED.format(f"{k} ({name})"))
    if a.charge_universes is not None:
        from larndsim_amd import charge_universes as lcu  # (standard library only)
        from larndsim_amd import fee_universes as lfu
        if a.charge_statistics:
            ap.error(CHARGE_UNIVERSES_NO_STATISTICS)
        if a.tracks_current_mc:
            ap.error(CHARGE_UNIVERSES_NO_MC)
        try:
            entries = lcu.read(a.charge_universes)
        except (OSError, ValueError) as e:
            ap.error(f"--charge_universes {a.charge_universes}: {e}")
        for k, (name, _, fee_changes) in enumerate(entries):
            if lfu.changes_noisy(fee_changes) and a.rng != "keyed":
                ap.error(CHARGE_UNIVERSES_NEED_KEYED.format(f"{k} ({name})"))
    if a.light_universes is not None:
        from larndsim_amd import light_universes as llu  # (standard library only)
        if a.rng != "keyed":
            ap.error(LIGHT_UNIVERSES_NEED_KEYED)
        if a.mod2mod_variation:
            ap.error(LIGHT_UNIVERSES_NO_MODVAR)
        if a.light_simulated is False:
            ap.error(LIGHT_UNIVERSES_NEED_LIGHT)
        try:
            llu.read(a.light_universes)
        except (OSError, ValueError) as e:
            ap.error(f"--light_universes {a.light_universes}: {e}")
    return a


def launch_ranks_if_asked(argv=None):
    """--n_gpus N (or --n_gpus 1 --force_dist) without a launcher: N fresh child processes, one rank each, and exit with the
    worst child's code.  Runs before the simulation modules are imported: this parent loads neither numpy nor the HIP
    library, touches no GPU and is never replaced by exec.  Returns (without doing anything) in every other case."""
    a = vars(_parse_args(argv))
    try:
        _, world = launch.dist_mode(a["n_gpus"], a["force_dist"])  # (refuses a WORLD_SIZE that contradicts --n_gpus)
    except ValueError as e:
        raise SystemExit(f"simulate_pixels.py: {e}")
    if world is not None and world > 1 and a["raw_arrays"]:
        raise SystemExit("simulate_pixels.py: --raw_arrays is not available with --n_gpus > 1 (the compact path is the "
                         "production one)")
    if world is not None and world > 1 and a["pixel_truth"]:
        raise SystemExit("simulate_pixels.py: --pixel_truth is not available with --n_gpus > 1 (its rows are not gathered "
                         "over the ranks)")
    if world is not None and world > 1 and a["pixel_waveforms"]:
        raise SystemExit("simulate_pixels.py: --pixel_waveforms is not available with --n_gpus > 1 (its rows are not gathered "
                         "over the ranks)")
    if world is not None and world > 1 and a["fee_universes"]:
        raise SystemExit("simulate_pixels.py: --fee_universes is not available with --n_gpus > 1 (its rows are not gathered "
                         "over the ranks)")
    if world is not None and world > 1 and a["charge_universes"]:
        raise SystemExit("simulate_pixels.py: --charge_universes is not available with --n_gpus > 1 (its rows are not gathered "
                         "over the ranks)")
    if world is not None and world > 1 and a["light_universes"]:
        raise SystemExit(f"simulate_pixels.py: {LIGHT_UNIVERSES_NO_MULTI_GPU}")
    if world is None or "WORLD_SIZE" in os.environ:
        return
    if os.path.exists(a["output_filename"]):
        raise SystemExit(f"Output file {a['output_filename']} already exists.")
    code, bad = launch.launch_ranks([sys.executable, os.path.abspath(__file__)] + list(sys.argv[1:] if argv is None else argv),
                                    world)
    if code:
        sys.stderr.write(f"simulate_pixels.py --n_gpus {world}: ranks failed (rank, exit code): {bad}\n")
    raise SystemExit(code)


if __name__ == "__main__":
    launch_ranks_if_asked()

import numpy as np  # noqa: E402
import numpy.lib.recfunctions as rfn  # noqa: E402

from larndsim_amd import batching, charge_stats, consts, fee, light_sim, packets, synth  # noqa: E402
from larndsim_amd import config as cfgmod  # noqa: E402
from larndsim_amd import dist as ldist  # noqa: E402
from larndsim_amd import charge_universes as lcu  # noqa: E402
from larndsim_amd import fee_universes as lfu  # noqa: E402
from larndsim_amd import field_map as lfmap  # noqa: E402
from larndsim_amd import light_universes as llu  # noqa: E402
from larndsim_amd import pixel_truth as lptruth  # noqa: E402
from larndsim_amd import pixel_waveforms as lpwave  # noqa: E402
from larndsim_amd import rng as lrng  # noqa: E402
from larndsim_amd.chain import ChargeChain  # noqa: E402

SEED = int(time())
TRUTH_DATASETS = ("trajectories", "vertices", "mc_hdr", "mc_stack")


def _h5py():
    try:
        import h5py
        return h5py
    except ImportError:
        return None


def load_input(path, dset="segments"):
    """(segments, {truth dataset name: array}) from HDF5 (needs h5py), .npz (same dataset names) or .npy (segments only)."""
    if path.endswith(".npy"):
        return np.load(path), {}
    if path.endswith(".npz"):
        with np.load(path) as f:
            return f[dset], {k: f[k] for k in TRUTH_DATASETS if k in f.files}
    h5py = _h5py()
    if h5py is None:
        raise RuntimeError("HDF5 input needs h5py; .npy/.npz structured arrays with the same dtype are accepted")
    with h5py.File(path, "r") as f:
        return np.array(f[dset]), {k: np.array(f[k]) for k in TRUTH_DATASETS if k in f}


def prepare_tracks(tracks):
    """cli/simulate_pixels.py:482-494, 550-587: add missing columns, reset spill time, swap x<->z."""
    sim = consts.sim
    if "segment_id" not in tracks.dtype.names:
        tracks = rfn.append_fields(tracks, "segment_id", np.arange(tracks.shape[0], dtype="u4"), usemask=False)
    if "n_photons" not in tracks.dtype.names:
        tracks = rfn.append_fields(tracks, "n_photons", np.zeros(tracks.shape[0], dtype="f4"), usemask=False)
    if "t0" not in tracks.dtype.names:
        t0, t0s, t0e = tracks["t"].copy(), tracks["t_start"].copy(), tracks["t_end"].copy()
        tracks = rfn.append_fields(tracks, ["t0", "t0_start", "t0_end"], [t0, t0s, t0e], dtypes=["f4"] * 3,
                                   usemask=False)
        for f in ("t", "t_start", "t_end"):
            tracks[f] = 0
    if sim.IS_SPILL_SIM:
        ev = tracks[sim.EVENT_SEPARATOR]
        local = ev - (ev // sim.MAX_EVENTS_PER_FILE) * sim.MAX_EVENTS_PER_FILE
        for f in ("t0_start", "t0_end", "t0"):
            tracks[f] = tracks[f] - local * sim.SPILL_PERIOD
    return batching.swap_coordinates(tracks)


def gen_event_times(nevents, rng):
    """fee.gen_event_times (fee.py:70-82): cumulative exponential gaps after NON_BEAM_EVENT_GAP (numpy generator here, cupy's there)."""
    d = consts.detector
    return np.cumsum(rng.exponential(scale=d.EVENT_RATE, size=int(nevents))) + d.NON_BEAM_EVENT_GAP


class _Output:
    """HDF5 when h5py is importable, else one .npz with the same dataset names (written at close)."""

    def __init__(self, filename):
        self.filename = filename
        self.h5py = _h5py() if filename.endswith((".h5", ".hdf5")) else None
        if filename.endswith((".h5", ".hdf5")) and self.h5py is None:
            raise RuntimeError("HDF5 output needs h5py; give an .npz output name instead")
        self.parts = {}
        self.appended = set()           # datasets `append` has written rows of
        self.pixel_truth_tracks = 0     # rows of pixel_truth_tracks so far (pixel_truth's track_begin counts over the file)
        self.pixel_waveform_samples = 0   # values of pixel_waveform_samples so far (pixel_waveforms' sample_begin likewise)

    def append_packets(self, pk, assn):
        if self.h5py is not None:
            packets.write_hdf5(self.filename, pk, assn)
        else:
            self.parts.setdefault("packets", []).append(pk)
            self.parts.setdefault("mc_packets_assn", []).append(assn)

    def append(self, name, data):
        """resizable dataset grown along axis 0 (light_trig, light_wvfm, light_wvfm_mc_assn)"""
        if data.shape[0] == 0:
            return
        self.appended.add(name)
        if self.h5py is not None:
            with self.h5py.File(self.filename, "a") as f:
                light_sim._append(f, name, data, (None,) * data.ndim)
        else:
            self.parts.setdefault(name, []).append(data)

    def merge_module_waveforms(self, module_indices):
        """light_sim.merge_module_light_wvfm_same_trigger (light_sim.py:759-775): the per-module waveform datasets side by side
        along the channel axis as `light_wvfm`."""
        names = [f"light_wvfm/light_wvfm_mod{i}" for i in module_indices]
        if self.h5py is not None:
            with self.h5py.File(self.filename, "r") as f:
                present = all(n in f for n in names)
            if present:
                light_sim.merge_module_light_wvfm_same_trigger(self.filename, [i + 1 for i in module_indices])
            return
        if not all(n in self.parts for n in names):
            return
        parts = [np.concatenate(self.parts.pop(n)) for n in names]
        if len({p.shape[0] for p in parts}) != 1:
            raise ValueError("The number of triggers should be the same in each module with light trigger mode 1 "
                             "(light waveform).")
        self.parts["light_wvfm"] = [np.concatenate(parts, axis=1)]

    def put(self, name, data, attrs=None):
        if self.h5py is not None:
            with self.h5py.File(self.filename, "a") as f:
                ds = f.create_dataset(name, data=data)
                for k, v in (attrs or {}).items():
                    ds.attrs[k] = v
        else:
            self.parts[name.replace("/", "__")] = [data]

    def close(self, pixel_layout=None):
        if self.h5py is not None:                                   # cli/simulate_pixels.py:1299-1301
            with self.h5py.File(self.filename, "a") as f:
                if "configs" in f.keys() and pixel_layout is not None:
                    f["configs"].attrs["pixel_layout"] = pixel_layout
        if self.h5py is None:
            # stored members like np.savez (uncompressed like the HDF5 datasets they stand in for), each written from its
            # per-launch pieces as they are, checksummed on all host threads (larndsim_amd/npz_stream.py)
            from larndsim_amd.npz_stream import NpzStream
            with NpzStream(self.filename if self.filename.endswith(".npz") else self.filename + ".npz") as z:
                for k, v in self.parts.items():
                    if len(v):
                        z.write(k, v)


class _Collect:
    """what a rank > 0 of a sharded run would write: kept in memory for rank 0"""

    def __init__(self):
        self.parts = {}

    def append(self, name, data):
        if data.shape[0]:
            self.parts.setdefault(name, []).append(data)


def _prepend_t_event(arr):
    """The dataset with an f4 ``t_event`` field in front (aligned dtype, cli/simulate_pixels.py:618-625, 632-639)."""
    if "t_event" in arr.dtype.names:
        return arr
    descr = [("t_event", "f4")] + arr.dtype.descr
    new = np.empty(arr.shape, dtype=np.dtype(descr, align=True))
    for field in descr[1:]:
        if len(field[0]) == 0:
            continue
        new[field[0]] = arr[field[0]]
    return new


def attach_event_times(truth, event_times, sim):
    """Event times into the truth datasets that are passed through (cli/simulate_pixels.py:614-642): ``vertices['t_event']``
    for non-spill simulations -- one time per distinct event id, repeated over that event's rows in file order --, then
    copied row by row into ``mc_hdr``.  ``truth`` is changed in place."""
    if "vertices" in truth and not sim.IS_SPILL_SIM:
        vertices = _prepend_t_event(truth["vertices"])
        uniq_ev, counts = np.unique(vertices[sim.EVENT_SEPARATOR], return_counts=True)
        vertices["t_event"] = np.repeat(np.take(np.asarray(event_times), uniq_ev, mode="wrap"), counts)   # (cupy.take wraps)
        truth["vertices"] = vertices
    if "mc_hdr" in truth and "vertices" in truth and "t_event" in truth["vertices"].dtype.names:
        vertices, mc_hdr = truth["vertices"], _prepend_t_event(truth["mc_hdr"])
        if len(vertices) != len(mc_hdr):
            raise ValueError("vertices and mc_hdr datasets have different number of vertices! The number should be the same.")
        mc_hdr["t_event"] = vertices["t_event"]
        truth["mc_hdr"] = mc_hdr


def _as_list(v):
    """a flag given as 'a,b,c' (argparse) or a list (fire-style call) -> list; a plain value stays"""
    if isinstance(v, str) and "," in v:
        return [x.strip() for x in v.split(",") if x.strip()]
    return v


NUMBA_F32_FIELDS = ("x_start", "x_end", "y_start", "y_end", "z_start", "z_end", "tran_diff", "long_diff", "t_start")


def numba_f32_mode(flag, dtype):
    """--numba_f32 {auto,0,1} -> 0 / 1.  auto: 1 when the fields whose f4 storage makes Numba type sub-expressions of
    tracks_current as f32 are all f4 in the input records (the edep-sim schema), 0 when they are f8 (what the reference's own
    tests and the golden vectors use).  A mixed record keeps the all-f64 arithmetic and says so."""
    v = str(flag).strip().lower()
    if v in ("0", "false", "off"):
        return 0
    if v in ("1", "true", "on"):
        return 1
    if v != "auto":
        raise ValueError(f"--numba_f32 must be auto, 0 or 1, not {flag!r}")
    kinds = {np.dtype(dtype[f]).itemsize for f in NUMBA_F32_FIELDS if f in dtype.names and np.dtype(dtype[f]).kind == "f"}
    if kinds == {4}:
        return 1
    if kinds - {8}:
        print("[simulate_pixels] the segment records mix f4 and f8 hot-path fields: all-f64 arithmetic is used (--numba_f32 0)")
    return 0


def run_simulation(input_filename, output_filename, config="module0", mod2mod_variation=None, pixel_layout=None,
                   detector_properties=None, simulation_properties=None, response_file=None, light_simulated=None,
                   light_lut_filename=None, light_det_noise_filename=None, bad_channels=None, n_events=None,
                   pixel_thresholds_file=None, pixel_gains_file=None, rand_seed=None, config_root=None,
                   tracks_current_mc=False, chunk_segments=50000, raw_arrays=False, overlap_downloads=None,
                   pixel_layout_id=None, response_id=None, light_lut_id=None, pixel_thresholds_id=None, pixel_gains_id=None,
                   numba_f32="auto", n_gpus=None, force_dist=False, rng="table", field_map=None, charge_statistics=False,
                   fano_factor=None, pixel_truth=False, pixel_truth_min_charge=None, light_lut_interpolation="nearest",
                   pixel_waveforms=False, pixel_waveforms_threshold=None, pixel_waveforms_pad=None, pixel_waveforms_hits_only=False,
                   fee_universes=None, charge_universes=None, light_universes=None, sipm_crosstalk=None, sipm_afterpulse=None,
                   sipm_afterpulse_tau=None, sipm_dark_rate=None, **ignored):
    rank, world = launch.dist_mode(n_gpus, force_dist)
    if world is not None and "WORLD_SIZE" not in os.environ:
        raise RuntimeError(f"--n_gpus {n_gpus}: run_simulation runs one rank; start the ranks with main() (simulate_pixels.py "
                           "--n_gpus N starts them itself) or a launcher that sets WORLD_SIZE")
    if world is not None and world > 1 and raw_arrays:
        raise ValueError("--raw_arrays is not available with --n_gpus > 1: the per-pixel arrays stay on the rank that made them "
                         "(the compact path is the production one)")
    if world is not None and world > 1 and pixel_truth:
        raise ValueError("--pixel_truth is not available with --n_gpus > 1: its rows are not gathered over the ranks")
    if pixel_truth_min_charge is not None and not pixel_truth:
        raise ValueError("--pixel_truth_min_charge sets the selection of --pixel_truth: give --pixel_truth as well")
    if world is not None and world > 1 and pixel_waveforms:
        raise ValueError("--pixel_waveforms is not available with --n_gpus > 1: its rows are not gathered over the ranks")
    if (pixel_waveforms_threshold is not None or pixel_waveforms_pad is not None or pixel_waveforms_hits_only) \
            and not pixel_waveforms:
        raise ValueError("--pixel_waveforms_threshold, --pixel_waveforms_pad and --pixel_waveforms_hits_only set the selection of "
                         "--pixel_waveforms: give --pixel_waveforms as well")
    if world is not None and world > 1 and fee_universes:
        raise ValueError("--fee_universes is not available with --n_gpus > 1: its rows are not gathered over the ranks")
    if fee_universes is not None:
        for k, (name, changes) in enumerate(lfu.read(fee_universes)):           # (the file's keys, before anything is simulated)
            if lfu.changes_noisy(changes) and rng != "keyed":
                raise ValueError(FEE_UNIVERSES_NEED_KEYED.format(f"{k} ({name})"))
    if world is not None and world > 1 and charge_universes:
        raise ValueError("--charge_universes is not available with --n_gpus > 1: its rows are not gathered over the ranks")
    if charge_universes is not None:
        if charge_statistics:
            raise ValueError(CHARGE_UNIVERSES_NO_STATISTICS)
        if tracks_current_mc:
            raise ValueError(CHARGE_UNIVERSES_NO_MC)
        for k, (name, _, fee_changes) in enumerate(lcu.read(charge_universes)):   # (the file's keys, before anything is simulated)
            if lfu.changes_noisy(fee_changes) and rng != "keyed":
                raise ValueError(CHARGE_UNIVERSES_NEED_KEYED.format(f"{k} ({name})"))
    sipm = sipm_noise_of(sipm_crosstalk, sipm_afterpulse, sipm_afterpulse_tau, sipm_dark_rate)
    if sipm is not None and rng != "keyed":
        raise ValueError(SIPM_NOISE_NEEDS_KEYED)
    if light_universes is not None:
        if world is not None and world > 1:
            raise ValueError(LIGHT_UNIVERSES_NO_MULTI_GPU)
        if rng != "keyed":
            raise ValueError(LIGHT_UNIVERSES_NEED_KEYED)
        try:
            llu.read(light_universes)                                          # (the file's keys, before anything is simulated)
        except OSError as e:
            raise ValueError(f"--light_universes {light_universes}: {e}")
    wave_sel = None
    if pixel_waveforms:
        wave_sel = (float(pixel_waveforms_threshold or 0.0), int(pixel_waveforms_pad or 0), bool(pixel_waveforms_hits_only))
        try:
            lpwave.check_args(wave_sel[0], wave_sel[1])
        except ValueError as e:
            raise ValueError(f"--pixel_waveforms: {e}")
    if light_lut_interpolation not in LIGHT_LUT_INTERPOLATION:
        raise ValueError(f"--light_lut_interpolation must be nearest or trilinear, not {light_lut_interpolation!r}")
    if not os.path.exists(input_filename):
        raise Exception(f"Input file {input_filename} does not exist.")
    if rank == 0 and os.path.exists(output_filename):             # (only rank 0 writes)
        raise Exception(f"Output file {output_filename} already exists.")
    for k, v in ignored.items():
        if v is not None:
            print(f"[simulate_pixels] --{k} concerns a stage that is not built and is ignored")
    from larndsim_amd import lib
    if world is not None and n_gpus > lib.device_count():
        raise RuntimeError(f"--n_gpus {n_gpus} but only {lib.device_count()} GPU(s) are visible")

    # ---- configuration (cli/simulate_pixels.py:269-384) ------------------------------------------------------------------
    cfg = cfgmod.get_config(config, config_root)
    snapshot = cfg.get("SNAPSHOT")                                  # built-in keyword: numbers-only constants, no YAML files
    pixel_layout, response_file, light_lut_filename, pixel_thresholds_file, pixel_gains_file = (
        _as_list(v) for v in (pixel_layout, response_file, light_lut_filename, pixel_thresholds_file, pixel_gains_file))
    explicit_files = bool(detector_properties or pixel_layout or simulation_properties)
    if snapshot is None or explicit_files:
        pixel_layout = pixel_layout or cfg.get("PIXEL_LAYOUT")
        detector_properties = detector_properties or cfg.get("DET_PROPERTIES")
        simulation_properties = simulation_properties or cfg.get("SIM_PROPERTIES")
        if not (detector_properties and pixel_layout and simulation_properties) or snapshot is not None and not all(
                os.path.isfile(f) for f in [detector_properties, simulation_properties] + list(np.atleast_1d(pixel_layout))):
            raise AssertionError("pixel_layout, detector_properties and simulation_properties (files) must all be specified")
        snapshot = None
        n_modules = len(consts.get_n_modules(detector_properties))
    else:
        n_modules = len(snapshot) if isinstance(snapshot, list) else 1
    if response_file is None and snapshot is None:
        response_file = cfg.get("RESPONSE")
    if pixel_thresholds_file is None and cfg.get("PIXEL_THRESHOLDS_FILE"):   # :280-285
        pixel_thresholds_file = _as_list(cfg["PIXEL_THRESHOLDS_FILE"])
        if pixel_thresholds_id is None:
            pixel_thresholds_id = cfg.get("PIXEL_THRESHOLDS_ID")
    if pixel_gains_file is None and cfg.get("PIXEL_GAINS_FILE"):             # :286-291
        pixel_gains_file = _as_list(cfg["PIXEL_GAINS_FILE"])
        if pixel_gains_id is None:
            pixel_gains_id = cfg.get("PIXEL_GAINS_ID")
    if light_simulated is None:
        light_simulated = bool(cfg.get("LIGHT_SIMULATED", True))
    if light_simulated and light_lut_filename is None:
        light_lut_filename = cfg.get("LIGHT_LUT")
    m2m = cfgmod.module_variation_active(cfg, n_modules, mod2mod_variation,
                                         snapshot if snapshot is not None else pixel_layout, response_file, light_lut_filename)
    if m2m:                                                         # one entry per module (:374-384)
        # The reference reads the *_id flags (:272-290) and then looks the pointer lists up in the keyword's entry only
        # (load_mod2mod_variation_properties(cfg, ..), :106-122), so a list given on its command line never takes effect.
        # Here a given list is the pointer list -- what the flag is documented to be (:147-160) --, the keyword's otherwise.
        ids = {k: cfgmod.id_list(v) for k, v in (("PIXEL_LAYOUT_ID", pixel_layout_id), ("RESPONSE_ID", response_id),
                                                   ("LIGHT_LUT_ID", light_lut_id), ("PIXEL_THRESHOLD_ID", pixel_thresholds_id),
                                                   ("PIXEL_GAIN_ID", pixel_gains_id))}
        if snapshot is None:
            pixel_layout = cfgmod.module_files(cfg, pixel_layout, "PIXEL_LAYOUT_ID", n_modules, "pixel layout", ids["PIXEL_LAYOUT_ID"])
        response_file = cfgmod.module_files(cfg, response_file, "RESPONSE_ID", n_modules, "response files", ids["RESPONSE_ID"])
        pixel_thresholds_file = cfgmod.module_files(cfg, pixel_thresholds_file, "PIXEL_THRESHOLD_ID", n_modules,
                                                    "pixel threshold files", ids["PIXEL_THRESHOLD_ID"])
        pixel_gains_file = cfgmod.module_files(cfg, pixel_gains_file, "PIXEL_GAIN_ID", n_modules, "pixel gain files",
                                               ids["PIXEL_GAIN_ID"])
        light_lut_filename = cfgmod.module_files(cfg, light_lut_filename, "LIGHT_LUT_ID", n_modules, "light LUT", ids["LIGHT_LUT_ID"])
    else:
        if isinstance(snapshot, list):
            snapshot = snapshot[0]
        pixel_layout = cfgmod.single_file(pixel_layout, "pixel layout file")
        response_file = cfgmod.single_file(response_file, "response file")
        pixel_thresholds_file = cfgmod.single_file(pixel_thresholds_file, "pixel threshold file")
        pixel_gains_file = cfgmod.single_file(pixel_gains_file, "pixel gain file")
        light_lut_filename = cfgmod.single_file(light_lut_filename, "light lookup table")

    def load_constants(i_mod):
        """module i_mod's constants (i_mod = -1: the one configuration of all modules), :452-464, 678-682"""
        if snapshot is not None:
            consts.load_snapshot(snapshot[i_mod - 1] if m2m else snapshot)
        else:
            consts.load_properties(detector_properties, pixel_layout, simulation_properties, i_module=i_mod if m2m else -1)
        consts.sim.MOD2MOD_VARIATION = bool(m2m)

    def per_module(value, i_mod):
        return value[i_mod - 1] if (m2m and isinstance(value, (list, tuple))) else value

    load_constants(1 if m2m else -1)                               # geometry: any module's pixel layout will do (:657-661)
    det, sim, light = consts.detector, consts.sim, consts.light
    light_simulated = bool(light_simulated) and bool(light.LIGHT_SIMULATED) and light.N_OP_CHANNEL > 0
    if light_simulated and not all(f and os.path.isfile(f) for f in np.atleast_1d(light_lut_filename if light_lut_filename is not None else "")):
        print("light_lut_filename is not provided (required if light_simulated is True): light is not simulated")
        light_simulated = False
    if light_universes is not None and m2m:
        raise ValueError(LIGHT_UNIVERSES_NO_MODVAR)
    if light_universes is not None and not light_simulated:
        raise ValueError(LIGHT_UNIVERSES_NEED_LIGHT)
    if not rand_seed:
        rand_seed = SEED
    print("Random seed:", rand_seed)
    bad_list = None
    if bad_channels:
        import yaml
        with open(bad_channels) as f:
            bad_list = yaml.safe_load(f)

    # ---- input (:476-587) ---------------------------------------------------------------------------------------------------------
    tracks, truth = load_input(input_filename, sim.TRACKS_DSET_NAME)
    if tracks.size == 0:
        print("Empty input dataset, exiting")
        return None
    if n_events:
        max_ev = np.unique(tracks[sim.EVENT_SEPARATOR])[n_events - 1]
        tracks = tracks[tracks[sim.EVENT_SEPARATOR] <= max_ev]
        truth = {k: v[v[sim.EVENT_SEPARATOR] <= max_ev] for k, v in truth.items()}
    tracks = prepare_tracks(tracks)
    num_evids = int(tracks[sim.EVENT_SEPARATOR].max() % sim.MAX_EVENTS_PER_FILE) + 1
    host_rng = np.random.default_rng(rand_seed)
    event_times = (np.arange(num_evids) * sim.SPILL_PERIOD if sim.IS_SPILL_SIM else gen_event_times(num_evids, host_rng))
    attach_event_times(truth, event_times, sim)                                             # :614-642
    all_tracks = tracks[batching.select_active_volume(tracks, det.TPC_BORDERS)]            # :664-668
    all_events = np.unique(all_tracks[sim.EVENT_SEPARATOR])
    traj_field = "file_traj_id" if "file_traj_id" in all_tracks.dtype.names else "traj_id"
    mod_ids = list(det.MOD_IDS) if m2m else [-1]

    out = _Output(output_filename) if rank == 0 else _Collect()    # (ranks > 0 write nothing: their results travel to rank 0)
    totals = dict(n_segments=0, n_batches=0, n_hits=0, n_packets=0, n_light_triggers=0)
    rows_per_rank = np.zeros(world or 1, dtype=np.int64)
    kept_tracks, light_dat = [], {}
    rng_seeded = False
    lib.set_option("mc_current", 1 if tracks_current_mc else 0)
    # Numba types f32 (op) f32 as f32: with the real 152-byte schema (f4 coordinates, widths, times) a few sub-expressions of
    # tracks_current run in single precision in the reference (detsim.py:74-79,116-118,141,387); with f8 fields everything is f64.
    # "auto" follows the record's dtype.  The restatement of Numba's typing is UNPINNED (no Numba here to check it against:
    # INTEGRATION.md); it differs from all-f64 by up to 5e-5 of a waveform's peak.
    f32_mode = numba_f32_mode(numba_f32, all_tracks.dtype)
    print("Numba f32 typing mode:", "on" if f32_mode else "off", f"(--numba_f32 {numba_f32})")
    if rng not in ("table", "keyed"):
        raise ValueError(f"--rng must be table or keyed, not {rng!r}")
    print("Random streams:", rng, f"(--rng {rng})")
    field_maps = lfmap.load(field_map, len(det.TPC_BORDERS)) if field_map is not None else None
    print("Drift-field map:", f"{field_map} (TPCs {sorted(field_maps)})" if field_maps else "none (uniform field)")
    if charge_statistics and rng != "keyed":
        raise ValueError(CHARGE_STATISTICS_NEEDS_KEYED)
    fano = charge_stats.FANO_DEFAULT if fano_factor is None else float(fano_factor)
    print("Charge statistics:", f"on (--charge_statistics, Fano factor {fano:g})" if charge_statistics
          else "off (mean-value charge)")
    print("SiPM noise:", "off (Poisson fluctuations only)" if sipm is None else
          f"on (--sipm_crosstalk {sipm['crosstalk']:g}, --sipm_afterpulse {sipm['afterpulse']:g}, --sipm_afterpulse_tau "
          f"{sipm['afterpulse_tau']:g} us, --sipm_dark_rate {sipm['dark_rate']:g} per us)")
    truth_min = None if not pixel_truth else float(pixel_truth_min_charge or 0.0)
    if pixel_truth:                     # (without the flag the header, like the file, is what it was)
        print("Pixel charge truth:", f"on (--pixel_truth, --pixel_truth_min_charge {truth_min:g} e)")
    if pixel_waveforms:                 # (likewise)
        print("Pixel current waveforms:", f"on (--pixel_waveforms, --pixel_waveforms_threshold {wave_sel[0]:g}, "
              f"--pixel_waveforms_pad {wave_sel[1]}" + (", --pixel_waveforms_hits_only)" if wave_sel[2] else ")"))
    if fee_universes is not None:       # (likewise)
        print("FEE universes:", f"{fee_universes} (--fee_universes; hits only, no packets per universe)")
    if charge_universes is not None:    # (likewise)
        print("Charge universes:", f"{charge_universes} (--charge_universes; hits only, no packets per universe)")
    if light_universes is not None:     # (likewise)
        print("Light universes:", f"{light_universes} (--light_universes; triggers and waveforms, no truth slots per universe)")
    print("Light LUT interpolation:", light_lut_interpolation if light_lut_interpolation == "nearest"
          else f"{light_lut_interpolation} (--light_lut_interpolation {light_lut_interpolation})")
    lib.set_option("numba_f32", f32_mode)
    # once for the process-wide ctx: holds through the module loop and on every rank (each rank runs this function)
    lib.set_option("light_lut_interp", LIGHT_LUT_INTERPOLATION[light_lut_interpolation])
    dist = None
    if world is not None:
        from larndsim_amd import comm as lcomm
        dist = lcomm.Communicator(lib.context(refresh_consts=False), rank, world)
        n_rccl, r_rccl = dist.count()
        if (n_rccl, r_rccl) != (world, rank):
            raise RuntimeError(f"rank {rank} of {world}: the RCCL communicator reports rank {r_rccl} of {n_rccl}")
    universes_written = charge_universes_written = False
    try:
        for i_mod in mod_ids:                                       # convention: module ids count from 1 (:676-715)
            if m2m:
                print(f"Simulating module {i_mod - 1}")
                load_constants(i_mod)
                det, sim, light = consts.detector, consts.sim, consts.light
                det_borders = det.TPC_BORDERS[(i_mod - 1) * 2: i_mod * 2]
                tracks = all_tracks[batching.select_active_volume(all_tracks, det_borders)]
            else:
                det_borders = det.TPC_BORDERS
                tracks = all_tracks
            rf = per_module(response_file, i_mod)
            if rf and os.path.isfile(rf):
                response = np.load(rf)
            else:
                warnings.warn(f"response file {rf!r} not available (the reference checkout ships none): using the "
                              f"synthetic survey response table")
                response = synth.make_response("survey", response_sampling=det.RESPONSE_SAMPLING)
            chain = ChargeChain(response)
            chain.clear_pixel_tables()
            if field_maps:
                chain.set_field_map(field_maps)
            if charge_statistics:
                chain.set_charge_statistics(True, fano)
            if sipm is not None:
                chain.set_sipm_noise(**sipm)
            if not rng_seeded:
                # create_xoroshiro128p_states(1024*256, seed) (:396), once; rank r of a sharded run seeds rand_seed + r.
                # Keyed mode: every rank seeds rand_seed (the streams follow the identity of what is simulated)
                if rng == "keyed":
                    chain.seed_keyed(rank_seed(rand_seed, rank, rng))
                else:
                    chain.seed_rng(rank_seed(rand_seed, rank, rng))
                rng_seeded = True
            thr_file, gain_file = per_module(pixel_thresholds_file, i_mod), per_module(pixel_gains_file, i_mod)
            if thr_file is not None:                                # :439-443, 698-706, 1079-1084
                print("Pixel thresholds file:", thr_file)
                chain.set_pixel_thresholds(*fee.load_pixel_table(thr_file))
            if gain_file is not None:                               # :445-449, 1097-1100
                print("Pixel gains file:", gain_file)
                chain.set_pixel_gains(*fee.load_pixel_table(gain_file))
            universes = None
            if fee_universes is not None:
                # every universe is this module's constants with the file's keys applied
                uni_names, universes = lfu.load(fee_universes)
                for k, v in enumerate(universes):
                    if lfu.is_noisy(v) and rng != "keyed":
                        raise ValueError(FEE_UNIVERSES_NEED_KEYED.format(f"{k} ({uni_names[k]})"))
                if not universes_written:                               # (once: with module variation, the first module's values)
                    out.put("fee_universes", lfu.universe_rows(uni_names, universes))
                    universes_written = True
            cuni = None
            if charge_universes is not None:
                # every universe is this module's constants (and the driver's recombination model) with the file's keys applied
                cu_names, cu_charge, cu_fee = lcu.load(charge_universes, consts.physics.BIRKS)
                for k, v in enumerate(cu_fee):
                    if lfu.is_noisy(v) and rng != "keyed":
                        raise ValueError(CHARGE_UNIVERSES_NEED_KEYED.format(f"{k} ({cu_names[k]})"))
                if not charge_universes_written:                        # (once: with module variation, the first module's values)
                    out.put("charge_universes", lcu.universe_rows(cu_names, cu_charge, cu_fee))
                    charge_universes_written = True
                cuni = (cu_fee, cu_charge)
            luni = None
            if light_universes is not None:
                # every universe is the light constants with the file's keys applied (no module variation: written once)
                lu_names, lu_vars = llu.load(light_universes)
                out.put("light_universes", llu.universe_rows(lu_names, lu_vars))
                luni = lu_vars
            res = _simulate_module(chain, out, i_mod, m2m, tracks, all_events, det_borders, event_times, rand_seed, traj_field,
                                   per_module(light_lut_filename, i_mod) if light_simulated else None, light_det_noise_filename,
                                   cfg, len(mod_ids), bad_list, chunk_segments, raw_arrays, overlap_downloads, dist,
                                   keyed=rng == "keyed", pixel_truth_min=truth_min, pixel_waveforms_sel=wave_sel,
                                   fee_universes=universes, charge_universes=cuni, light_universes=luni)
            for k in totals:
                totals[k] += res[k]
            rows_per_rank += res["rows_per_rank"]
            kept_tracks.append(res["tracks"])
            if res["light_dat"] is not None:
                light_dat[i_mod] = res["light_dat"]
        if dist is not None:
            dist.destroy()
        if rank > 0:
            return None                                             # (rank 0 writes the file and the summary)
        # ---- end of file (:1226-1297) --------------------------------------------------------------------------------------------------
        out_tracks = np.concatenate(kept_tracks) if len(kept_tracks) > 1 else kept_tracks[0].copy()
        if sim.IS_SPILL_SIM:
            ev = out_tracks[sim.EVENT_SEPARATOR]
            local = ev - (ev // sim.MAX_EVENTS_PER_FILE) * sim.MAX_EVENTS_PER_FILE
            for f in ("t0_start", "t0_end", "t0"):
                out_tracks[f] = out_tracks[f] + local * sim.SPILL_PERIOD
        if light_simulated and light.LIGHT_TRIG_MODE == 1:          # one beam trigger per spill / event (:1252-1259)
            ev_all = out_tracks[sim.EVENT_SEPARATOR]
            lev = np.unique(ev_all - (ev_all // sim.MAX_EVENTS_PER_FILE) * sim.MAX_EVENTS_PER_FILE) if sim.IS_SPILL_SIM \
                else (truth["vertices"]["event_id"] if "vertices" in truth else np.unique(ev_all))
            lt = lev * sim.SPILL_PERIOD if sim.IS_SPILL_SIM else event_times
            out.append("light_trig", light_sim.build_light_trig(lev, np.full(len(lev), 0), np.full(len(lev), 0),
                                                                light.TPC_TO_OP_CHANNEL[:].ravel(), lt))
        if light_simulated and m2m and light.LIGHT_TRIG_MODE == 1:  # merge_module_light_wvfm_same_trigger (:759-775)
            out.merge_module_waveforms([m - 1 for m in mod_ids])
        batching.swap_coordinates(out_tracks)
        out.put(sim.TRACKS_DSET_NAME, out_tracks, attrs={"zbeam": True})
        for i_mod, dat in light_dat.items():
            out.put(f"light_dat/light_dat_module{i_mod - 1}" if m2m else "light_dat/light_dat_allmodules", dat)
        for k, v in truth.items():
            out.put(k, v)
        if pixel_truth:                 # (both datasets exist even when no pixel was reached)
            for name, dt in (("pixel_truth", lptruth.FILE_PIXEL), ("pixel_truth_tracks", lptruth.FILE_TRACK)):
                if name not in out.appended:
                    out.put(name, np.zeros(0, dtype=dt))
        if pixel_waveforms:             # (likewise)
            for name, dt in (("pixel_waveforms", lpwave.FILE_SPAN), ("pixel_waveform_samples", np.dtype("f4"))):
                if name not in out.appended:
                    out.put(name, np.zeros(0, dtype=dt))
        if fee_universes is not None and "fee_universe_hits" not in out.appended:
            out.put("fee_universe_hits", np.zeros(0, dtype=lfu.FILE_HIT))
        if charge_universes is not None and "charge_universe_hits" not in out.appended:
            out.put("charge_universe_hits", np.zeros(0, dtype=lcu.FILE_HIT))
        if light_universes is not None and "light_universe_trig" not in out.appended:
            out.put("light_universe_trig", llu.file_rows(0, 0, 0.0, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                                         np.zeros((0, 1), dtype=np.int32)))
        out.close(pixel_layout if isinstance(pixel_layout, str) else None if pixel_layout is None else list(pixel_layout))
    finally:
        lib.set_option("mc_current", 0)
        lib.set_option("numba_f32", 0)
        lib.set_option("light_lut_interp", 0)
        if charge_statistics:                                       # (the ctx is process-wide: leave it as it was found)
            lib.check(lib.load().ldsim_set_charge_statistics(lib.context(refresh_consts=False), 0, 0))
        if sipm is not None:
            lib.check(lib.load().ldsim_set_sipm_noise(lib.context(refresh_consts=False), 0, None))
    print(f"simulated {totals['n_segments']} segments in {totals['n_batches']} batches -> {totals['n_hits']} hits, "
          f"{totals['n_packets']} packets" + (f", {totals['n_light_triggers']} light triggers" if light_simulated else ""))
    print("Output saved in:", output_filename)
    totals["n_ranks"] = world or 1
    totals["rows_per_rank"] = [int(v) for v in rows_per_rank]
    return totals


def _simulate_module(chain, out, i_mod, m2m, tracks, all_events, det_borders, event_times, rand_seed, traj_field, light_lut,
                     light_det_noise_filename, cfg, n_mod_ids, bad_list, chunk_segments, raw_arrays, overlap_downloads=None,
                     dist=None, keyed=False, pixel_truth_min=None, pixel_waveforms_sel=None, fee_universes=None,
                     charge_universes=None, light_universes=None):
    """One pass of the driver's module loop body (cli/simulate_pixels.py:717-1232) on the device-resident chain: quench + drift,
    light leg, charge chain, packets.  ``tracks``: the module's active segments (all active segments without module
    variation); ``all_events``: event ids of every active segment (a module without segments in an event still reads out).

    ``dist`` (a larndsim_amd.comm.Communicator, --n_gpus): quench + drift and light incidence stay whole-input on every rank;
    the per-batch work -- photon sums, light response, triggers, waveforms, charge chain launches -- runs over the rank's
    contiguous run of whole events (dist.shard_events).  Ranks > 0 keep their light results on the host and their compact
    charge results in HBM; at the end of the module rank 0 receives them rank by rank and exports them after its own, so
    the file's rows come in the one-rank order."""
    det, sim, light = consts.detector, consts.sim, consts.light
    one = lambda v: v[0] if isinstance(v, (list, tuple)) else v          # noqa: E731
    bid, order, table = batching.assign_batches(tracks, tpc_borders=det_borders)
    tracks, bid = np.ascontiguousarray(tracks[order]), bid[order]
    nsim = int((bid >= 0).sum())
    res = dict(n_segments=nsim, n_batches=len(table), n_hits=0, n_packets=0, n_light_triggers=0, light_dat=None)
    if len(tracks):                                                 # a module may hold no segment at all: it still reads out
        chain.upload(tracks, bid)
        if keyed:
            chain.set_batch_keys(table, i_mod)
        chain.quench_drift(consts.physics.BIRKS)
        chain.download_segments(tracks)
    # the batch-sorted copy is the device's; the file gets the module's segments in input order, like the reference's
    # `segments_to_files = tracks` (cli/simulate_pixels.py:1230-1234), with light_dat rows aligned to it (:759-760)
    file_rows = np.empty_like(tracks)
    file_rows[order] = tracks
    res["tracks"] = file_rows
    edges = np.flatnonzero(np.r_[True, bid[1:nsim] != bid[:nsim - 1], True]) if nsim else np.array([0])
    n_groups = int(np.ceil(np.asarray(det_borders).shape[0] / sim.EVENT_BATCH_SIZE))
    rank, world = (dist.rank, dist.world) if dist is not None else (0, 1)
    res["rows_per_rank"] = np.zeros(world, dtype=np.int64)
    own_edges = edges                                               # segment boundaries of the batches this rank simulates
    owner = lambda ev: 0                                            # noqa: E731  (rank that simulates an event)
    if dist is not None:
        brank = ldist.shard_events(table, world)
        mine = np.flatnonzero(brank == rank)
        own_edges = edges[mine[0]:mine[-1] + 2] if len(mine) else np.array([0])
        ev_of_b = np.array([t[0] for t in table])

        def owner(ev):
            # an event without a batch in this module (its light leg still reads out) goes with the next event that has one
            if not len(table):
                return 0
            return int(brank[min(int(np.searchsorted(ev_of_b, ev, side="left")), len(table) - 1)])
    batch_of = {}
    for ib, (ev, grp, sub, _n) in enumerate(table):
        batch_of.setdefault((int(ev), int(grp)), []).append(ib)
    light_trig_of = {}                                              # (event, TPC group) -> trigger arrays for the packet stream
    if light_lut is not None:
        lut = np.load(light_lut)["arr"]
        mask = lut["vis"] > 0                                       # no voxel with 0 visibility (:778-780)
        lut["vis"][~mask] = lut["vis"][mask].min()
        n_light_channel = int(light.N_OP_CHANNEL / n_mod_ids) if m2m else light.N_OP_CHANNEL        # :750
        if len(tracks):
            chain.light_incidence(lut, n_out=n_light_channel)
        # in the module-variation case the channel indices of the first module stand for every module's (:1127-1131)
        op_channel = (light.TPC_TO_OP_CHANNEL[:2].ravel() if m2m else light.TPC_TO_OP_CHANNEL[:].ravel()).astype(np.int32)
        n_det = op_channel.shape[0]
        noise_file = light_det_noise_filename or one(cfg.get("LIGHT_DET_NOISE"))
        if noise_file and os.path.isfile(noise_file):
            print("Light detector noise: ", noise_file)
            light_noise = np.load(noise_file)
            if m2m:
                light_noise = light_noise[n_light_channel * (i_mod - 1): n_light_channel * i_mod]          # :789-790
        else:
            print("light_det_noise_filename is not provided (required if light_simulated is True): no detector noise")
            light_noise = None
        digit_samples = ceil((light.LIGHT_TRIG_WINDOW[1] + light.LIGHT_TRIG_WINDOW[0]) / light.LIGHT_DIGIT_SAMPLE_SPACING)
        # group thresholds of the active channels (:1183-1185)
        thr = np.repeat(np.array(light.LIGHT_TRIG_THRESHOLD)[..., np.newaxis], light.OP_CHANNEL_PER_TRIG, axis=-1)
        thr = thr.ravel()[op_channel].copy().reshape(-1, light.OP_CHANNEL_PER_TRIG)[..., 0]
        wvfm_name = f"light_wvfm/light_wvfm_mod{i_mod - 1}" if (m2m and light.LIGHT_TRIG_MODE == 1) else "light_wvfm"
        light_rows, i_trig = [], 0
        null_wvfm = None
        for ev in all_events:                                       # the reference's loop order: events, TPC groups (:864)
            if owner(ev) != rank:
                continue
            ev_time = np.array([event_times[int(ev) % sim.MAX_EVENTS_PER_FILE]])
            for grp in range(n_groups):
                acc = dict(start=[], idx=[], typ=[], opc=[], wv=[], tid=[], tph=[])
                ibs = batch_of.get((int(ev), grp), [])
                if not ibs:
                    # nothing to simulate in this module group: waveforms of an empty response (:805-841, 894-899)
                    if null_wvfm is None or keyed:
                        # (keyed: the noise of an empty group's waveforms belongs to that (event, group), so no cache)
                        if keyed:
                            chain.set_rng_key(lrng.call_key(i_mod, int(ev), grp, -1))
                        nt0 = int((light.LIGHT_WINDOW[1] + light.LIGHT_WINDOW[0]) / light.LIGHT_TICK_SIZE)
                        zero = np.zeros((n_det, nt0), dtype=np.float32)
                        mt = sim.MAX_MC_TRUTH_IDS
                        null_wvfm = light_sim.sim_triggers(
                            None, None, zero, op_channel, np.full((n_det, nt0, mt), -1, dtype=np.int64),
                            np.zeros((n_det, nt0, mt)), np.array([0]), op_channel[None, :], digit_samples, light_noise)
                    acc["start"].append(np.full(1, 0.0)); acc["idx"].append(np.array([0]))
                    acc["typ"].append(np.full(1, light.LIGHT_TRIG_MODE)); acc["opc"].append(op_channel[None, :])
                    for k, v in zip(("wv", "tid", "tph"), null_wvfm):
                        acc[k].append(v)
                    for ku, lv in enumerate(light_universes or ()):
                        # --light_universes: the empty response is every universe's; only its noise follows noise_scale
                        u_wv = null_wvfm[0]
                        if light_noise is not None and lv["noise_scale"] != 1.0:
                            u_wv = light_sim.sim_triggers(None, None, zero, op_channel, None, None, np.array([0]),
                                                          op_channel[None, :], digit_samples, light_noise * lv["noise_scale"])[0]
                        out.append("light_universe_trig", llu.file_rows(ku, int(ev), 0.0, np.array([0]),
                                                                        np.full(1, light.LIGHT_TRIG_MODE), op_channel[None, :]))
                        out.append("light_universe_wvfm", u_wv)
                for ib in ibs:                                      # sub-batches of BATCH_SIZE segments (:902-905, 1120-1205)
                    b0, b1 = int(edges[ib]), int(edges[ib + 1])
                    n_ticks, t_start = chain.sum_light(b0, b1, op_channel,
                                                       segment_track_id=tracks["segment_id"][b0:b1].astype(np.int64))
                    if raw_arrays:
                        light_rows.append(chain.download_light(truth=False)[0])
                    if keyed:
                        chain.set_rng_key(lrng.call_key(i_mod, int(ev), grp, int(table[ib][2])))
                    else:
                        chain.extend_rng(n_det * (-(-int(n_ticks) // 64)) * 64, rand_seed + int(ev) + table[ib][2] * sim.BATCH_SIZE)
                    chain.light_response(fluctuate=True)
                    t_idx, t_opc, t_type = light_sim.get_triggers(None, thr, op_channel, table[ib][2])
                    wv = light_sim.sim_triggers(None, None, None, op_channel, None, None, t_idx, t_opc, digit_samples,
                                                light_noise)
                    acc["start"].append(np.full(t_idx.shape[0], t_start)); acc["idx"].append(t_idx)
                    acc["typ"].append(t_type); acc["opc"].append(t_opc)
                    for k, v in zip(("wv", "tid", "tph"), wv):
                        acc[k].append(v)
                    if light_universes is not None:
                        # --light_universes: the same photon sum under every universe's constants and the same call key, then
                        # the calls just made for the nominal, on each universe's response (thresholds and noise spectrum scaled)
                        chain.light_universes(light_universes, fluctuate=True)
                        for ku, lv in enumerate(light_universes):
                            u_idx, u_opc, u_type = light_sim.get_triggers_universe(ku, thr * lv["trig_threshold_scale"], op_channel,
                                                                                   table[ib][2])
                            u_noise = None if light_noise is None else light_noise * lv["noise_scale"]
                            u_wv = light_sim.sim_triggers_universe(ku, op_channel, u_idx, u_opc, digit_samples, u_noise)
                            if u_idx.shape[0]:
                                out.append("light_universe_trig", llu.file_rows(ku, int(ev), t_start, u_idx, u_type, u_opc))
                                out.append("light_universe_wvfm", u_wv)
                if not any(len(a) for a in acc["idx"]):
                    continue
                cat = {k: np.concatenate(v, axis=0) for k, v in acc.items()}
                ntr = cat["idx"].shape[0]
                lev = np.full(ntr, ev)
                if light.LIGHT_TRIG_MODE == 0:
                    out.append("light_trig", light_sim.build_light_trig(lev, cat["start"], cat["idx"], cat["opc"], ev_time))
                out.append(wvfm_name, cat["wv"])
                if sim.MAX_MC_TRUTH_IDS > 0:
                    out.append("light_wvfm_mc_assn",
                               light_sim.zero_suppress_waveform_truth(cat["tid"], cat["tph"], lev[0], i_trig, i_mod))
                i_trig += 1
                res["n_light_triggers"] += ntr
                if ibs:
                    mods = (cat["typ"] if light.LIGHT_TRIG_MODE == 1 else
                            np.array([det.TPC_TO_MODULE[int(t)] for t in light.OP_CHANNEL_TO_TPC[cat["opc"]][:, 0]]))
                    light_trig_of[(int(ev), grp)] = (cat["start"] + cat["idx"] * light.LIGHT_TICK_SIZE, lev, mods)
        if len(tracks):
            inc, _ = chain.download_light_incidence(0, len(tracks))
            inc["segment_id"] = tracks["segment_id"][:, None]
            inc_file = np.empty_like(inc)
            inc_file[order] = inc
            res["light_dat"] = inc_file
        if raw_arrays and light_rows:
            nt_max = max(r.shape[1] for r in light_rows)           # the tick count follows each batch's arrival times
            out.put("light_sample_inc" + (f"_mod{i_mod - 1}" if m2m else ""),
                    np.stack([np.pad(r, ((0, 0), (0, nt_max - r.shape[1]))) for r in light_rows]))
        if dist is not None:
            # the ranks' light results to rank 0 (small: trigger rows, waveforms, truth rows, the trigger tuples of the packet
            # stream), appended after its own in rank order; truth rows carry the rank's running trigger index from 0
            payload = pickle.dumps((out.parts, light_trig_of, i_trig, res["n_light_triggers"]), protocol=5) if rank else b""
            counts = dist.gatherv_bytes(payload)
            if rank > 0:
                out.parts.clear()
            else:
                for r in range(1, world):
                    parts, trig_of, n_calls, n_trig = pickle.loads(dist.gathered_bytes(r, counts))
                    for name, arrs in parts.items():
                        data = np.concatenate(arrs)
                        if name == "light_wvfm_mc_assn":
                            data["trigger_id"] += i_trig
                        out.append(name, data)
                    light_trig_of.update(trig_of)
                    i_trig += n_calls
                    res["n_light_triggers"] += n_trig

    # ---- sync / timestamp / trigger packets at every new event (:866-890), then the event's charge packets ------------------
    period = det.CLOCK_RESET_PERIOD * det.CLOCK_CYCLE
    sync_start = event_times[0] // period * period + period
    io_rows = np.array(list(det.MODULE_TO_IO_GROUPS.values()))
    trig_module = int(np.argwhere(io_rows == packets.get_trig_io())[0][0]) + 1
    announced = 0                                                   # events of all_events whose packets are out

    def announce_until(event):
        nonlocal sync_start, announced
        while announced < len(all_events) and all_events[announced] <= event:
            t_ev = event_times[int(all_events[announced]) % sim.MAX_EVENTS_PER_FILE]
            if t_ev - sync_start >= 0:
                sync_times = np.arange(sync_start, t_ev + 1, period)
                if len(sync_times):
                    spk = packets.build_sync_packets(np.full(sync_times.shape, period), i_mod)
                    out.append_packets(*spk)
                    res["n_packets"] += len(spk[0])
                    sync_start = sync_times[-1] + period
            if i_mod == trig_module or i_mod == -1:                 # the trigger is forwarded to one PACMAN only
                tpk = packets.build_timestamp_trigger_packets([t_ev], i_mod)
                out.append_packets(*tpk)
                res["n_packets"] += len(tpk[0])
            announced += 1

    parts = []
    seg_ids_all = tracks["segment_id"].astype(np.int64)            # (once: a copy of the tail per batch is quadratic in a spill)
    trj_ids_all = tracks[traj_field].astype(np.int64)

    # Batches per export (sim.WRITE_BATCH_SIZE, default 1; cli/simulate_pixels.py:1207-1214): the reference gathers that many
    # batches' arrays and hands fee.export_to_hdf5 their concatenation (save_results, :179-258) -- one set of timestamp / sync /
    # trigger packets per event of the export, clock-rollover state from its first row -- and exports what is left after the event
    # loop.  A batch counts when it holds a pixel the chain returns rows for.
    write_batch = max(int(getattr(sim, "WRITE_BATCH_SIZE", 1)), 1)
    pending = []            # (event, arrays of the batch, its light triggers or None)

    event_of_batch = np.array([t[0] for t in table], dtype=np.int64)
    first_seg_of_batch = np.searchsorted(bid[:nsim], np.arange(len(table)), side="left").astype(np.int64)

    def export_triggers(events_in_order):
        """light triggers embedded in the charge stream of an export (:206-222)"""
        uniq = np.unique(np.asarray(events_in_order))
        ev_time = np.array([event_times[int(e) % sim.MAX_EVENTS_PER_FILE] for e in uniq])
        if all(p[2] is None for p in pending):
            # each event triggers once at perfect t0 (:218-222)
            return ev_time, (np.zeros(len(uniq)), uniq, np.ones(len(uniq)))
        # the simulated triggers of the export's batches (:209-216); a batch without any keeps the perfect one
        trip = [p[2] if p[2] is not None else (np.zeros(1), np.array([p[0]]), np.ones(1)) for p in pending]
        return ev_time, tuple(np.concatenate([np.atleast_1d(t[k]) for t in trip]) for k in range(3))

    def flush_pending_compact():
        """the same export from the compact rows of the chain, through the native hit loop (ldsim_packets_build): no dense
        [pixel][30][50] fraction rows are rebuilt to feed an array-shaped exporter"""
        pieces = [packets.compact_to_rows(p[1][1], event_of_batch, first_seg_of_batch, seg_ids_all, trj_ids_all, rows=p[1][2:4])
                  for p in pending]
        rows = pieces[0] if len(pieces) == 1 else {k: np.concatenate([q[k] for q in pieces]) for k in pieces[0]}
        ev_time, (lt_times, lt_events, lt_mods) = export_triggers([p[0] for p in pending])
        pk, assn = packets.build_packets_compact(**rows, event_start_times=ev_time, light_trigger_times=lt_times,
                                                 light_trigger_event_id=lt_events, light_trigger_modules=lt_mods,
                                                 bad_channels=bad_list, i_mod=i_mod)
        out.append_packets(pk, assn)
        res["n_packets"] += len(pk)
        pending.clear()

    def flush_pending():
        if not pending:
            return
        if isinstance(pending[0][1][0], str):           # ("compact", download, first row, row after the last)
            return flush_pending_compact()
        events = [p[0] for p in pending]
        cat = [np.concatenate([p[1][k] for p in pending]) if len(pending) > 1 else pending[0][1][k] for k in range(7) if k != 4]
        # (the fraction rows, 12 KB per pixel: batches that follow each other in one launch's array are one slice of it)
        src = [p[3] for p in pending]
        one_run = all(a is not None and b is not None and a[0] is b[0] and a[2] == b[1] for a, b in zip(src[:-1], src[1:]))
        frac = src[0][0][src[0][1]:src[-1][2]] if (one_run and src[0] is not None) else \
            (np.concatenate([p[1][4] for p in pending]) if len(pending) > 1 else pending[0][1][4])
        cat.insert(4, frac)
        uniq = np.unique(np.asarray(events))
        ev_time = np.array([event_times[int(e) % sim.MAX_EVENTS_PER_FILE] for e in uniq])
        if all(p[2] is None for p in pending):
            # each event triggers once at perfect t0 (:218-222)
            lt_times, lt_events, lt_mods = np.zeros(len(uniq)), uniq, np.ones(len(uniq))
        else:
            # the simulated triggers of the export's batches (:209-216); a batch without any keeps the perfect one
            trip = [p[2] if p[2] is not None else (np.zeros(1), np.array([p[0]]), np.ones(1)) for p in pending]
            lt_times, lt_events, lt_mods = (np.concatenate([np.atleast_1d(t[k]) for t in trip]) for k in range(3))
        pk, assn = packets.build_packets(*cat, ev_time, light_trigger_times=lt_times, light_trigger_event_id=lt_events,
                                         light_trigger_modules=lt_mods, bad_channels=bad_list, i_mod=i_mod)
        out.append_packets(pk, assn)
        res["n_packets"] += len(pk)
        pending.clear()

    def export_chunk_compact(c):
        """packets and association rows of one chain launch from its compact download: a batch is a run of hit-pixel rows (its
        first unique pixel always among them, hits or not: kernels_compact.hip)"""
        hp = c["hit_pixels"]
        rb = hp[:, 2]
        starts = np.flatnonzero(np.r_[True, rb[1:] != rb[:-1]]) if len(rb) else np.zeros(0, dtype=np.int64)
        ends = np.r_[starts[1:], len(rb)]
        for a, b in zip(starts, ends):
            bb = int(rb[a])
            event = table[bb][0]
            announce_until(event)
            pending.append((event, ("compact", c, int(a), int(b)), light_trig_of.get((int(event), int(table[bb][1]))), None))
            if len(pending) >= write_batch:
                flush_pending()
        res["n_hits"] += len(c["hit_rows"])

    def export_chunk(r):
        """packets and association rows of one chain launch (`r`: the launch's per-pixel arrays)"""
        # the chain returns the unique pixels ordered by batch: a batch is a contiguous run (a view, not a 12 KB-per-pixel copy
        # of the backtracking array); an unordered result falls back to masks
        rb = r["batch"]
        ordered = len(rb) < 2 or bool((rb[1:] >= rb[:-1]).all())
        for bb in np.unique(rb):
            m = slice(int(np.searchsorted(rb, bb, side="left")), int(np.searchsorted(rb, bb, side="right"))) if ordered \
                else rb == bb
            lo = int(np.searchsorted(bid[:nsim], bb, side="left"))
            seg_ids, trj_ids = seg_ids_all[lo:], trj_ids_all[lo:]
            tpm = r["track_pixel_map"][m]
            digit, ticks_b, upix_b, frac_b = r["adc_digit"][m], r["adc_ticks_list"][m], r["unique_pix"][m], r["current_fractions"][m]
            # (compact form: a batch whose first unique pixel holds no hit comes with that hit-less row in front --
            # expand_compact(lead_rows=True) -- because the reference's exporter keeps its clock-rollover state in row 0 of what
            # it is handed, fee.py:164-183, 267-277)
            track_ids = np.where(tpm >= 0, seg_ids[np.maximum(tpm, 0)], -1)
            traj_ids = np.where(tpm >= 0, trj_ids[np.maximum(tpm, 0)], -1)
            event = table[int(bb)][0]
            announce_until(event)
            ev_ids = np.full(digit.shape, event)
            # light triggers embedded in the charge stream (:209-221): the simulated ones, else one perfect trigger per event
            pending.append((event, (ev_ids, digit, ticks_b, upix_b, frac_b, track_ids, traj_ids),
                            light_trig_of.get((int(event), int(table[int(bb)][1]))),
                            (r["current_fractions"], m.start, m.stop) if ordered else None))
            if len(pending) >= write_batch:
                flush_pending()
        # batches that wait for the next launch's: their rows are views of this launch's arrays, which a later download may
        # overwrite (page-locked buffers are reused) -- keep copies
        for i, p in enumerate(pending):
            if p[3] is not None:
                pending[i] = (p[0], tuple(np.array(a) for a in p[1]), p[2], None)
        res["n_hits"] += int((r["adc_list"] != 0).sum())
        if raw_arrays:
            r = {k: np.array(v) for k, v in r.items()}       # (views of page-locked buffers that later launches reuse)
            r["event_id"] = np.array([t[0] for t in table])[r["batch"]]
            parts.append(r)

    def export_pixel_waveforms():
        """--pixel_waveforms: the last launch's pixel current waveforms (ChargeChain.pixel_waveforms) as rows of the file's two
        datasets, sample_begin counted over the whole file"""
        if pixel_waveforms_sel is None:
            return
        thr, pad, hits_only = pixel_waveforms_sel
        rows, samples = lpwave.file_rows(chain.pixel_waveforms(thr, pad, hits_only), event_of_batch, out.pixel_waveform_samples)
        out.pixel_waveform_samples += len(samples)
        out.append("pixel_waveforms", rows)
        out.append("pixel_waveform_samples", samples)

    def export_fee_universes():
        """--fee_universes: the last launch digitised again under every universe (ChargeChain.fee_universes), as hit rows"""
        if fee_universes is None:
            return
        out.append("fee_universe_hits", lfu.file_rows(chain.fee_universes(fee_universes), event_of_batch))

    def export_charge_universes():
        """--charge_universes: the last launch re-weighted and digitised again under every universe (ChargeChain.universes), as
        hit rows; a pass of its own beside --fee_universes"""
        if charge_universes is None:
            return
        cu_fee, cu_charge = charge_universes
        out.append("charge_universe_hits", lcu.file_rows(chain.universes(fee=cu_fee, charge=cu_charge), event_of_batch))

    def export_pixel_truth():
        """--pixel_truth: the last launch's pixel charge truth (ChargeChain.pixel_truth) as rows of the file's two datasets;
        segment ids mapped like mc_packets_assn's (packets.compact_to_rows), track_begin counted over the whole file"""
        if pixel_truth_min is None:
            return
        rows, entries = lptruth.file_rows(chain.pixel_truth(pixel_truth_min), event_of_batch, first_seg_of_batch, seg_ids_all,
                                          out.pixel_truth_tracks)
        out.pixel_truth_tracks += len(entries)
        out.append("pixel_truth", rows)
        out.append("pixel_truth_tracks", entries)

    # What crosses PCIe per launch: the compact form (hit pixels, hits, per-hit fractions: ldsim_chain_compact_*), expanded on the
    # host to the dense rows of the hit pixels -- the only rows the exporter reads.  --raw_arrays wants every unique pixel's
    # arrays and takes the dense download: launch k's rows then travel on the library's copy stream (download_async) while
    # launch k - 1's packets are built (page-locking the two sets of host arrays costs ~0.5 s: from about eight launches on).
    from larndsim_amd.chain import expand_compact
    overlapped = raw_arrays and ((nsim >= 8 * chunk_segments) if overlap_downloads is None else bool(overlap_downloads))
    b = 0
    in_flight = None
    launches = [(int(b0), int(e0)) for b0, e0 in _launch_ranges(own_edges, int(own_edges[-1]), chunk_segments)]
    if dist is not None:
        dist.accumulate_compact(reset=True)
    if rank > 0:
        # a rank > 0 exports nothing: its launches' compact results stay in HBM until rank 0 gathers them
        for b0, e0 in launches:
            chain.run(b0, e0, want_fractions=True)
            chain.build_compact()
            dist.accumulate_compact()
        for r in range(1, world):                                   # (collective: every rank takes part in each rank's turn)
            dist.gather_compact(r)
        return res
    if not raw_arrays:
        # Default path.  Launch k runs on a worker thread (ChargeChain.run_async: the C call blocks on its size read-backs but
        # releases the interpreter) while launch k - 1's packets are built here from its compact download -- host work that never
        # enters the ctx.
        prev = None
        for b0, e0 in launches:
            chain.run_async(b0, e0, want_fractions=True)
            if prev is not None:
                export_chunk_compact(prev)
            chain.wait()
            prev = chain.download_compact()
            export_pixel_truth()
            export_pixel_waveforms()
            export_fee_universes()
            export_charge_universes()
        if prev is not None:
            export_chunk_compact(prev)
        launches = []
    for b, e in launches:
        chain.run(int(b), int(e), want_fractions=True)
        export_pixel_truth()
        export_pixel_waveforms()
        export_fee_universes()
        export_charge_universes()
        if not overlapped:
            export_chunk(chain.download())
            continue
        arriving = chain.download_async()
        if in_flight is not None:
            export_chunk(in_flight)
        in_flight = arriving
    if in_flight is not None:
        chain.wait_download()
        export_chunk(in_flight)
    res["rows_per_rank"][0] = res["n_hits"]
    if dist is not None:
        # rank 0's own launches were exported as they came; the others' streams arrive one rank at a time (rank 0 holds one
        # of them, in HBM and on the host), each exported through the same pending / WRITE_BATCH_SIZE bookkeeping as if it had
        # come from rank 0's own launches before the next rank's is received
        for r in range(1, world):
            sizes = dist.gather_compact(r)
            c = dist.gathered_compact(r, sizes)
            res["rows_per_rank"][r] = len(c["hit_rows"])
            export_chunk_compact(c)
            del c
    if len(all_events):
        announce_until(all_events[-1])
    flush_pending()                                  # (what is left after the event loop, :1219-1222)
    if raw_arrays and parts:
        for k in parts[0]:
            out.put(("raw/" if not m2m else f"raw_mod{i_mod - 1}/") + k, np.concatenate([p[k] for p in parts]))
    return res


def rank_seed(rand_seed, rank, rng="table"):
    """the seed rank `rank` gives its random streams: rand_seed + rank in table mode, rand_seed itself in keyed mode"""
    return int(rand_seed) if rng == "keyed" else int(rand_seed) + int(rank)


def _launch_ranges(edges, nsim, chunk_segments):
    """segment ranges of the chain launches over the batches of ``edges`` (batch boundaries, ending at ``nsim``): whole batches,
    at least chunk_segments each (the last one: what is left)"""
    b = edges[0]
    for e in edges[1:]:
        if e - b >= chunk_segments or e == nsim:
            yield b, e
            b = e


def main(argv=None):
    launch_ranks_if_asked(argv)                                     # (does not return when it started the ranks)
    a = vars(_parse_args(argv))
    rank, world = launch.dist_mode(a["n_gpus"], a["force_dist"])
    if world is not None and os.environ.get("LDSIM_CLI_REHEARSAL"):
        # CPU rehearsal of the launch path (tests/test_cpu_multirank.py): the ranks meet over the ncclUniqueId hand-out and stop
        # before anything touches a GPU; LDSIM_CLI_REHEARSAL_FAIL_RANK=r makes rank r exit non-zero before the rendezvous
        from larndsim_amd import comm as lcomm

        def say(line):          # (the ranks share the launcher's stdout and print together: line and newline in one write, or an
            print(line + "\n", end="", flush=True)          # unbuffered stdout lets the other rank's line in between)

        say(f"rehearsal: rank {rank} of {world} started (pid {os.getpid()})")
        if a["field_map"] is not None:
            say(f"rehearsal: rank {rank} field_map {a['field_map']}")
        if a["light_lut_interpolation"] != "nearest":
            say(f"rehearsal: rank {rank} light_lut_interpolation {a['light_lut_interpolation']}")
        if os.environ.get("LDSIM_CLI_REHEARSAL_FAIL_RANK") == str(rank):
            raise SystemExit(f"rank {rank}: asked to fail (test of the launcher's error path)")
        got = lcomm.exchange_id(bytes(range(128)) if rank == 0 else b"", rank, world, timeout=120.0)
        if got != bytes(range(128)):
            raise SystemExit(f"rank {rank}: rendezvous payload differs")
        say(f"rehearsal: rank {rank} of {world} met")
        return
    run_simulation(**a)


if __name__ == "__main__":
    main()
