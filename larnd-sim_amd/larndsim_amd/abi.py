"""
ctypes mirror of include/ldsim.h (struct layouts + ``pack_consts``).

Only declarations live here; loading the shared library is in ``lib.py``.
"""
import ctypes as C

import numpy as np

from . import consts
from .layout import LdsimTrackLayout, NFIELDS  # noqa: F401  (re-exported)

LDSIM_MAX_TPC = 128

LDSIM_OK, LDSIM_EINVAL, LDSIM_EHIP, LDSIM_ENOSPC, LDSIM_ESTATE, LDSIM_ENODEV = 0, -1, -2, -3, -4, -5
LDSIM_ENOMEM, LDSIM_ENOCONV = -6, -7


class LdsimConsts(C.Structure):
    _fields_ = [
        ("box_alpha", C.c_double), ("box_beta", C.c_double), ("birks_ab", C.c_double), ("birks_kb", C.c_double),
        ("w_ion", C.c_double),
        ("w_ph", C.c_double), ("scint_prescale", C.c_double),
        ("e_field", C.c_double), ("lar_density", C.c_double), ("v_drift", C.c_double),
        ("electron_lifetime", C.c_double), ("long_diff", C.c_double), ("tran_diff", C.c_double),
        ("n_tpc", C.c_int32), ("default_plane_index", C.c_int32),
        ("tpc_borders", C.c_double * 2 * 3 * LDSIM_MAX_TPC),
        ("n_pixels", C.c_int32 * 2), ("sampled_points", C.c_int32), ("n_time_ticks", C.c_int32),
        ("pixel_pitch", C.c_double),
        ("time_sampling", C.c_double), ("time_padding", C.c_double), ("time_window", C.c_double),
        ("time_interval", C.c_double * 2),
        ("response_sampling", C.c_double), ("response_bin_size", C.c_double),
        ("discrimination_threshold", C.c_double), ("clock_cycle", C.c_double), ("buffer_risetime", C.c_double),
        ("gain", C.c_double), ("v_cm", C.c_double), ("v_ref", C.c_double), ("v_pedestal", C.c_double),
        ("adc_hold_delay", C.c_int32), ("adc_busy_delay", C.c_int32), ("reset_cycles", C.c_int32),
        ("adc_counts", C.c_int32),
        ("reset_noise_charge", C.c_double), ("uncorrelated_noise_charge", C.c_double),
        ("discriminator_noise", C.c_double),
        ("max_tracks_per_pixel", C.c_int32), ("max_adc_values", C.c_int32),
        ("light_trig_mode", C.c_int32), ("enable_lut_smearing", C.c_int32),
        ("n_op_channel", C.c_int32), ("max_mc_truth_ids", C.c_int32),
        ("light_tick_size", C.c_double), ("mc_truth_threshold", C.c_double),
        ("light_window", C.c_double * 2), ("singlet_fraction", C.c_double), ("tau_s", C.c_double), ("tau_t", C.c_double),
        ("light_response_time", C.c_double), ("light_oscillation_period", C.c_double),
        ("impulse_tick_size", C.c_double), ("sipm_response_model", C.c_int32), ("mc_sample_multiplier", C.c_int32),
        ("min_step_size", C.c_double),
        ("light_trig_window", C.c_double * 2), ("light_digit_sample_spacing", C.c_double),
        ("light_det_noise_sample_spacing", C.c_double), ("light_nbit", C.c_int32), ("op_channel_per_trig", C.c_int32),
    ]


class LdsimChainStats(C.Structure):
    _fields_ = [("n_segments", C.c_int64), ("n_pairs", C.c_int64), ("n_unique", C.c_int64),
                ("n_batches", C.c_int64), ("n_overflow", C.c_int64),
                ("max_active", C.c_int32), ("max_neigh", C.c_int32), ("max_length", C.c_int32),
                ("n_ambiguous", C.c_int32), ("n_dfma", C.c_int64), ("n_fallback", C.c_int64), ("n_samples", C.c_int64), ("n_wbuf", C.c_int64),
                ("n_dfma_useful", C.c_int64)]


class LdsimFeeVariation(C.Structure):
    """include/ldsim.h LdsimFeeVariation (ldsim_chain_fee_universes): 112 bytes, absolute values"""
    _fields_ = [("discrimination_threshold", C.c_double), ("gain", C.c_double), ("v_cm", C.c_double), ("v_ref", C.c_double),
                ("v_pedestal", C.c_double), ("buffer_risetime", C.c_double),
                ("reset_noise_charge", C.c_double), ("uncorrelated_noise_charge", C.c_double), ("discriminator_noise", C.c_double),
                ("threshold_table_scale", C.c_double), ("threshold_table_offset", C.c_double), ("gain_table_scale", C.c_double),
                ("adc_hold_delay", C.c_int32), ("adc_busy_delay", C.c_int32), ("reset_cycles", C.c_int32), ("pad", C.c_int32)]


class LdsimChargeVariation(C.Structure):
    """include/ldsim.h LdsimChargeVariation (ldsim_chain_universes): 56 bytes, absolute values"""
    _fields_ = [("electron_lifetime", C.c_double), ("w_ion", C.c_double), ("box_alpha", C.c_double), ("box_beta", C.c_double),
                ("birks_ab", C.c_double), ("birks_kb", C.c_double), ("recomb_mode", C.c_int32), ("pad", C.c_int32)]


class LdsimLightVariation(C.Structure):
    """include/ldsim.h LdsimLightVariation (ldsim_dev_light_universes): 56 bytes, absolute values"""
    _fields_ = [("photon_scale", C.c_double), ("singlet_fraction", C.c_double), ("tau_s", C.c_double), ("tau_t", C.c_double),
                ("gain_scale", C.c_double), ("response_time", C.c_double), ("oscillation_period", C.c_double)]


class LdsimSipmNoise(C.Structure):
    """include/ldsim.h LdsimSipmNoise (ldsim_set_sipm_noise): 32 bytes"""
    _fields_ = [("crosstalk", C.c_double), ("afterpulse", C.c_double), ("afterpulse_tau", C.c_double), ("dark_rate", C.c_double)]


class LdsimLutBuildParams(C.Structure):
    """include/ldsim.h LdsimLutBuildParams (ldsim_light_lut_build): 112 bytes"""
    _fields_ = [("box", C.c_double * 3), ("rayleigh_cm", C.c_double), ("absorption_cm", C.c_double),
                ("group_velocity_cm_ns", C.c_double), ("wall_reflectivity", C.c_double * 6), ("emit_mode", C.c_int32),
                ("max_steps", C.c_int32), ("nprof", C.c_int32), ("reserved", C.c_int32)]


class LdsimLutDetector(C.Structure):
    """include/ldsim.h LdsimLutDetector: 40 bytes; wall 0..5 = u0 u1 v0 v1 w0 w1, lo / hi in the wall's in-plane coordinates"""
    _fields_ = [("wall", C.c_int32), ("pad", C.c_int32), ("lo", C.c_double * 2), ("hi", C.c_double * 2)]


class LdsimResponseBuildParams(C.Structure):
    """include/ldsim.h LdsimResponseBuildParams (ldsim_response_build): 56 bytes"""
    _fields_ = [("pad_size", C.c_double), ("bin_size", C.c_double), ("v_drift", C.c_double), ("sampling", C.c_double),
                ("n_i", C.c_int32), ("n_j", C.c_int32), ("n_k", C.c_int32), ("n_sub", C.c_int32), ("arrival_tick", C.c_int32),
                ("_pad", C.c_int32)]


class LdsimFieldMapBuildParams(C.Structure):
    """include/ldsim.h LdsimFieldMapBuildParams (ldsim_field_map_solve / _trace): 168 bytes"""
    _fields_ = [("origin", C.c_double * 3), ("spacing", C.c_double * 3), ("z_anode", C.c_double), ("z_cathode", C.c_double),
                ("e0", C.c_double), ("temperature", C.c_double), ("mobility", C.c_double * 6), ("tol", C.c_double),
                ("step", C.c_double), ("n", C.c_int32 * 3), ("max_iters", C.c_int32), ("check_every", C.c_int32),
                ("_pad", C.c_int32)]


class LdsimTrackGenParams(C.Structure):
    """include/ldsim.h LdsimTrackGenParams (ldsim_track_gen / _count): 192 bytes"""
    _fields_ = [("world_lo", C.c_double * 3), ("world_hi", C.c_double * 3), ("step", C.c_double), ("min_step", C.c_double),
                ("max_loss_fraction", C.c_double), ("t_cut", C.c_double), ("t_min", C.c_double), ("density", C.c_double),
                ("z_over_a", C.c_double), ("mean_excitation", C.c_double), ("rad_length", C.c_double), ("k_coeff", C.c_double),
                ("sternheimer", C.c_double * 6), ("straggling", C.c_int32), ("mcs", C.c_int32), ("energy_loss", C.c_int32),
                ("max_steps", C.c_int32)]


class LdsimTrackGenPrimary(C.Structure):
    """include/ldsim.h LdsimTrackGenPrimary: 80 bytes (track_generator.primary_dtype is the same record in numpy)"""
    _fields_ = [("pos", C.c_double * 3), ("dir", C.c_double * 3), ("kinetic_energy", C.c_double), ("time", C.c_double),
                ("pdg", C.c_int32), ("event_id", C.c_int32), ("track_in_event", C.c_int32), ("_pad", C.c_int32)]


class LdsimTrackGenParticle(C.Structure):
    """include/ldsim.h LdsimTrackGenParticle: 104 bytes (track_cascade.particle_dtype is the same record in numpy)"""
    _fields_ = LdsimTrackGenPrimary._fields_ + [("key", C.c_uint64), ("parent", C.c_int32), ("generation", C.c_int32),
                                                ("process", C.c_int32), ("parent_step", C.c_int32)]


class LdsimTrackGenCascadeParams(C.Structure):
    """include/ldsim.h LdsimTrackGenCascadeParams (ldsim_track_cascade / _count): 48 bytes"""
    _fields_ = [("t_track", C.c_double), ("mu_plus_lifetime", C.c_double), ("mu_minus_lifetime", C.c_double),
                ("capture_fraction", C.c_double), ("delta_tracks", C.c_int32), ("decays", C.c_int32), ("emit", C.c_int32),
                ("_pad", C.c_int32)]


FIELD_MAP_BUILD_MAX_STEPS = 1048576   # include/ldsim.h LDSIM_FIELD_MAP_BUILD_MAX_STEPS
RESPONSE_BUILD_MAX_K = 7679       # include/ldsim.h LDSIM_RESPONSE_BUILD_MAX_K
RESPONSE_BUILD_MAX_NSUB = 16      # include/ldsim.h LDSIM_RESPONSE_BUILD_MAX_NSUB
LUT_MAX_DETECTORS = 1024    # include/ldsim.h LDSIM_LUT_MAX_DETECTORS
LUT_MAX_NPROF = 512         # include/ldsim.h LDSIM_LUT_MAX_NPROF
FEE_UNIVERSES_MAX = 64      # include/ldsim.h LDSIM_FEE_UNIVERSES_MAX
LIGHT_UNIVERSES_MAX = 64    # include/ldsim.h LDSIM_LIGHT_UNIVERSES_MAX

ABI_VERSION = 8      # include/ldsim.h LDSIM_ABI_VERSION: the struct layouts of this file

# slots of ldsim_debug_gform_census, in the order of include/ldsim.h's LDSIM_GC_* enum (tests/test_cpu_host.py compares the two)
GFORM_CENSUS_SLOTS = (
    "pairs", "tables", "flagged", "emitted", "t_wave", "t_wide", "t_wg", "wg_shifts", "wg_bins", "wg_slices", "wg_forced",
    "nb1", "nb2", "nb3p", "rows4", "rows8", "rows12", "rows16", "cls0", "cls1", "cls2", "cls0_zrec", "cls1_zrec", "cls2_zrec",
    "nu_over_cap", "emask0", "emask1", "emask2", "m", "tt", "qb0", "qb12")
GFORM_CENSUS_N = len(GFORM_CENSUS_SLOTS)


def pack_consts(noise_zero=False):
    """Freeze the current ``consts`` namespaces into the plain struct the C-ABI takes."""
    d, l, s, p = consts.detector, consts.light, consts.sim, consts.physics
    c = LdsimConsts()
    c.box_alpha, c.box_beta, c.birks_ab, c.birks_kb, c.w_ion = p.BOX_ALPHA, p.BOX_BETA, p.BIRKS_Ab, p.BIRKS_kb, p.W_ION
    c.w_ph, c.scint_prescale = l.W_PH, l.SCINT_PRESCALE
    c.e_field, c.lar_density, c.v_drift = d.E_FIELD, d.LAR_DENSITY, d.V_DRIFT
    c.electron_lifetime, c.long_diff, c.tran_diff = d.ELECTRON_LIFETIME, d.LONG_DIFF, d.TRAN_DIFF
    B = np.asarray(d.TPC_BORDERS, dtype=np.float64)
    if B.shape[0] > LDSIM_MAX_TPC:
        raise ValueError(f"{B.shape[0]} TPCs > LDSIM_MAX_TPC")
    c.n_tpc = B.shape[0]
    c.default_plane_index = d.DEFAULT_PLANE_INDEX
    flat = np.zeros((LDSIM_MAX_TPC, 3, 2))
    flat[:B.shape[0]] = B
    C.memmove(C.addressof(c.tpc_borders), flat.ctypes.data, flat.nbytes)
    c.n_pixels[0], c.n_pixels[1] = int(d.N_PIXELS[0]), int(d.N_PIXELS[1])
    c.sampled_points = d.SAMPLED_POINTS
    c.n_time_ticks = len(d.TIME_TICKS)
    c.pixel_pitch = d.PIXEL_PITCH
    c.time_sampling, c.time_padding, c.time_window = d.TIME_SAMPLING, d.TIME_PADDING, d.TIME_WINDOW
    c.time_interval[0], c.time_interval[1] = float(d.TIME_INTERVAL[0]), float(d.TIME_INTERVAL[1])
    c.response_sampling, c.response_bin_size = d.RESPONSE_SAMPLING, d.RESPONSE_BIN_SIZE
    c.discrimination_threshold = d.DISCRIMINATION_THRESHOLD
    c.clock_cycle, c.buffer_risetime, c.gain = d.CLOCK_CYCLE, d.BUFFER_RISETIME, d.GAIN
    c.v_cm, c.v_ref, c.v_pedestal = d.V_CM, d.V_REF, d.V_PEDESTAL
    c.adc_hold_delay, c.adc_busy_delay, c.reset_cycles = d.ADC_HOLD_DELAY, d.ADC_BUSY_DELAY, d.RESET_CYCLES
    c.adc_counts = d.ADC_COUNTS
    z = 0.0 if noise_zero else 1.0
    c.reset_noise_charge = d.RESET_NOISE_CHARGE * z
    c.uncorrelated_noise_charge = d.UNCORRELATED_NOISE_CHARGE * z
    c.discriminator_noise = d.DISCRIMINATOR_NOISE * z
    c.max_tracks_per_pixel, c.max_adc_values = s.MAX_TRACKS_PER_PIXEL, s.MAX_ADC_VALUES
    c.light_trig_mode, c.enable_lut_smearing = l.LIGHT_TRIG_MODE, int(bool(l.ENABLE_LUT_SMEARING))
    c.n_op_channel, c.max_mc_truth_ids = int(l.N_OP_CHANNEL), int(s.MAX_MC_TRUTH_IDS)
    c.light_tick_size, c.mc_truth_threshold = l.LIGHT_TICK_SIZE, s.MC_TRUTH_THRESHOLD
    c.light_window[0], c.light_window[1] = float(l.LIGHT_WINDOW[0]), float(l.LIGHT_WINDOW[1])
    c.singlet_fraction, c.tau_s, c.tau_t = l.SINGLET_FRACTION, l.TAU_S, l.TAU_T
    c.light_response_time, c.light_oscillation_period = l.LIGHT_RESPONSE_TIME, l.LIGHT_OSCILLATION_PERIOD
    c.impulse_tick_size, c.sipm_response_model = l.IMPULSE_TICK_SIZE, int(l.SIPM_RESPONSE_MODEL)
    c.mc_sample_multiplier, c.min_step_size = int(s.MC_SAMPLE_MULTIPLIER), float(s.MIN_STEP_SIZE)
    c.light_trig_window[0], c.light_trig_window[1] = float(l.LIGHT_TRIG_WINDOW[0]), float(l.LIGHT_TRIG_WINDOW[1])
    c.light_digit_sample_spacing = float(l.LIGHT_DIGIT_SAMPLE_SPACING)
    c.light_det_noise_sample_spacing = float(l.LIGHT_DET_NOISE_SAMPLE_SPACING)
    c.light_nbit, c.op_channel_per_trig = int(l.LIGHT_NBIT), int(l.OP_CHANNEL_PER_TRIG)
    return c


class LdsimPacketsIn(C.Structure):
    """include/ldsim.h LdsimPacketsIn (ldsim_packets_build)"""
    _fields_ = [("n_rows", C.c_int64), ("row_event", C.c_void_p), ("row_base", C.c_void_p), ("row_ts_s", C.c_void_p),
                ("row_ok", C.c_void_p), ("row_io_group", C.c_void_p), ("row_io_channel", C.c_void_p), ("row_chip", C.c_void_p),
                ("row_channel", C.c_void_p), ("row_hit0", C.c_void_p), ("row_trk0", C.c_void_p), ("row_frac0", C.c_void_p),
                ("hit_adc", C.c_void_p), ("hit_tick", C.c_void_p), ("hit_frac", C.c_void_p), ("trk_segment", C.c_void_p),
                ("trk_traj", C.c_void_p), ("base0", C.c_int64), ("first_row_is_row0", C.c_int32), ("light_trig_mode", C.c_int32),
                ("n_trig", C.c_int64), ("trig_time", C.c_void_p), ("trig_event", C.c_void_p), ("trig_module", C.c_void_p),
                ("n_io_groups", C.c_int32), ("io_groups", C.c_void_p), ("n_modules", C.c_int32), ("module_ids", C.c_void_p),
                ("module_group0", C.c_void_p), ("module_groups", C.c_void_p), ("clock_reset_period", C.c_int64),
                ("clock_cycle", C.c_double), ("mus", C.c_double), ("s", C.c_double), ("n_keep", C.c_int32), ("max_tracks", C.c_int32)]
