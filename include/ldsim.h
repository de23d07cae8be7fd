/*
 * ldsim.h -- C-ABI of libldsim_hip.so: larnd-sim's charge/light hot path on MI355X (gfx950).
 *
 * The reference (DUNE/larnd-sim @2024-10-16) has no FFI for this path: the path sits behind
 * Python call sites `module.kernel[blocks, threads](ndarray, ...)` in one driver loop
 * (reference cli/simulate_pixels.py:732,742,797,923,944,1002,1016,1036,1057,1087,1150) plus
 * module-global constants frozen at JIT time.  Each entry point below names the reference
 * kernel / call site it replaces.  Conventions (same as the reference's call sites):
 *   - the caller owns every buffer; outputs are sized by the caller;
 *   - `tracks` is an array of records (any layout described by LdsimTrackLayout) mutated in place;
 *   - every function returns 0 on success or a negative LDSIM_E* code; ldsim_last_error()
 *     returns a thread-local message.  Nothing throws across the boundary.
 *   - one ldsim_ctx per device/process; a ctx is thread-compatible, not thread-safe.
 *
 * Two families:
 *   (1) stage-by-stage, HOST buffers in / out ("materialising" forms: one per reference kernel,
 *       used by the parity tests and by a drop-in driver);
 *   (2) device-resident chain: upload the segments once, run quench -> drift -> pixels ->
 *       induced current -> per-pixel sum -> ADC entirely in HBM, download per-pixel results.
 */
#ifndef LDSIM_H
#define LDSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDSIM_ABI_VERSION 8

/* error codes */
#define LDSIM_OK 0
#define LDSIM_EINVAL (-1)   /* bad argument */
#define LDSIM_EHIP (-2)     /* HIP runtime error (message has the hipError string) */
#define LDSIM_ENOSPC (-3)   /* caller-provided capacity too small (required size reported) */
#define LDSIM_ESTATE (-4)   /* call order violated (e.g. no response table set) */
#define LDSIM_ENODEV (-5)   /* no usable GPU */
#define LDSIM_ENOMEM (-6)   /* a device allocation of the call failed (the context stays usable) */
#define LDSIM_ENOCONV (-7)  /* an iterative solve missed its tolerance within its iteration limit (residual reported) */

/* record field dtype codes */
enum { LDSIM_F4 = 1, LDSIM_F8 = 2, LDSIM_I4 = 3, LDSIM_U4 = 4, LDSIM_I8 = 5, LDSIM_U8 = 6 };

/* hot-path record fields (reference cli/dumpTree.py:17-28 names) */
enum ldsim_field {
  LDSIM_X_START = 0, LDSIM_Y_START, LDSIM_Z_START, LDSIM_X_END, LDSIM_Y_END, LDSIM_Z_END,
  LDSIM_X, LDSIM_Y, LDSIM_Z, LDSIM_DEDX, LDSIM_DE, LDSIM_T, LDSIM_T_START, LDSIM_T_END,
  LDSIM_T0, LDSIM_T0_START, LDSIM_T0_END, LDSIM_N_ELECTRONS, LDSIM_N_PHOTONS,
  LDSIM_LONG_DIFF, LDSIM_TRAN_DIFF, LDSIM_PIXEL_PLANE, LDSIM_NFIELDS
};

/* Where each field lives inside one record; offset < 0 = field absent (reads 0, never written). */
typedef struct {
  int32_t itemsize;
  int32_t offset[LDSIM_NFIELDS];
  int32_t dtype[LDSIM_NFIELDS];
} LdsimTrackLayout;

#define LDSIM_MAX_TPC 128

/* Constants the reference keeps as module globals (larndsim/consts/{detector,light,sim,physics}.py),
 * passed as a plain struct instead of being frozen into JIT-compiled kernels. */
typedef struct {
  /* physics.py */
  double box_alpha, box_beta, birks_ab, birks_kb, w_ion;
  /* light.py: quenching needs W_PH and SCINT_PRESCALE */
  double w_ph, scint_prescale;
  /* detector.py drift */
  double e_field, lar_density, v_drift, electron_lifetime, long_diff, tran_diff;
  /* geometry */
  int32_t n_tpc;
  int32_t default_plane_index;             /* 0xBEEF */
  double tpc_borders[LDSIM_MAX_TPC][3][2]; /* [tpc][x,y,z][lo,hi]; anode = [.][2][0] */
  int32_t n_pixels[2];
  int32_t sampled_points;                  /* 40 */
  int32_t n_time_ticks;                    /* len(TIME_TICKS) */
  double pixel_pitch;
  /* time / response */
  double time_sampling, time_padding, time_window, time_interval[2];
  double response_sampling, response_bin_size;
  /* FEE */
  double discrimination_threshold, clock_cycle, buffer_risetime, gain, v_cm, v_ref, v_pedestal;
  int32_t adc_hold_delay, adc_busy_delay, reset_cycles, adc_counts;
  double reset_noise_charge, uncorrelated_noise_charge, discriminator_noise;
  int32_t max_tracks_per_pixel, max_adc_values;
  /* light */
  int32_t light_trig_mode, enable_lut_smearing;
  int32_t n_op_channel, max_mc_truth_ids;
  double light_tick_size, mc_truth_threshold;
  /* light waveform response (ABI 2): scintillation_model (light_sim.py:131-146), sipm_response_model (:274-300) */
  double light_window[2];                  /* LIGHT_WINDOW: conv_ticks = ceil((w[1] - w[0]) / LIGHT_TICK_SIZE) */
  double singlet_fraction, tau_s, tau_t;
  double light_response_time, light_oscillation_period, impulse_tick_size;
  int32_t sipm_response_model;             /* 0 = RLC model, 1 = measured impulse (IMPULSE_MODEL passed as an array) */
  int32_t mc_sample_multiplier;            /* sim.MC_SAMPLE_MULTIPLIER (ABI 3, tracks_current_mc, detsim.py:318-323) */
  double min_step_size;                    /* sim.MIN_STEP_SIZE [cm] */
  /* light triggers and digitisation (ABI 4): get_triggers / sim_triggers / gen_light_detector_noise, light_sim.py:339-619 */
  double light_trig_window[2];             /* LIGHT_TRIG_WINDOW [us] */
  double light_digit_sample_spacing;       /* LIGHT_DIGIT_SAMPLE_SPACING [us] */
  double light_det_noise_sample_spacing;   /* LIGHT_DET_NOISE_SAMPLE_SPACING [us] */
  int32_t light_nbit;                      /* LIGHT_NBIT */
  int32_t op_channel_per_trig;             /* OP_CHANNEL_PER_TRIG */
} LdsimConsts;

typedef struct ldsim_ctx ldsim_ctx;

/* ---- context ------------------------------------------------------------------------------ */
const char* ldsim_last_error(void);
int ldsim_abi_version(void);
int ldsim_device_count(void);
/* consts.load_properties + importlib.reload (cli/simulate_pixels.py:431,458-464) */
int ldsim_ctx_create(int device, const LdsimConsts* consts, ldsim_ctx** out);
int ldsim_ctx_destroy(ldsim_ctx* ctx);
/* page-locked host memory for the download / upload buffers of a caller that wants PCIe-rate copies (hipHostMalloc) */
int ldsim_host_alloc(void** p, size_t bytes);
int ldsim_host_free(void* p);
/* test seam: device buffers, streams and events the library holds in this process, over all contexts (page-locked host memory
 * is not counted).  All three are 0 once every context is destroyed. */
int ldsim_debug_live_objects(int64_t counts[3]);
/* test seam (host arithmetic, no device): the key bits the chain's pair-list sort looks at for a largest pixel id and a batch
 * count.  ranges = {e0, b1, e1}: a stable LSD sort over [0, e0), then one over [b1, e1) if e1 > b1 (else none).  Every key
 * batch << 36 | pixel << 4 | ring code with pixel <= pixel_max and batch < n_batches is zero outside them. */
int ldsim_debug_sort_key_ranges(uint64_t pixel_max, int64_t n_batches, int32_t ranges[3]);
int ldsim_set_consts(ldsim_ctx* ctx, const LdsimConsts* consts);
/* cp.load(response_file) (cli/simulate_pixels.py:436): f64 table [ni][nj][nk], host pointer */
int ldsim_set_response(ldsim_ctx* ctx, const double* response, int32_t ni, int32_t nj, int32_t nk);
/* light.OP_CHANNEL_EFFICIENCY / OP_CHANNEL_TO_TPC (consts/light.py:109-119) */
int ldsim_set_light_channels(ldsim_ctx* ctx, const double* efficiency, const int32_t* op_channel_to_tpc, int32_t n);
/* np.load(light_lut)['arr'] as SoA planes: vis,t0,t0_avg [nx*ny*nz*ndet] f32; time_dist [..*nprof] f32 */
int ldsim_set_light_lut(ldsim_ctx* ctx, const float* vis, const float* t0, const float* t0_avg,
                        const float* time_dist, int32_t nx, int32_t ny, int32_t nz, int32_t ndet, int32_t nprof);
/* tuning / validation knobs: "prune_log" (weights below exp(-v) of the local peak are skipped, 0 = keep all;
 * default 23 = 1e-10 of the peak like the quadrature rule: ADC charges move by < 1e-8 relative against keeping everything,
 * tools/prune_sweep.py; 30 was the default before and costs 16-19 % more correlation work),
 * "tail_log" (split path: charge samples bounded by exp(-v) of the segment's peak density are evaluated in f32,
 * relative error ~3e-7 of a term that small; 0 = every sample in f64),
 * "trim_response" (1 = skip leading/trailing response ticks that are empty for every cell), "trim_response_log" (what empty
 * means: below exp(-v) of the table's largest entry; default 23 = 1e-10, the level the weights are pruned at -- such ticks move a
 * waveform by less than 1e-10 of its peak; 0 = exactly 0.0 only),
 * "split_kernels" (1 = weights_kernel + mac_kernel, 0 = monolithic current_kernel),
 * "wbuf_doubles_per_pair" (initial average budget of the split path's weight pool; the pool grows to the measured
 * demand and the launch is repeated when it was exhausted, so this only affects the first launches; setting it forgets
 * the size learned so far), "split_max_items" (validation: pairs with more weight items than this are recomputed by
 * the monolithic kernel; 0 = the built-in capacity: 512 items at TIME_SAMPLING/RESPONSE_SAMPLING = 1, 2048 at 2),
 * "weights_mode" (split path: 2 = node-separable form, gtables_kernel + gcorr_kernel: the quadrature's tables correlated on the
 * f64 matrix pipe, no weight pool ("mac_mode" does not apply); 1 = qweights_kernel, Gauss-Legendre quadrature along the
 * segment, then the correlation kernel of "mac_mode"; 0 = weights_kernel, the closed form per charge sample),
 * "gform_max_support" (weights_mode 2 runs the node-separable form for response tables whose staged support is at most this
 * many time ticks and the kernels of weights_mode 1 for wider ones: the matrix form pays per response tick, the shifted-window
 * kernels per 512-tick tile; 0 = never, 1e9 = always = the default since round 4 -- 768 before, when full-support tables were
 * faster in the shifted-window kernels), "gform_chunks" (weights_mode 2: tables and correlation in this many ranges of the pair list, the tables of a range on a second
 * stream beside the correlation of the one before; 1..32, default 1: measured no faster), "gform_wave_tables" (weights_mode 2, tables stage: 1 =
 * gtables_wave_kernel, one wave per pair, for the pairs that fit it and gtables_kernel, one workgroup per pair, for the rest
 * (default); 0 = gtables_kernel for all: same tables entry for entry), "quad_max_nodes" (qweights_kernel: pairs that need more nodes,
 * i.e. segments longer than ~value/2 Gaussian widths, are recomputed by the monolithic kernel; 8..256, default 256),
 * "quad_accuracy_log10" (tables / weights stage: Gauss-Legendre nodes along the segment for a quadrature error of 1e-v of the peak
 * weight, v = 7 (default since round 4: N = ceil(3.4 + 1.38 r) nodes for a clipped segment r Gaussian widths long; per tick the
 * result stays at 0.012 of the parity tolerance 1e-5 |ref| + 1e-7 peak against the reference's goldens, where the f4 rounding of
 * the stored currents already is -- tools/quad_sweep.py, profiles/r04_acc_sweep_module0.log), 8, 9, 10 (4.8 + 1.6 r, the default
 * of rounds 2-3), 12 (6 + 1.9 r), or looser: 6 (3.0 + 1.3 r: 3.7 % faster, 0.033 of the tolerance at worst, but the pixel charges
 * move by 4.5e-8 against the closed form -- beyond the 2e-8 the parity tests hold them to, so it is not the default) and 5
 * (2.8 + 1.2 r: 0.32 of the tolerance) -- profiles/r04_acc_sweep_module0_5_6.log),
 * "mac_mode" (split path, correlation stage: 1 = mac_shift_kernel / mac_shift2_kernel (default), 0 = mac_kernel<M>, rows
 * staged in LDS; bit-identical results), "light_incidence_scalar" (1 = calculate_light_incidence with one channel per lane
 * instead of four (the form used when n_out or the LUT's detector count is not a multiple of 4); identical bits; default 0),
 * "light_lut_interp" (ldsim_light_incidence / ldsim_dev_light_incidence: 0 (default) = the visibility of the LUT voxel that holds
 * the segment, like the reference; 1 = interpolated trilinearly between the eight voxel centres around it -- per axis, with f the
 * voxel coordinate lightLUT.get_voxel forms before it truncates, u = f - 0.5, i0 = floor(u), corners clamp(i0) and clamp(i0 + 1) to
 * [0, n - 1] with weights 1 - (u - i0) and u - i0 (beyond the outermost centres both are the same voxel: constant, no
 * extrapolation), corner c = 4 dx + 2 dy + dz weighing (wx[dx] * wy[dy]) * wz[dz], n_photons_det from the f64 sum over the
 * corners in that order; t0_det from the weight-renormalised mean of t0 over the corners with visibility > 0, the nearest
 * voxel's t0 when none is lit; `voxel` stays the nearest voxel, so the photon sum's time profile is not interpolated; numpy
 * twin: larndsim_amd/lightLUT.py interpolated_light_incidence; another value returns LDSIM_EINVAL),
 * "light_sum_no_list" (1 = ldsim_dev_sum_light without truth slots launches a workgroup per (detector, tick tile) and clears
 * the whole array first, instead of summing over the device-built list of the lit tiles; same cells, values to the order of
 * the f64 additions; default 0), "light_sum_async" (1 = the ldsim_dev_sum_light calls without truth slots launch on a stream of the
 * ctx's own beside whatever its main stream carries next, e.g. the charge chain of the same segments; every entry point that
 * writes what they read -- segment upload / reset / quench-drift, incidence, LUT, channel tables, constants -- or reads their array
 * -- ldsim_dev_light_download, ldsim_dev_light_response, ldsim_synchronize -- waits for them first; default 0),
 * "light_truth_lds" (the truth slots of ldsim_scintillation_effect / ldsim_light_detector_response / ldsim_dev_light_response, at most
 * 64 of them: 1 (default) = by light_truth_lds_kernel, a wave's 64 output rows in LDS; 0 = by light_truth_rows_kernel on slot-major
 * copies of the rows in memory, what more than 64 slots always take -- same bits for rows of distinct ids in front of their first
 * -1, and the only path that follows light_sim.py:331-335 literally for other rows is the default; the plain sum is
 * light_plain_kernel's at either value),
 * "light_universes_nu" (ldsim_dev_light_universes: weight tables that share an input go through light_plain_kernel this many at
 * a time, 1 to 4 (default 4); same bits at every value),
 * "numba_f32" (1 = the sub-expressions Numba types float32 for f4 record fields are evaluated in float, detsim.py:74-79,
 * 116-118,141,387; 0 = all-f64, what the reference computes for f8 records and what the goldens pin; default 0),
 * "mc_current" (1 = the fused chain takes its induced currents from tracks_current_mc like the reference driver does;
 * default 0 = tracks_current),
 * "debug_phases" (timing tools only, tools/phase_timing3.py: bit mask that drops phases of the tracks_current kernels;
 * results are wrong unless it is 15, the default).  An unknown name returns LDSIM_EINVAL. */
int ldsim_set_option(ldsim_ctx* ctx, const char* name, double value);
/* Per-pixel discrimination thresholds and gains of the fused chain -- the reference driver's
 * pixel_thresholds_lut[unique_pix] (cli/simulate_pixels.py:1079-1084) and pixel_gains_lut[unique_pix] (:1097-1100),
 * CudaDict lookups of util/cuda_dict.py:49-53 loaded from an .npz with keys / values / default (:82-88).
 * keys[n] are pixel ids (unique), values[n] their entries, every other pixel id gets default_value; keys outside the
 * current pixel geometry can never be looked up and are skipped.  Held as a dense table over
 * n_pixels[0]*n_pixels[1]*n_tpc ids: set the constants first, and set the tables again after a change of geometry
 * (ldsim_charge_chain returns LDSIM_ESTATE otherwise).  Without a table the chain uses DISCRIMINATION_THRESHOLD*e and
 * GAIN*mV/e.  The stage functions ldsim_get_adc_values / ldsim_digitize take their arrays from the caller as before. */
int ldsim_set_pixel_thresholds(ldsim_ctx* ctx, const int32_t* keys, const double* values, int64_t n,
                               double default_value);
int ldsim_set_pixel_gains(ldsim_ctx* ctx, const int32_t* keys, const double* values, int64_t n, double default_value);
int ldsim_clear_pixel_tables(ldsim_ctx* ctx);
int ldsim_synchronize(ldsim_ctx* ctx);

/* Random streams of the noisy stages: numba.cuda.random.create_xoroshiro128p_states(n, seed) (cli/simulate_pixels.py:
 * 92-104,396; third-party algorithm restated in csrc/rng.h -- unpinned).  State ip serves pixel row ip of
 * a get_adc_values call / of a chain launch and is advanced in place like the reference's rng_states[ip]; the table grows
 * on demand by continuing the 2^64-step jump sequence.  Needed before any call with a non-zero noise charge
 * (RESET_NOISE_CHARGE, UNCORRELATED_NOISE_CHARGE, DISCRIMINATOR_NOISE): such a call without it returns LDSIM_ESTATE. */
int ldsim_rng_seed(ldsim_ctx* ctx, uint64_t seed, int64_t n_states);
int ldsim_rng_states_download(ldsim_ctx* ctx, uint64_t* states /* [n][2] = s0, s1 */, int64_t n);
int ldsim_rng_clear(ldsim_ctx* ctx);
/* maybe_create_rng_states(n, seed, rng_states) (cli/simulate_pixels.py:92-104): no table -> n states from `seed`; a shorter
 * table -> create_xoroshiro128p_states(n - len, seed) appended; otherwise untouched.  ldsim_rng_count: states held, -1 none. */
int ldsim_rng_extend(ldsim_ctx* ctx, int64_t n_states, uint64_t seed);
int64_t ldsim_rng_count(ldsim_ctx* ctx);
/* Keyed random streams (opt-in; csrc/rng.h states the generator): every draw is Philox4x32-10 keyed by the 64-bit run seed,
 * counter (draw block, stream key lo, stream key hi, stage tag), with stream keys folded from what is simulated -- FEE row:
 * key_mix(batch key, pixel id); tracks_current_mc (pair, tick): key_mix(key_mix(key_mix(batch key, segment index within its
 * batch), pixel id), tick); light fluctuation of (det, tick): key_mix(key_mix(call key, det), tick); light noise phases:
 * seeded by the call key.  Results then do not depend on chunking, rank count or call history.
 *   ldsim_rng_keyed_seed       switches the ctx to keyed mode (drops the table); ldsim_rng_seed / ldsim_rng_clear switch back.
 *   ldsim_chain_set_batch_keys one key per batch id of the upload; a keyed chain launch whose batches have none: LDSIM_ESTATE.
 *   ldsim_rng_set_call_key     identity of the light response / trigger / noise calls that follow.
 *   ldsim_rng_keyed_normals / _uniforms: out[s*nd + j] = draw d0 + j of stream (tag, stream_keys[s]) (tests).
 * The host-array stage calls that draw (ldsim_get_adc_values with noise, ldsim_tracks_current_mc, ldsim_stat_fluctuations)
 * carry no identity for their rows and return LDSIM_ESTATE in keyed mode. */
int ldsim_rng_keyed_seed(ldsim_ctx* ctx, uint64_t seed);
int ldsim_rng_is_keyed(ldsim_ctx* ctx);
int ldsim_chain_set_batch_keys(ldsim_ctx* ctx, const uint64_t* keys, int64_t n_batches);
int ldsim_rng_set_call_key(ldsim_ctx* ctx, uint64_t key);
int ldsim_rng_keyed_normals(ldsim_ctx* ctx, uint32_t tag, const uint64_t* stream_keys, int64_t n, uint32_t d0, int32_t nd,
                            float* out);
int ldsim_rng_keyed_uniforms(ldsim_ctx* ctx, uint32_t tag, const uint64_t* stream_keys, int64_t n, uint32_t d0, int32_t nd,
                             float* out);

/* ---- (1) stage-by-stage, host buffers ---------------------------------------------------------- */
/* quenching.quench[bpg,tpb](tracks, mode)            -- reference larndsim/quenching.py:11-44 */
int ldsim_quench(ldsim_ctx* ctx, void* tracks, int64_t n, const LdsimTrackLayout* layout, int32_t mode);
/* drifting.drift[bpg,tpb](tracks)                    -- larndsim/drifting.py:11-58 */
int ldsim_drift(ldsim_ctx* ctx, void* tracks, int64_t n, const LdsimTrackLayout* layout);
/* pixels_from_track.max_pixels[bpg,tpb](tracks, n_max) -- larndsim/pixels_from_track.py:43-65 */
int ldsim_max_pixels(ldsim_ctx* ctx, const void* tracks, int64_t n, const LdsimTrackLayout* layout,
                     int64_t* n_max_pixels);
/* pixels_from_track.get_pixels[bpg,tpb](tracks, active, neigh, nrad, n_pixels_list, radius)
 *                                                     -- larndsim/pixels_from_track.py:67-109 */
int ldsim_get_pixels(ldsim_ctx* ctx, const void* tracks, int64_t n, const LdsimTrackLayout* layout,
                     int32_t radius, int32_t* active_pixels, int32_t max_active,
                     int32_t* neighboring_pixels, int32_t* neighboring_radius, int32_t max_neigh,
                     double* n_pixels_list);
/* detsim.time_intervals[bpg,tpb](track_starts, time_max, tracks) -- larndsim/detsim.py:18-40 */
int ldsim_time_intervals(ldsim_ctx* ctx, const void* tracks, int64_t n, const LdsimTrackLayout* layout,
                         double* track_starts, int64_t* time_max);
/* detsim.tracks_current[(S,P,T/64),(1,1,64)](signals, pixels, tracks, response)
 *                                                     -- larndsim/detsim.py:351-453
 * Runs the kernels the options select, exactly like ldsim_charge_chain does for its sorted pair list ("split_kernels",
 * "weights_mode", "mac_mode", "gform_max_support").  Default: the node-separable form (weights_mode 2) -- pair_setup_kernel,
 * gtables_wave_kernel (Gauss-Legendre tables X, Y, Z per pair) and gcorr_kernel (the two products on v_mfma_f64_16x16x4) -- for
 * response tables of any support (gform_max_support ticks at most, default unlimited; wider tables would be handed to round 2's
 * qweights_kernel + mac_shift kernels, weights_mode 1); pairs beyond a kernel's capacities (rules of more than quad_max_nodes
 * nodes ...) are recomputed by the monolithic closed-form kernel.  Response ticks below exp(-trim_response_log) (default 23:
 * 1e-10) of the table's largest entry are not read: an approximation relative to the reference of < 1e-10 of a waveform's peak
 * that the headline throughput on the SURVEY table relies on (bench.py reports `exact_zero_trim` beside it).  All on the dense
 * [S][P] pixel array; pixel id -1 is evaluated as the reference evaluates it (Python index wrap). */
int ldsim_tracks_current(ldsim_ctx* ctx, const void* tracks, int64_t n, const LdsimTrackLayout* layout,
                         const int32_t* pixels, int32_t max_neigh, float* signals, int32_t n_ticks);
/* detsim.tracks_current_mc[(S,P,T/64),(1,1,64)](signals, pixels, tracks, response, rng_states) -- larndsim/detsim.py:258-348,
 * what the reference driver calls (cli/simulate_pixels.py:1016).  The reference lets all tick threads of a (segment, pixel)
 * race on rng_states[itrk + ntrk*ipix]; here every (segment, pixel, tick) draws from its own stream derived from that state
 * (SplitMix64 of its words and the tick index), so the result is reproducible and statistically equivalent, not equal.
 * Needs ldsim_rng_seed; the table is grown to n * max_neigh states and each used state is stepped once afterwards. */
int ldsim_tracks_current_mc(ldsim_ctx* ctx, const void* tracks, int64_t n, const LdsimTrackLayout* layout,
                            const int32_t* pixels, int32_t max_neigh, float* signals, int32_t n_ticks);
/* detsim.get_track_pixel_map2[bpg,tpb](track_pixel_map, unique_pix, pixels, distances, max_distance)
 *                                                     -- larndsim/detsim.py:564-607 */
int ldsim_track_pixel_map(ldsim_ctx* ctx, const int32_t* unique_pix, int64_t n_unique,
                          const int32_t* pixels, const int32_t* distances, int64_t n, int32_t max_neigh,
                          int32_t max_distance, int64_t* track_pixel_map, int32_t max_tracks);
/* detsim.sum_pixel_signals[...](pixels_signals, signals, track_starts, pixel_index_map, track_pixel_map,
 *                               pixels_tracks_signals, overflow_flag) -- larndsim/detsim.py:468-527 */
int ldsim_sum_pixel_signals(ldsim_ctx* ctx, const float* signals, int64_t n, int32_t max_neigh, int32_t n_ticks,
                            const double* track_starts, const int64_t* pixel_index_map,
                            const int64_t* track_pixel_map, int32_t max_tracks, int64_t n_unique,
                            double* pixels_signals, double* pixels_tracks_signals /* may be NULL */,
                            double* overflow_flag);
/* fee.get_adc_values[bpg,tpb](pixels_signals, pixels_signals_tracks, time_ticks, adc_list, adc_ticks_list,
 *                             time_padding, rng_states, current_fractions, pixel_thresholds)
 *                                                     -- larndsim/fee.py:517-655; with non-zero noise charges rng_states = the
 *                                                        table of ldsim_rng_seed (state ip for pixel ip) */
int ldsim_get_adc_values(ldsim_ctx* ctx, const double* pixels_signals, const double* pixels_signals_tracks,
                         int64_t n_unique, int32_t n_ticks, int32_t max_tracks, const double* time_ticks,
                         int32_t n_time_ticks, double time_padding, const double* pixel_thresholds,
                         double* adc_list, double* adc_ticks_list, double* current_fractions /* may be NULL */);
/* fee.digitize(integral_list, gain)                   -- larndsim/fee.py:499-515; gain NULL = GAIN*mV/e */
int ldsim_digitize(ldsim_ctx* ctx, const double* integral_list, int64_t n, const double* gain_list, double* adcs);
/* lightLUT.calculate_light_incidence[bpg,tpb](tracks, lut, light_incidence, voxel)
 *                                                     -- larndsim/lightLUT.py:65-136
 * The three arrays are read and written: rows of segments outside every TPC, and t0_det in trigger mode 1, come back as
 * they were passed (the reference does not touch them); under option "light_lut_interp" they come back zero. */
int ldsim_light_incidence(ldsim_ctx* ctx, const void* tracks, int64_t n, const LdsimTrackLayout* layout,
                          int32_t n_out_channels, float* n_photons_det, float* t0_det, int32_t* voxel);
/* light_sim.sum_light_signals[...](segments, segment_voxel, segment_track_id, light_inc, op_channel, lut,
 *   start_time, light_sample_inc, true_track_id, true_photons, sorted_indices, t0_profile_length)
 *                                                     -- larndsim/light_sim.py:58-129 */
int ldsim_sum_light_signals(ldsim_ctx* ctx, const void* tracks, int64_t n, const LdsimTrackLayout* layout,
                            const int32_t* voxel, const int64_t* segment_track_id,
                            const float* n_photons_det, int32_t n_inc_channels,
                            const int32_t* op_channel, int32_t n_det, const int32_t* sorted_indices,
                            double start_time, int32_t n_ticks,
                            float* light_sample_inc, int64_t* true_track_id, double* true_photons,
                            int32_t max_truth);

/* Light waveform response, the two deterministic stages after the photon sum.  Arrays are [n_det][n_ticks]
 * f4 and truth slots [n_det][n_ticks][max_truth] (i8 ids, f8 photons; max_truth may be 0 with NULL pointers).  Outputs are
 * accumulated into: the caller pre-fills them like the driver does (zeros, ids -1; cli/simulate_pixels.py:1160-1162,
 * 1172-1174).  Every term is added in ascending tick order with an f4 store after it, as the reference's kernels do.
 * light_sim.calc_scintillation_effect[bpg,tpb](light_sample_inc, true_track_id, true_photons, scint, scint_true_track_id,
 *                                              scint_true_photons)        -- larndsim/light_sim.py:148-184, model :131-146 */
int ldsim_scintillation_effect(ldsim_ctx* ctx, const float* light_sample_inc, const int64_t* true_track_id,
                               const double* true_photons, int32_t n_det, int32_t n_ticks, int32_t max_truth,
                               float* scint, int64_t* scint_true_track_id, double* scint_true_photons);
/* light_sim.calc_light_detector_response[bpg,tpb](light_sample_inc, true_track_id, true_photons, light_response,
 *                                                 response_true_track_id, response_true_photons)
 *                                                                         -- larndsim/light_sim.py:303-337, model :274-300
 * light_gain[n_det] is LIGHT_GAIN indexed by array ROW like the reference (:320); impulse_model[n_impulse] is IMPULSE_MODEL,
 * read when sipm_response_model == 1.  The truth part keeps the reference's slot test on the input ids at [idet, itick]. */
int ldsim_light_detector_response(ldsim_ctx* ctx, const float* light_sample_inc, const int64_t* true_track_id,
                                  const double* true_photons, int32_t n_det, int32_t n_ticks, int32_t max_truth,
                                  const double* light_gain, const double* impulse_model, int32_t n_impulse,
                                  float* response, int64_t* response_true_track_id, double* response_true_photons);

/* Second half of the light chain: Poisson fluctuations, triggers, detector noise, digitised waveforms.
 * light_sim.calc_stat_fluctuations[bpg,tpb](light_sample_inc, light_sample_inc_disc, rng_states)
 *                                                                         -- larndsim/light_sim.py:186-238
 * Element (idet, itick) draws from state idet*n_ticks + itick of the ldsim_rng_seed table (advanced in place): one float32
 * uniform for a mean below 30 PE per tick, one float32 normal above.  The generator is third-party and unpinned. */
int ldsim_stat_fluctuations(ldsim_ctx* ctx, const float* light_sample_inc, int32_t n_det, int32_t n_ticks,
                            float* light_sample_inc_disc);

/* ---- SiPM correlated noise in the fluctuation stage (DESIGN.md "SiPM correlated noise") --------------------------------------
 * Mirrors nothing in the reference, whose only statistical model of the light leg is the Poisson draw above.  Opt-in, off by
 * default; keyed mode only.  While enabled, the fluctuation stage of ldsim_dev_light_response and ldsim_dev_light_universes (and
 * ldsim_sipm_stat_fluctuations below) counts avalanches per element (idet, itick) of the rate array x [PE / us], with
 * tick = LIGHT_TICK_SIZE and the element's keyed stream (stage tag 2, key_mix(key_mix(call key, idet), itick)); "Poisson(m, i)" is
 * the sampler above on draw i (m <= 0: 0; m < 30: inversion on uniform i; else (long long)(normal i * sqrt(m) + m) clamped at 0):
 *   n_p = Poisson(x * tick, 0)                                   primaries: the draw of the stage with the noise off
 *   n_d = Poisson(dark_rate * tick, 1)                           dark counts, also where x <= 0
 *   g_0 = n_p + n_d, g_{k+1} = Poisson(crosstalk * g_k, 2 + k)   prompt cross-talk by generations, until g_k = 0 or k = 31
 *   N = sum of g_k
 *   n_ap = Binomial(N, afterpulse)                               the charge statistics' sampler on normal 34 and uniform 35
 *   after-pulse j lands on tick itick + 1 + floor(-afterpulse_tau * log((double)u_j) / tick), u_j = uniform 64 + j (f64); it has
 *   full amplitude, starts no cross-talk and no after-pulse, and is dropped at or beyond n_ticks (it never reaches the next row)
 *   count[idet][t] = N of the element + the after-pulses that landed on it (int32)
 *   out = (float)(1 / tick * (double)count)
 * With the four constants 0 the output equals the plain keyed stage's bit for bit.  Dark counts exist only inside the tick window
 * of a fluctuated array; truth slots are untouched.
 * Ranges (LDSIM_EINVAL, the message names the field; a refused call changes nothing): 0 <= crosstalk <= 0.5,
 * 0 <= afterpulse <= 0.5, afterpulse_tau finite and > 0 when afterpulse > 0, dark_rate finite, >= 0 and dark_rate * tick < 30.
 * The values are kept when enable = 0 (noise may then be NULL).  A fluctuation while enabled outside keyed mode: LDSIM_ESTATE. */
typedef struct {
  double crosstalk;        /* mean number of secondary avalanches per avalanche */
  double afterpulse;       /* probability of one after-pulse per avalanche */
  double afterpulse_tau;   /* [us] mean delay of an after-pulse */
  double dark_rate;        /* [avalanches / us] per detector row */
} LdsimSipmNoise;
int ldsim_set_sipm_noise(ldsim_ctx* ctx, int32_t enable, const LdsimSipmNoise* noise);
int ldsim_get_sipm_noise(ldsim_ctx* ctx, int32_t* enable, LdsimSipmNoise* noise);
/* The fluctuation stage on a host array under the current call key (ldsim_rng_set_call_key): rate, out [n_det][n_ticks] f4; rows
 * are keyed by their index in this call.  Keyed mode only (LDSIM_ESTATE).  With the noise enabled, counts (or NULL) receives the
 * int32 avalanche counts; with it disabled the plain keyed stage runs and counts must be NULL (LDSIM_ESTATE). */
int ldsim_sipm_stat_fluctuations(ldsim_ctx* ctx, const float* rate, int32_t n_det, int32_t n_ticks, float* out,
                                 int32_t* counts);
/* light_sim.get_triggers(signal, group_threshold, op_channel_idx, i_subbatch), LIGHT_TRIG_MODE 0 branch
 *                                                                         -- larndsim/light_sim.py:339-411
 * signal [n_det][n_ticks] f4 (NULL: the resident response of ldsim_dev_light_response), group_threshold [n_grp] with
 * n_det = n_grp * OP_CHANNEL_PER_TRIG; row_module [n_det] = index (0..n_mod-1, ascending module id) of the module whose
 * channels contain the row's optical channel, -1 for none.  Returns the trigger ticks module by module in the order the
 * reference appends them, with the reference's bookkeeping of the re-sliced mask (:404-411).  LDSIM_ENOSPC with *n_trig =
 * the number found when `capacity` is too small.  (LIGHT_TRIG_MODE 1 is one trigger at tick 0 and needs no call.) */
int ldsim_light_triggers(ldsim_ctx* ctx, const float* signal, int32_t n_det, int32_t n_ticks, const double* group_threshold,
                         int32_t n_grp, const int32_t* row_module, int32_t n_mod, int64_t* trigger_idx,
                         int32_t* trigger_module, int64_t capacity, int64_t* n_trig);
/* light_sim.gen_light_detector_noise(shape, light_det_noise)              -- larndsim/light_sim.py:445-478
 * spectrum [n_rows][nbins] (the rows light_det_noise[...] selects), noise [n_rows][n_samples] f8.  phases [n_rows]
 * [n_samples/2+1] = the uniform numbers of :465, or NULL to draw them from a counter hash seeded by ldsim_rng_seed (the
 * reference draws them from cupy's global generator: unpinned by construction).  n_samples < 2 is refused (NaN there). */
int ldsim_light_detector_noise(ldsim_ctx* ctx, int32_t n_rows, int32_t n_samples, const double* spectrum, int32_t nbins,
                               const double* phases, double* noise);
/* light_sim.sim_triggers(bpg, tpb, signal, signal_op_channel_idx, signal_true_track_id, signal_true_photons, trigger_idx,
 *                        op_channel_idx, digit_samples, light_det_noise) incl. digitize_signal
 *                                                                         -- larndsim/light_sim.py:480-619
 * signal [n_det][n_ticks] f4 with truth [n_det][n_ticks][max_truth] (signal NULL: the resident response and its truth);
 * trigger_op_channel_idx [n_trig][n_det_trig]; light_det_noise [n_noise_channels][n_noise_bins] indexed by optical channel
 * (NULL or all zero: no noise).  phases_signal [n_det][Tp/2+1] / phases_missing [n_missing][Tp/2+1] (Tp = padded length)
 * stand for the two cp.random.uniform calls, NULL = counter hash.  Outputs digit_signal [n_trig][n_det_trig][digit_samples]
 * f8 (rounded to the digitiser's LSB), truth ids (i8, -1) / photons (f8) [..][max_truth].  The padded copies of the
 * reference are not materialised; an f4 signal that needs no padding keeps its f4 rounding when the noise is added. */
int ldsim_sim_triggers(ldsim_ctx* ctx, const float* signal, const int32_t* signal_op_channel_idx, int32_t n_det,
                       int32_t n_ticks, const int64_t* signal_true_track_id, const double* signal_true_photons,
                       int32_t max_truth, const int64_t* trigger_idx, int32_t n_trig,
                       const int32_t* trigger_op_channel_idx, int32_t n_det_trig, int32_t digit_samples,
                       const double* light_det_noise, int32_t n_noise_channels, int32_t n_noise_bins,
                       const double* phases_signal, const double* phases_missing, double* digit_signal,
                       int64_t* digit_true_track_id, double* digit_true_photons);

/* ---- (2) device-resident chain ---------------------------------------------------------------------- */
/* Upload `n` records (H2D) and unpack them into the ctx's SoA segment store.  `batch_id[i]` is the
 * reference's (event, TPC-group, sub-batch) batch of segment i (cli/simulate_pixels.py:864,902);
 * segments of one batch must be contiguous and batch ids non-decreasing; batch_id < 0 = not simulated. */
int ldsim_segments_upload(ldsim_ctx* ctx, const void* tracks, int64_t n, const LdsimTrackLayout* layout,
                          const int32_t* batch_id);
/* Write the mutated fields (n_electrons, n_photons, pixel_plane, long_diff, tran_diff, t, t_start, t_end)
 * back into host records (D2H). */
int ldsim_segments_download(ldsim_ctx* ctx, void* tracks, int64_t n, const LdsimTrackLayout* layout);
/* Re-unpack the uploaded (device-resident) records into the SoA store, discarding what quench/drift wrote:
 * lets a caller re-run the path on the same resident input without another H2D copy. */
int ldsim_segments_reset(ldsim_ctx* ctx);
/* quench + drift over the resident segments (cli/simulate_pixels.py:732,742) */
int ldsim_dev_quench_drift(ldsim_ctx* ctx, int32_t mode);

/* ---- drift-field maps ------------------------------------------------------------------------
 * A regular grid per TPC in the simulation frame (TPC_BORDERS after swap_coordinates, cm; z = drift coordinate), keyed by
 * the global TPC index so it survives ldsim_set_consts.  Channels, each C-order [nx][ny][nz] and each may be NULL:
 *   E       local field (kV/cm, finite, > 0) replacing e_field in the recombination (NULL: the constants' e_field);
 *   dx, dy  displacement of the charge that starts at a node where it reaches the anode (cm, finite; NULL: 0);
 *   dz      shift of the equivalent drift coordinate: arrival time |z + dz - z_anode| / v_drift (cm, finite; NULL: 0).
 * Node (i, j, k) sits at origin + (i, j, k) * spacing; the map is interpolated trilinearly, clamped to the edge nodes.
 * While any map is set, ldsim_dev_quench_drift quenches with E at the true midpoint and drifts the anode view -- start, end
 * and midpoint moved by the offsets at themselves, clamped into the TPC's box (never further out than the true point) and
 * rounded to the record's dtype; every charge stage of ldsim_charge_chain reads that view, the light leg and
 * ldsim_segments_download keep the true positions.  ldsim_charge_chain refuses (LDSIM_ESTATE) when the maps changed since
 * the last quench_drift; the host-array stage calls that take records (ldsim_quench, ldsim_drift, ldsim_get_pixels,
 * ldsim_tracks_current, ...) refuse while a map is set.  Validation failures: LDSIM_EINVAL (tpc outside [0, n_tpc), a
 * dimension < 2, spacing not finite and > 0, E not finite and > 0, an offset not finite). */
int ldsim_set_field_map(ldsim_ctx* ctx, int32_t tpc, const int64_t shape[3], const double origin[3], const double spacing[3],
                        const double* E, const double* dx, const double* dy, const double* dz);
int ldsim_clear_field_maps(ldsim_ctx* ctx);
/* test export: the anode view of the resident segments after a mapped quench_drift, out[k * n + i] for k = the nine
 * position fields in enum order (x_start, y_start, z_start, x_end, y_end, z_end, x, y, z) */
int ldsim_dev_anode_view_download(ldsim_ctx* ctx, double* out);

/* ---- charge statistics -----------------------------------------------------------------------
 * Opt-in, off by default: while enabled, ldsim_dev_quench_drift counts charge instead of writing mean values.  Per
 * simulated segment (batch id >= 0), in f64:
 *   N_i = max(0, rint(dE / W_ion + sqrt(fano * dE / W_ion) * z0))       ion pairs (fano = 0: rint(dE / W_ion) exactly)
 *   n_q ~ Binomial(N_i, R)                                              R = the Box / Birks factor (at the local field
 *                                                                       under a field map), clamped to [0, 1]
 *   n_photons = (dE / W_ph - n_q) * scint_prescale
 *   n_electrons ~ Binomial(n_q, exp(-t_drift / lifetime)) inside a TPC, n_q outside every TPC
 * Binomial(n, p): with pm = min(p, 1 - p), n * pm >= 30 draws clamp(rint(n p + sqrt(n p (1 - p)) z), 0, n) from one normal;
 * below, inversion on the minority outcome at u - 2^-25 of one uniform, the walk stopping at min(n, 256).  Every other drift
 * output is what it is with the mode off; segments with batch id < 0 and a NaN recombination (LDSIM_EINVAL, as with the mode
 * off) keep the mean values.  Draws: keyed stream (stage tag 5, key_mix(batch key, index of the segment within its batch)),
 * draw 0 = Fano normal, 1 / 2 = recombination normal / uniform, 3 / 4 = attachment normal / uniform, whichever branch is
 * taken -- the same charge at any chunking or rank count.
 * State rules: ldsim_dev_quench_drift returns LDSIM_ESTATE unless the ctx is in keyed mode (ldsim_rng_keyed_seed) and
 * ldsim_chain_set_batch_keys covers every batch id of the upload; the host-array stage calls that take records refuse
 * (LDSIM_ESTATE) while the mode is enabled, as under a field map; ldsim_charge_chain refuses (LDSIM_ESTATE) when the setting
 * differs from the one of the last ldsim_dev_quench_drift.  fano must be finite and >= 0 (LDSIM_EINVAL); it is kept when
 * enable = 0. */
int ldsim_set_charge_statistics(ldsim_ctx* ctx, int32_t enable, double fano);
int ldsim_get_charge_statistics(ldsim_ctx* ctx, int32_t* enable, double* fano);

typedef struct {
  int64_t n_segments;      /* segments simulated in this call */
  int64_t n_pairs;         /* (segment, pixel) pairs with a valid pixel id */
  int64_t n_unique;        /* unique (batch, pixel) rows produced */
  int64_t n_batches;
  int64_t n_overflow;      /* pixels with more than max_tracks_per_pixel contributing segments */
  int32_t max_active, max_neigh, max_length;
  int32_t n_ambiguous;     /* z slices whose response shift sat within 1e-7 of a rounding boundary */
  int64_t n_dfma;          /* f64 FMAs issued by the induced-current correlation loop (lanes x instructions) */
  int64_t n_fallback;      /* pairs recomputed by the monolithic kernel (split-path capacity overflow) */
  int64_t n_samples;       /* charge samples that passed the bound and were evaluated (2 erf + exp each) */
  int64_t n_wbuf;          /* f64 entries of the weight arena used by the split path in this call */
  int64_t n_dfma_useful;   /* of n_dfma, the FMAs of the quadrature path that are neither padding of an 8-shift weight block
                              nor ticks outside the pair's window: sum over pairs of (weights kept) x (window ticks); 0 when
                              another weights stage ran */
} LdsimChainStats;

/* counters of the last ldsim_tracks_current call (n_segments, n_pairs = S * P, n_fallback, n_wbuf, n_samples, n_dfma,
 * n_dfma_useful, n_ambiguous; the rest 0): which kernels carried the pairs -- n_wbuf > 0 means the split path's weights
 * stage ran, n_fallback counts the pairs the monolithic kernel recomputed */
int ldsim_tracks_current_stats(ldsim_ctx* ctx, LdsimChainStats* stats);

/* Slots of the census below.  Every count but the first three is over the pairs the node-separable form emitted itself
 * (tables built, not flagged for the monolithic kernel). */
enum {
  LDSIM_GC_PAIRS = 0,      /* pairs of the launch */
  LDSIM_GC_TABLES,         /* pairs with tables (status 1), flagged ones included */
  LDSIM_GC_FLAGGED,        /* pairs flagged for the monolithic kernel */
  LDSIM_GC_EMITTED,        /* pairs with tables that are not flagged */
  LDSIM_GC_T_WAVE,         /* tables kernel: gtables_wave_kernel<M, 55> */
  LDSIM_GC_T_WIDE,         /*                its wide instantiation <M, 81> */
  LDSIM_GC_T_WG,           /*                the workgroup gtables_kernel<M>, for any of the four reasons below */
  LDSIM_GC_WG_SHIFTS,      /*   more than 256 response shifts */
  LDSIM_GC_WG_BINS,        /*   more than 80 X | Y bins */
  LDSIM_GC_WG_SLICES,      /*   neither: more than 64 slices (or a sample count the wave kernel's maps do not cover) */
  LDSIM_GC_WG_FORCED,      /*   a pair the wave kernels take, under option gform_wave_tables 0 */
  LDSIM_GC_NB1,            /* node batches: 1 */
  LDSIM_GC_NB2,            /*               2 */
  LDSIM_GC_NB3P,           /*               3 or more */
  LDSIM_GC_ROWS4,          /* node rows of the last batch: 4 */
  LDSIM_GC_ROWS8,
  LDSIM_GC_ROWS12,
  LDSIM_GC_ROWS16,
  LDSIM_GC_CLS0,           /* LDS class of the correlation: 0 (the launch over all pairs) */
  LDSIM_GC_CLS1,           /*                               1 (listed) */
  LDSIM_GC_CLS2,           /*                               2 (listed) */
  LDSIM_GC_CLS0_ZREC,      /* of that class, the pairs whose Z table the correlation reads from the record (z_lds false) */
  LDSIM_GC_CLS1_ZREC,
  LDSIM_GC_CLS2_ZREC,
  LDSIM_GC_NU_OVER_CAP,    /* more response shifts than the LDS copy of Z holds (NU > 128) */
  LDSIM_GC_EMASK0,         /* window-edge columns: bit 0 of emask set */
  LDSIM_GC_EMASK1,
  LDSIM_GC_EMASK2,
  LDSIM_GC_M,              /* launch scalars: TIME_SAMPLING / RESPONSE_SAMPLING */
  LDSIM_GC_TT,             /*   ticks per tile */
  LDSIM_GC_QB0,            /*   1 = the launch over all pairs ran the 4-node-block instance of gcorr_kernel, 0 = the 16-node product */
  LDSIM_GC_QB12,           /*   the same for the listed launches */
  LDSIM_GFORM_CENSUS_N
};
/* Test seam.  Which code paths the pairs of the last ldsim_tracks_current / ldsim_charge_chain call took in the node-separable
 * form (weights_mode 2): counts[LDSIM_GFORM_CENSUS_N] int64, n >= LDSIM_GFORM_CENSUS_N.  With n >= LDSIM_GFORM_CENSUS_N + pairs
 * of the launch, counts[LDSIM_GFORM_CENSUS_N + p] is in addition the set of slots pair p was counted in (bit s = slot s; slots
 * 0 and 28.. are never set), so that a caller can tell WHICH pairs a slot held.  Counted on the host from the launch's own
 * per-pair records with the functions the launch dealt the pairs by.  LDSIM_ESTATE if the last current stage did not run
 * that form, or its records are gone. */
int ldsim_debug_gform_census(ldsim_ctx* ctx, int64_t* counts, int32_t n);
/* Test seam.  The fused correlation launches (gcorr_fused_kernel<1>, <2>: a short second node batch in the first batch's pass)
 * of the same call: out[0] = pairs of the launch, out[1], out[2] = pairs the two fused kernels were launched over; with
 * n >= 3 + 4 pairs, for pair p at out[3 + 4 p]: its mark (1, 2 = the fused kernel that took it, 0 = none), and for a pair of two
 * node batches with tables the cells listed by the first batch alone, by the second batch alone and by both (read back from the
 * launch's records; zeros for other pairs).  LDSIM_ESTATE if the last current stage did not run that form, its records are
 * gone, or the marks and the launched counts disagree. */
int ldsim_debug_gform_fused(ldsim_ctx* ctx, int64_t* out, int32_t n);

/* Fused a5-a16 (max_pixels .. digitize) on resident segments [seg_begin, seg_end):
 * per unique (batch, pixel), sorted by batch then pixel id exactly like the reference's concatenated
 * per-batch `unique_pix`.  Results stay in HBM; fetch with ldsim_chain_download(). */
int ldsim_charge_chain(ldsim_ctx* ctx, int64_t seg_begin, int64_t seg_end, int32_t want_fractions,
                       LdsimChainStats* stats);
/* Copy the last chain call's rows [0, n_unique) to host.  Any pointer may be NULL.
 *   unique_pix i32[U], batch i32[U], adc_list f64[U][A] (integrated charge), adc_ticks f64[U][A],
 *   adc_digit f64[U][A] (fee.digitize), track_pixel_map i64[U][M] (segment index within the batch, -1 pad),
 *   current_fractions f64[U][A][M] (only if want_fractions). */
int ldsim_chain_download(ldsim_ctx* ctx, int64_t capacity, int32_t* unique_pix, int32_t* batch,
                         double* adc_list, double* adc_ticks, double* adc_digit,
                         int64_t* track_pixel_map, double* current_fractions);
/* The same rows on a second HIP stream, returning at once: the next ldsim_charge_chain computes, into the other of two sets
 * of output buffers, while these rows cross PCIe (the copy engines run beside the kernels).  The host buffers must be
 * page-locked (ldsim_host_alloc) for the copy to be asynchronous, and hold the rows after ldsim_chain_download_wait.  One
 * download is in flight at a time (a second call waits for the first); a launch that would overwrite rows still being
 * copied waits for that copy.  Replaces nothing in the reference (its driver copies with cupy .get() after every batch). */
int ldsim_chain_download_async(ldsim_ctx* ctx, int64_t capacity, int32_t* unique_pix, int32_t* batch, double* adc_list,
                               double* adc_ticks, double* adc_digit, int64_t* track_pixel_map, double* fractions);
int ldsim_chain_download_wait(ldsim_ctx* ctx);
/* The same results in compact form: what the exporter reads (fee.export_to_hdf5, fee.py:143-344: the pixels that hold a hit, their
 * slots up to the first ADC at the pedestal, the fractions of the track slots the pixel has) gathered in HBM, a few MB instead of
 * the dense arrays' 13 KB per unique pixel.  ldsim_chain_compact_build: sizes[4] = hit pixels, hits, track entries (sum over
 * hit pixels of their filled track_pixel_map slots), fraction entries (sum over hits of their pixel's track slots; 0 without
 * want_fractions).  ldsim_chain_compact_download: hit_pixels [n_hp][5] i32 = {row in the dense arrays, pixel id, batch, hits,
 * track slots + 256 if the pixel is the first row of its batch in the dense arrays}, hit pixels in row order; track_segments i64, the filled track_pixel_map entries pixel after pixel; hit_rows
 * [n_hits] 24-byte rows {batch i32, pixel i32, ADC code i32, slot i32, tick f64} and hit_charge f64 (adc_list) in the same
 * order (pixel after pixel, slot 0 up); fractions f64: per hit, one value per track slot of its pixel.  Any pointer may be NULL. */
int ldsim_chain_compact_build(ldsim_ctx* ctx, int64_t* sizes);
int ldsim_chain_compact_download(ldsim_ctx* ctx, int32_t* hit_pixels, int64_t* track_segments, void* hit_rows,
                                 double* hit_charge, double* fractions);
/* Device pointers of the last chain call's compact hit list (for a collective without a host round trip):
 * hits are (batch i32, pixel i32, adc u8-as-i32, tick f64) rows for every written ADC slot. */
int ldsim_chain_compact_hits(ldsim_ctx* ctx, void** dev_rows, int64_t* n_rows, int32_t* row_bytes);

/* ---- pixel charge truth: induced charge per pixel and per (pixel, track) of the last chain launch ---------------------
 * Mirrors nothing in the reference, whose output ends in hits: it keeps neither the charge that never triggered, nor the
 * pixels without a hit, nor the absolute charge a segment put on a pixel (its backtracking fractions are normalised per
 * hit).  One reduction pass over what the launch left in HBM -- the per-pair current rows and the set-up record of the sum
 * sum_pixel_signals stands for (detsim.py:468-527) -- per unique-pixel row u of ldsim_chain_download, in the unit of
 * adc_list (electrons), dt = time_sampling:
 *   q_track[u][k]  dt * sum_t wf_k[t], k < the pixel's filled track_pixel_map slots (the others 0): the f32 current row of
 *                  slot k over exactly the ticks the pixel sum takes from it (its written window on the pixel's time axis,
 *                  clipped to [0, N_t)), accumulated in f64
 *   q_induced[u]   dt * sum_t S[t], S the pixel's summed waveform as the FEE kernel forms it (f64, slots added in slot order)
 *   q_abs[u]       dt * sum_t |S[t]|: a pixel that only saw induction has q_induced ~ 0 and q_abs > 0
 *   n_hits[u], q_hits[u] = sum_{h < n_hits} adc_list[u][h], read from the launch's own results: with FEE noise on, q_hits
 *                  includes the noise charges the hits were read out with; the three values above never do.
 * ldsim_chain_pixel_truth runs the pass and a selection on the device: a pixel is kept when n_hits > 0 or
 * q_abs >= min_abs_charge (electrons; 0 keeps every unique pixel).  sizes[2] = kept pixels, track entries (one per filled
 * slot of a kept pixel); one synchronisation.  A launch without unique pixels gives sizes 0, 0.
 * ldsim_chain_pixel_truth_download: the compact form, pixel rows in row order and track entries pixel after pixel, slot 0
 * up; either pointer may be NULL.  ldsim_chain_pixel_truth_dense_download: the dense arrays of the last pass, U = the
 * launch's n_unique, q_track [U][M] with M = MAX_TRACKS_PER_PIXEL; any pointer may be NULL.
 * State rules: the pass reads scratch buffers the library reuses, so it returns LDSIM_ESTATE, with a message naming the
 * call, once anything may have rewritten them since the launch: ldsim_segments_upload, ldsim_segments_reset,
 * ldsim_dev_quench_drift, any host-array stage call, ldsim_set_consts with other constants, a later ldsim_charge_chain that
 * failed.  The downloads return LDSIM_ESTATE unless the pass has run for the last chain launch.
 * ldsim_chain_pixel_truth_row_samples (timing tools): the current samples q_track sums over all pixels of the last launch,
 * counted on the device from the same record under the same state rule; the bytes the pass reads from the current rows
 * are four times that. */
typedef struct LdsimPixelTruthRow {
  int32_t row;          /* u: index in the arrays of ldsim_chain_download */
  int32_t pixel_id;
  int32_t batch;
  int32_t n_hits;
  int32_t n_tracks;     /* filled track_pixel_map slots = the pixel's track entries */
  int32_t pad;
  double q_hits, q_induced, q_abs;
} LdsimPixelTruthRow;
typedef struct LdsimPixelTruthTrack {
  int64_t segment;      /* segment index within the batch, as in track_pixel_map */
  double q;             /* q_track */
} LdsimPixelTruthTrack;
int ldsim_chain_pixel_truth(ldsim_ctx* ctx, double min_abs_charge, int64_t sizes[2]);
int ldsim_chain_pixel_truth_download(ldsim_ctx* ctx, LdsimPixelTruthRow* pixel_rows, LdsimPixelTruthTrack* track_entries);
int ldsim_chain_pixel_truth_dense_download(ldsim_ctx* ctx, int64_t U, double* q_induced, double* q_abs, double* q_track);
int ldsim_chain_pixel_truth_row_samples(ldsim_ctx* ctx, int64_t* n_samples);

/* ---- pixel current waveforms: the summed induced current of every pixel of the last chain launch, zero-suppressed ------
 * Mirrors nothing in the reference.  Per unique-pixel row u of ldsim_chain_download, on the pixel's time axis [0, N_t)
 * (tick t = the time t * time_sampling on the axis adc_ticks_list uses; N_t = n_time_ticks):
 *   S[t]     f64: the f32 current rows of the pixel's slots added in slot order, each over its written window placed at
 *            the slot's start tick and clipped to [0, N_t) -- the sum the FEE kernel and pixel truth form, so
 *            time_sampling * sum_t S[t] = q_induced.  No FEE noise, ever; 0 outside every window; a pixel with more pairs
 *            than slots is summed over its slots only.
 *   active   A = { t : |S[t]| > min_abs_current }, strict, in f64, on the unrounded S (0: the ticks with S != 0)
 *            (the samples returned are rounded to f32: a threshold equal to a returned sample excludes that tick only
 *            when its S is exactly an f32, a sum of one slot)
 *   kept     K = { t in [0, N_t) : some a in A has |t - a| <= pad_ticks }, 0 <= pad_ticks <= 64
 *   spans    the maximal runs of consecutive ticks of K (padded neighbourhoods that overlap or touch are one span; a span
 *            clipped at tick 0 or N_t - 1 is shorter); samples: (float)S[t] of a span's ticks in rising t
 * ldsim_chain_pixel_waveforms runs a count pass, two 64-bit scans and a fill pass on the device.  hits_only != 0: only
 * pixels with n_hits > 0 (the launch's own hit counts) produce spans.  sizes[3] = spans, samples, N_t; one synchronisation.
 * A launch without unique pixels gives 0, 0, N_t.  Span rows are ordered by (row, t_begin) and the samples of all spans are
 * concatenated in that order: no atomics decide a position.  Sample offsets are 64-bit throughout; the only limit is the
 * device memory the result needs (32 bytes per span + 4 per sample), and a result that does not fit returns LDSIM_ENOMEM
 * before anything of it is written.
 * ldsim_chain_pixel_waveforms_download: the compact form of the last pass; either pointer may be NULL.
 * ldsim_chain_pixel_waveforms_ms (timing tools): HIP-event times of the last pass's count kernel and fill kernel (0 for a
 * kernel that was not launched); it synchronises; either pointer may be NULL; LDSIM_ESTATE like the download.
 * ldsim_chain_pixel_waveforms_dense (tests, debugging): (float)S[t] of the rows [u_begin, u_end), zeros included, formed by
 * the device code the spans are formed by; S holds [u_end - u_begin][N_t] values.
 * Errors: LDSIM_EINVAL for a negative or non-finite min_abs_current, pad_ticks outside [0, 64], rows that are no range of
 * [0, n_unique].  State rules: those of pixel truth -- LDSIM_ESTATE, the message naming the call, once anything may have
 * rewritten the launch's buffers; the download returns LDSIM_ESTATE unless the pass ran for the last chain launch.  The pass
 * owns its buffers: it and ldsim_chain_pixel_truth may run for one launch in either order, any number of times. */
typedef struct LdsimPixelWaveSpan {   /* 32 bytes */
  int32_t row;          /* u: index in the arrays of ldsim_chain_download */
  int32_t pixel_id;
  int32_t batch;
  int32_t t_begin;      /* first tick */
  int32_t n_samples;
  int32_t pad;
  int64_t sample_begin; /* index of its first sample in the samples array */
} LdsimPixelWaveSpan;
int ldsim_chain_pixel_waveforms(ldsim_ctx* ctx, double min_abs_current, int32_t pad_ticks, int32_t hits_only,
                                int64_t sizes[3]);
int ldsim_chain_pixel_waveforms_download(ldsim_ctx* ctx, LdsimPixelWaveSpan* spans, float* samples);
int ldsim_chain_pixel_waveforms_dense(ldsim_ctx* ctx, int64_t u_begin, int64_t u_end, float* S);
int ldsim_chain_pixel_waveforms_ms(ldsim_ctx* ctx, double* count_ms, double* fill_ms);

/* ---- FEE universes: the last chain launch digitised again under varied front-end constants ------------------------------
 * Mirrors nothing in the reference, where a variation of a front-end constant is another run.  A launch spends its time on
 * the per-pair current rows; the LArPix front end (fee.py:499-655) only reads them.  This pass forms every unique pixel's
 * summed waveform S[t] once more from those rows and the launch's set-up record (the sum of pixel current waveforms above)
 * and runs the launch's own trigger scan and digitisation on it once per universe: universe k of the result is, bit for
 * bit, what ldsim_charge_chain gives after ldsim_set_consts with the universe's fifteen values (same seed, same batch keys).
 * A variation holds absolute values, not deltas; ldsim_fee_variation_nominal fills one from the context's constants (scales
 * 1, offset 0).  With pixel tables set (ldsim_set_pixel_thresholds / ldsim_set_pixel_gains) a universe's threshold is
 * table[pixel] * threshold_table_scale + threshold_table_offset and its gain table[pixel] * gain_table_scale (each product
 * and the sum rounded on its own), and discrimination_threshold / gain are not read, as in the launch; without tables the
 * three table fields are not read.
 * Not varied: time_sampling, n_time_ticks, max_adc_values, max_tracks_per_pixel, clock_cycle, adc_counts -- they shape the
 * record or the clock.  Not produced per universe: backtracking fractions and track_pixel_map (the map is the launch's own
 * and does not depend on the front end).
 * ldsim_chain_fee_universes runs n universes; n_hits [n] (may be NULL) receives every universe's hits.  Two synchronisations.
 * ldsim_chain_fee_universe_download: universe k's adc_list, adc_ticks, adc_digit f64 [U][A] and hit_count i32 [U] in the row
 * order of ldsim_chain_download (capacity >= U rows, else LDSIM_ENOSPC); any pointer may be NULL.
 * ldsim_chain_fee_universe_hits_download: universe k's compact rows, the 24-byte rows of ldsim_chain_compact_hits {batch i32,
 * pixel i32, ADC code i32, slot i32, tick f64}, and their charges f64 (adc_list) in the same order; either may be NULL.
 * ldsim_chain_fee_universes_ms (timing tools): HIP-event time of the last pass's scan kernel; it synchronises.
 * Errors: LDSIM_EINVAL, nothing written and an earlier result still downloadable, for n outside [1,
 * LDSIM_FEE_UNIVERSES_MAX], a non-finite field, v_ref == v_cm, a negative delay, cycle count or noise charge, a rise time
 * beyond the kernel's 62 taps (10 * buffer_risetime / time_sampling > 62, ldsim_charge_chain's own limit), pad != 0; in the
 * downloads for k outside [0, n).
 * Noise: a universe with a non-zero noise charge draws from the keyed streams of the launch's pixels (every universe of a
 * pixel sees the same normals and scales them by its own charges), so the context must be in keyed mode
 * (ldsim_rng_keyed_seed) with the launch's batch keys set (ldsim_chain_set_batch_keys): LDSIM_ESTATE otherwise.  In table
 * mode the pass never draws and never advances the table.  A universe with noise walks every tick, whatever the launch did.
 * State rules: those of pixel truth -- LDSIM_ESTATE, the message naming the call, once anything may have rewritten the
 * launch's buffers; the downloads return LDSIM_ESTATE unless the pass ran for the last chain launch.  The pass owns its
 * buffers and writes nothing of the launch (not its results, not its counters, not its tap table): it,
 * ldsim_chain_pixel_truth and ldsim_chain_pixel_waveforms may run for one launch in any order, any number of times.
 * Memory: n * U * A * 24 bytes for the dense arrays, 8 n U for the counts, 32 bytes per hit; a result that does not fit
 * returns LDSIM_ENOMEM before anything of it is written.  A launch without unique pixels returns 0 with zero counts. */
typedef struct LdsimFeeVariation {   /* 112 bytes; absolute values, not deltas */
  double discrimination_threshold, gain, v_cm, v_ref, v_pedestal, buffer_risetime;
  double reset_noise_charge, uncorrelated_noise_charge, discriminator_noise;
  double threshold_table_scale, threshold_table_offset, gain_table_scale;   /* used only when pixel tables are set */
  int32_t adc_hold_delay, adc_busy_delay, reset_cycles, pad;
} LdsimFeeVariation;
#define LDSIM_FEE_UNIVERSES_MAX 64
int ldsim_fee_variation_nominal(ldsim_ctx* ctx, LdsimFeeVariation* out);
int ldsim_chain_fee_universes(ldsim_ctx* ctx, const LdsimFeeVariation* v, int32_t n, int64_t* n_hits);
int ldsim_chain_fee_universe_download(ldsim_ctx* ctx, int32_t k, int64_t capacity, double* adc_list, double* adc_ticks,
                                      double* adc_digit, int32_t* hit_count);
int ldsim_chain_fee_universe_hits_download(ldsim_ctx* ctx, int32_t k, void* hit_rows, double* hit_charge);
int ldsim_chain_fee_universes_ms(ldsim_ctx* ctx, double* scan_ms);

/* ---- charge universes: the last chain launch re-weighted for recombination and lifetime --------------------------------
 * Mirrors nothing in the reference, where a variation of a charge constant is another run.  Charge enters the induced
 * current as one linear factor per segment, and neither the pair list nor the time windows read it, so a universe that only
 * changes how many electrons a segment delivers is the launch's rows, each times one number per segment, summed and scanned
 * again.  A charge variation holds absolute values: electron_lifetime, w_ion, box_alpha, box_beta, birks_ab, birks_kb and
 * recomb_mode (1 = box, 2 = Birks, the mode of ldsim_dev_quench_drift; a universe may switch the model).
 * Weights: for segment i of the launch's range, n_k[i] is what ldsim_dev_quench_drift would have stored in n_electrons under
 * the universe's values, by the launch's own arithmetic (recombination at the field the resident quench read -- the map's E
 * at the true midpoint when a map is set --, the column's truncating store, exp(-t_drift / lifetime) over the drift
 * coordinate the drift used, the store again); w_k[i] = n_k[i] / n_res[i] in f64, n_res the resident column.  n_res == 0:
 * weight 0, and the segment is counted (n_unweightable) when n_k != 0: its rows are zero and cannot be re-weighted.
 * Segments outside every TPC and segments with batch < 0 have no pairs: weight 1.  Under the nominal variation
 * (ldsim_charge_variation_nominal) the replay equals the resident column bit for bit and every weight is exactly 1.0.
 * Sum: S_k[t] = sum over the pixel's slots of w_k[segment of the slot] * (double)row[t], in f64 and in slot order, each
 * product rounded before it is added; windows and clipping as in the FEE universes pass.  The scan and everything behind it
 * run on S_k with universe k's FEE variation, unchanged.
 * Not varied: e_field and v_drift (they set the drift times: where the rows sit on the time axis), the diffusion constants
 * (the rows' shapes), lar_density (redundant with birks_kb and box_beta), w_ph and the light leg (n_photons is not
 * re-weighted).
 * ldsim_chain_universes: n universes, universe k with fee[k] and charge[k].  fee == NULL: the nominal FEE variation for every
 * universe.  charge == NULL: the call is exactly ldsim_chain_fee_universes(ctx, fee, n, n_hits).  The result is the universes
 * result of the launch: ldsim_chain_fee_universe_download, ldsim_chain_fee_universe_hits_download and
 * ldsim_chain_fee_universes_ms read it.  State, LDSIM_EINVAL and LDSIM_ENOMEM rules of ldsim_chain_fee_universes, and
 * nothing of the launch is written.  Validation per universe, before anything is touched, the message naming the universe
 * and the field: every field finite, electron_lifetime > 0, w_ion > 0, recomb_mode 1 or 2, pad == 0.  LDSIM_ESTATE with
 * charge variations when the resident charge has no recorded mode (ldsim_dev_quench_drift records it; ldsim_segments_upload
 * and ldsim_segments_reset forget it: segments uploaded already quenched cannot be replayed), when charge statistics are on
 * (binomial draws are not linear in the constants), or under option mc_current.  A universe whose recombination comes out
 * NaN for a segment returns LDSIM_EINVAL once the weights have been formed (the earlier result is gone by then).
 * ldsim_chain_universe_weights_download (tests, tools): universe k's weights f64 [n_segments] (n_segments = the launch's
 * range, else LDSIM_EINVAL; w may be NULL) and its count of unweightable segments; LDSIM_ESTATE when the last pass had no
 * charge variations.  ldsim_chain_universes_weights_ms: HIP-event time of the weights kernel of the last pass.
 * ldsim_chain_universe_waveforms_dense (tests, tools): f64 S_k of the rows [u_begin, u_end), S [u_end - u_begin][N_t],
 * formed by the device function the scan kernel forms it with (after a pass without charge variations: the plain sum). */
typedef struct LdsimChargeVariation {   /* 56 bytes; absolute values, not deltas */
  double electron_lifetime, w_ion, box_alpha, box_beta, birks_ab, birks_kb;
  int32_t recomb_mode, pad;
} LdsimChargeVariation;
int ldsim_charge_variation_nominal(ldsim_ctx* ctx, LdsimChargeVariation* out);
int ldsim_chain_universes(ldsim_ctx* ctx, const LdsimFeeVariation* fee, const LdsimChargeVariation* charge, int32_t n,
                          int64_t* n_hits);
int ldsim_chain_universe_weights_download(ldsim_ctx* ctx, int32_t k, double* w, int64_t n_segments, int64_t* n_unweightable);
int ldsim_chain_universes_weights_ms(ldsim_ctx* ctx, double* weights_ms);
int ldsim_chain_universe_waveforms_dense(ldsim_ctx* ctx, int32_t k, int64_t u_begin, int64_t u_end, double* S);

/* ---- device-resident light leg (cli/simulate_pixels.py:749-797 and :1120-1153 on the resident segments) ---------- */
/* lightLUT.calculate_light_incidence[bpg,tpb](tracks, lut, light_sim_dat, track_light_voxel) over ALL resident segments,
 * after ldsim_dev_quench_drift (it needs n_photons and pixel_plane): n_photons_det [n][n_out] f4, t0_det [n][n_out] f4
 * (LIGHT_TRIG_MODE 0 only) and voxel [n][3] i4 stay in HBM; segments outside every TPC hold zeros. */
int ldsim_dev_light_incidence(ldsim_ctx* ctx, int32_t n_out_channels);
/* rows [seg_begin, seg_end) of those arrays to host; any pointer may be NULL */
int ldsim_dev_light_incidence_download(ldsim_ctx* ctx, int64_t seg_begin, int64_t seg_end, float* n_photons_det,
                                       float* t0_det, int32_t* voxel);
/* inputs of light_sim.get_nticks (larndsim/light_sim.py:24-41) for the rows of one batch: min / max of t0_det over the
 * entries with n_photons_det > 0, and whether there is any (trigger mode 0) */
int ldsim_dev_light_t0_range(ldsim_ctx* ctx, int64_t seg_begin, int64_t seg_end, float* t0_min, float* t0_max,
                             int32_t* any);
/* light_sim.sum_light_signals[...] for the resident segments [seg_begin, seg_end) (one batch of the reference's loop):
 * light_sample_inc [n_det][n_ticks] f4 and, with max_truth = MAX_MC_TRUTH_IDS > 0, the truth slots [n_det][n_ticks][max_truth]
 * (i8 ids from segment_track_id[seg_end - seg_begin], f8 photons) are initialised (0 / -1) and filled in HBM.  Segments are
 * visited per detector in descending n_photons_det like the driver's argsort (cli/simulate_pixels.py:1141-1144; equal
 * values, which numpy's unstable sort leaves unpinned, by descending index).
 * Without truth slots (max_truth = 0) the call returns with its kernels in flight on the ctx's stream (every consumer --
 * ldsim_dev_light_download, ldsim_dev_light_response, ldsim_light_kernel_ms -- is ordered after them); the array is brought back to
 * zero by clearing the tick tiles the previous such sum lit when the same buffer serves again (a batch lights its own TPCs' rows
 * only), and op_channel is checked and sent again only when it differs from the last call's. */
int ldsim_dev_sum_light(ldsim_ctx* ctx, int64_t seg_begin, int64_t seg_end, const int32_t* op_channel, int32_t n_det,
                        const int64_t* segment_track_id, int32_t max_truth, double start_time, int32_t n_ticks);
/* results of the last ldsim_dev_sum_light to host; any pointer may be NULL */
int ldsim_dev_light_download(ldsim_ctx* ctx, float* light_sample_inc, int64_t* true_track_id, double* true_photons);
/* HIP-event durations of the last ldsim_dev_light_incidence launch and the last ldsim_dev_sum_light call */
int ldsim_light_kernel_ms(ldsim_ctx* ctx, double* incidence_ms, double* sum_ms);
/* calc_scintillation_effect -> calc_stat_fluctuations (fluctuate != 0; needs ldsim_rng_seed) -> calc_light_detector_response
 * on the photon sum of the last ldsim_dev_sum_light, all in HBM (cli/simulate_pixels.py:1159-1180).  light_gain [n_det] by
 * array row, impulse_model as in ldsim_light_detector_response.  ldsim_light_triggers / ldsim_sim_triggers with a NULL
 * signal then work on the result. */
int ldsim_dev_light_response(ldsim_ctx* ctx, const double* light_gain, const double* impulse_model, int32_t n_impulse,
                             int32_t fluctuate);
/* the three stages' arrays to host ([n_det][n_ticks] f4; truth of the response); any pointer may be NULL */
int ldsim_dev_light_response_download(ldsim_ctx* ctx, float* scint, float* disc, float* response,
                                      int64_t* response_true_track_id, double* response_true_photons);
/* HIP-event durations of the three stages of the last ldsim_dev_light_response */
int ldsim_light_response_ms(ldsim_ctx* ctx, double* scint_ms, double* fluct_ms, double* response_ms);

/* ---- light universes: the resident photon sum under varied light constants ---------------------------------------------------
 * Mirrors nothing in the reference, where a variation of a light constant is another run.  Everything behind
 * ldsim_dev_sum_light reads only the photon sum and a handful of constants, which enter as two host-tabulated weight tables and
 * a gain per row; a universe is another pair of tables.  A light variation holds absolute values:
 *   photon_scale        multiplies the resident photon sum (light yield, W_PH, SCINT_PRESCALE, a global efficiency); finite, > 0
 *   singlet_fraction    SINGLET_FRACTION; finite, in [0, 1]
 *   tau_s, tau_t        TAU_S, TAU_T; finite, > 0
 *   gain_scale          multiplies LIGHT_GAIN[row]; finite, != 0
 *   response_time, oscillation_period   LIGHT_RESPONSE_TIME, LIGHT_OSCILLATION_PERIOD; finite, > 0.  Under SIPM_RESPONSE_MODEL 1
 *                       they are not read, and a value that differs from the context's is refused (a knob that does nothing)
 * Universe k of the photon sum inc:  x_k = (float)((double)inc * photon_scale) (one rounding, exact at 1.0);  scint_k =
 * calc_scintillation_effect of x_k under (singlet_fraction, tau_s, tau_t), without truth slots;  disc_k =
 * calc_stat_fluctuations of scint_k under the context's current call key (fluctuate != 0), else scint_k;  resp_k =
 * calc_light_detector_response of disc_k under (response_time, oscillation_period) or the impulse model, the row gain
 * light_gain[d] * gain_scale formed once in f64.  Every array equals, bit for bit, what ldsim_dev_light_response gives on x_k
 * under those constants and the same call key; the nominal universe equals the launch's own arrays.  photon_scale acts on the
 * summed photons, not on n_photons before the f4 sums: a universe is not bit-equal to a fresh run under a changed W_PH.
 * With keyed streams the draws of element (detector, tick) depend on the call key only, so all universes see the same random
 * numbers.  Truth slots are not produced per universe.
 * ldsim_dev_light_universes: n in [1, LDSIM_LIGHT_UNIVERSES_MAX]; needs a resident photon sum (LDSIM_ESTATE), and with
 * fluctuate != 0 keyed streams (LDSIM_ESTATE: table-mode draws would advance the state table).  Every universe is validated
 * before anything is touched, the message naming the universe and the field (LDSIM_EINVAL); a refused call leaves the earlier
 * result in place.  Universes with byte-equal photon_scale share one input; within it equal (singlet_fraction, tau_s, tau_t)
 * share one scint and one disc; per disc equal (gain_scale, response_time, oscillation_period) share one response: no stage
 * runs twice on the same input with the same table, and tables that share an input go through light_plain_kernel
 * together.  resp_k stays resident for every k, scint_k and disc_k only with keep_stages != 0.  The launch's own arrays
 * (ldsim_dev_light_response), its truth arrays and the call key are left as they were.  The result is invalidated by the next
 * ldsim_dev_sum_light, ldsim_dev_light_response, ldsim_segments_upload and ldsim_segments_reset.
 * ldsim_dev_light_universe_download: any pointer may be NULL; stages that were not kept: LDSIM_ESTATE.
 * ldsim_dev_light_universe_triggers / _waveforms: ldsim_light_triggers / ldsim_sim_triggers on resp_k without truth slots.
 * ldsim_light_universes_ms: HIP-event times of the three stages summed over the last ldsim_dev_light_universes. */
#define LDSIM_LIGHT_UNIVERSES_MAX 64
typedef struct LdsimLightVariation {   /* 56 bytes; absolute values, not deltas */
  double photon_scale, singlet_fraction, tau_s, tau_t, gain_scale, response_time, oscillation_period;
} LdsimLightVariation;
int ldsim_light_variation_nominal(ldsim_ctx* ctx, LdsimLightVariation* out);
int ldsim_dev_light_universes(ldsim_ctx* ctx, const LdsimLightVariation* v, int32_t n, const double* light_gain,
                              const double* impulse_model, int32_t n_impulse, int32_t fluctuate, int32_t keep_stages);
int ldsim_dev_light_universe_download(ldsim_ctx* ctx, int32_t k, float* scint, float* disc, float* response);
int ldsim_dev_light_universe_triggers(ldsim_ctx* ctx, int32_t k, int32_t n_det, int32_t n_ticks, const double* group_threshold,
                                      int32_t n_grp, const int32_t* row_module, int32_t n_mod, int64_t* trigger_idx,
                                      int32_t* trigger_module, int64_t capacity, int64_t* n_trig);
int ldsim_dev_light_universe_waveforms(ldsim_ctx* ctx, int32_t k, const int32_t* signal_op_channel_idx, int32_t n_det,
                                       int32_t n_ticks, const int64_t* trigger_idx, int32_t n_trig,
                                       const int32_t* trigger_op_channel_idx, int32_t n_det_trig, int32_t digit_samples,
                                       const double* light_det_noise, int32_t n_noise_channels, int32_t n_noise_bins,
                                       const double* phases_signal, const double* phases_missing, double* digit_signal);
int ldsim_light_universes_ms(ldsim_ctx* ctx, double* scint_ms, double* fluct_ms, double* response_ms);

/* ---- light LUT builder: keyed photon transport in a TPC box (csrc/kernels_lutbuild.hip) --------------------------------------
 * The producer of the table ldsim_set_light_lut loads: scintillation photons walked from every voxel of a box to rectangular
 * detectors on its walls under Rayleigh scattering, bulk absorption and diffuse wall reflection.  larndsim_amd/lut_builder.py
 * restates the walk in numpy (trace_twin) and turns the tallies into the table (to_lut).
 * Frame: the box [0, box[0]] x [0, box[1]] x [0, box[2]] cm (axes u, v, w) with a grid (nx, ny, nz); voxel (i, j, k) spans
 * [i, i + 1) * box[0] / nx and likewise, linear index (i * ny + j) * nz + k.  A detector is an axis-aligned rectangle on wall
 * 0..5 = u0, u1, v0, v1, w0, w1 (u0: u = 0, u1: u = box[0]); lo / hi are in the wall's two in-plane coordinates in cyclic axis
 * order (u walls: (v, w); v walls: (w, u); w walls: (u, v)); a point belongs to it when lo <= point < hi in both.  Its index in
 * the list is the LUT's detector index.  Rectangles of one wall must not overlap.
 * All geometry is f64.  Uniforms are keyed_uniform values (csrc/rng.h; f32 in (0, 1], widened exactly) of the stream
 * (seed, stage tag 6, key_mix(key_mix(RNG_KEY_ROOT, voxel linear index), photon index)), indexed serially; an index whose
 * branch is not taken stays unused.  The seed is the call's own argument: the context need not be in keyed mode.
 * Emission: draws 0, 1, 2: p = voxel_lo + u * voxel_size, clamped into the box (emit_mode 1: the voxel's centre, the three
 * indices unused); draws 3, 4: mu = 1 - 2 u3, phi = 2 pi u4, d = (sqrt(1 - mu^2) cos phi, sqrt(1 - mu^2) sin phi, mu).
 * Step s = 0, 1, ... uses draws a, b, c, e = 5 + 4s .. 8 + 4s.  lambda_t = 1 / (1 / rayleigh + 1 / absorption);
 * l = -lambda_t ln(u_a) (inf when lambda_t is); d_wall = the smallest distance to a wall along d (never negative; on a tie the
 * lowest axis).  If l < d_wall: p += l d, path += l; with u_b <= lambda_t / absorption the photon is absorbed in the bulk, else
 * it Rayleigh-scatters: q = 4 u_c - 2, A = cbrt(q + sqrt(q^2 + 1)), mu = A - 1 / A (the exact inverse of the (1 + mu^2) law),
 * phi = 2 pi u_e, and with st = sqrt(1 - mu^2), den = sqrt(1 - d_z^2):
 *   d' = (st (d_x d_z cos phi - d_y sin phi) / den + d_x mu, st (d_y d_z cos phi + d_x sin phi) / den + d_y mu,
 *         -st cos phi den + d_z mu), or (st cos phi, st sin phi, sign(d_z) mu) where |d_z| > 0.99999; d' is renormalised.
 * Otherwise: path += d_wall, p is put on the wall; the first rectangle of that wall (lowest index) holding the point detects the
 * photon; if none does, with u_b <= wall_reflectivity[wall] it is re-emitted Lambertian about the inward normal
 * (cos theta = sqrt(u_c), phi = 2 pi u_e; the in-plane components (sin theta cos phi, sin theta sin phi) in cyclic axis order),
 * else it is absorbed at the wall.  After max_steps steps the photon is truncated.  Every photon has exactly one fate.
 * Tallies (integers, so independent of order): per (voxel, detector) count u32; hist[nprof] u32, bin min(floor(t), nprof - 1)
 * of t = path / group_velocity in ns (late photons land in the last bin); tmin = the least (float)t (+inf where count is 0);
 * tsum u64 = sum of llrint(1024 t).  Per voxel three u64 fate counters: absorbed in the bulk, absorbed at a wall, truncated;
 * sum(count) + the three == n_photons.
 * ldsim_light_lut_build fills the host arrays for the voxels [voxel_begin, voxel_end) only (counts [nv][ndet],
 * hist [nv][ndet][nprof], tmin [nv][ndet], tsum [nv][ndet], fates [nv][3]): a table can be built in slices, or on several GPUs
 * by separate processes, and concatenated -- the same integers at any slicing, any lut_build_group_photons (ldsim_set_option:
 * photons one workgroup walks, 64 .. 2^20, default 4096) and either tally path (option lut_build_lds_tile 0 sends every
 * arrival to global atomics, as happens by itself when ndet * nprof does not fit the workgroup's LDS tile).
 * ldsim_light_lut_trace writes, for photons [photon_begin, photon_end) of one voxel: fate (the detector index, or -1 absorbed
 * in the bulk, -2 absorbed at a wall, -3 truncated), the steps taken, the arrival time path / group_velocity and the end point
 * [n][3].  ldsim_light_lut_build_ms: HIP-event time of the last build's kernel.
 * LDSIM_EINVAL (with a message): ndet outside 1 .. 1024, nprof outside 1 .. 512, n_photons outside 1 .. 2^31 - 1, a zero-sized
 * box, grid or rectangle, a rectangle outside its wall or on an unknown wall, overlapping rectangles, lengths <= 0, a
 * reflectivity outside [0, 1), a range outside the grid. */
#define LDSIM_LUT_MAX_DETECTORS 1024
#define LDSIM_LUT_MAX_NPROF 512
typedef struct LdsimLutBuildParams {   /* 112 bytes */
  double box[3];                 /* offset 0: extents of the box, cm */
  double rayleigh_cm;            /* 24: Rayleigh scattering length, > 0, inf allowed */
  double absorption_cm;          /* 32: bulk absorption length, > 0, inf allowed */
  double group_velocity_cm_ns;   /* 40: 13.4 is a literature value for 128 nm in LAr */
  double wall_reflectivity[6];   /* 48: u0 u1 v0 v1 w0 w1, each in [0, 1) */
  int32_t emit_mode;             /* 96: 0 uniformly in the voxel, 1 at its centre */
  int32_t max_steps;             /* 100 */
  int32_t nprof;                 /* 104: 1 ns bins of the arrival-time histogram */
  int32_t reserved;              /* 108 */
} LdsimLutBuildParams;
typedef struct LdsimLutDetector {      /* 40 bytes */
  int32_t wall;                  /* 0..5 = u0 u1 v0 v1 w0 w1 */
  int32_t pad;
  double lo[2];
  double hi[2];
} LdsimLutDetector;
int ldsim_light_lut_build(ldsim_ctx* ctx, const LdsimLutBuildParams* params, const LdsimLutDetector* detectors, int32_t ndet,
                          int32_t nx, int32_t ny, int32_t nz, int64_t voxel_begin, int64_t voxel_end, int64_t n_photons,
                          uint64_t seed, uint32_t* counts, uint32_t* hist, float* tmin, uint64_t* tsum, uint64_t* fates);
int ldsim_light_lut_trace(ldsim_ctx* ctx, const LdsimLutBuildParams* params, const LdsimLutDetector* detectors, int32_t ndet,
                          int32_t nx, int32_t ny, int32_t nz, int64_t voxel, int64_t photon_begin, int64_t photon_end,
                          uint64_t seed, int32_t* fate, int32_t* steps, double* time, double* end);
int ldsim_light_lut_build_ms(ldsim_ctx* ctx, double* ms);

/* ---- field-response builder: pixel induction tables by Shockley-Ramo (csrc/kernels_respbuild.hip) ---------------------------
 * The producer of the table ldsim_set_response loads.  The anode is the plane z = 0; the pixel is a square pad of side pad_size
 * centred on its pitch cell, everything else in the plane is grounded, the cathode is far away, the drift field uniform: an
 * electron at transverse offset (x, y) from the pad centre moves straight down at v_drift.  The pad's weighting potential is the
 * solid angle it subtends over 2 pi:
 *   phi(x, y, z) = 1 / (2 pi) sum_{sx = -1, +1} sum_{sy = -1, +1} sx sy atan2(X Y, z sqrt(X^2 + Y^2 + z^2)),
 *   X = x + sx a, Y = y + sy a, a = pad_size / 2        (z = 0: 1 over the pad, 0 off it, 1/2 on an edge, 1/4 on a corner).
 * Tick edges m = 0 .. n_k: z_e(m) = v_drift max(0, (arrival_tick + 1/2) sampling - (m - 1/2) sampling): the charge reaches the
 * plane at the upper edge of tick arrival_tick.  phibar(i, j, m) = the sum over p = 0 .. n_sub - 1 (outer), q = 0 .. n_sub - 1
 * (inner) of phi(x, y, z_e(m)) at x = (i + (p + 1/2) / n_sub) bin_size, y = (j + (q + 1/2) / n_sub) bin_size, divided by n_sub^2;
 * table[i][j][k] = (phibar(i, j, k + 1) - phibar(i, j, k)) / sampling: the tick average of the induced current per unit charge
 * (Ramo), exact, without a derivative.  Entries after arrival_tick are exactly 0; a bin's entries sum to
 * (phibar(z = 0) - phibar(z_e(0))) / sampling.  All arithmetic is f64 in one fixed order: the same bytes at any n_i, n_j, n_k.
 * ldsim_response_build fills the host array table [n_i][n_j][n_k]; ldsim_response_build_ms: HIP-event time of the last build's
 * kernel.  The kernel keeps a row's n_k + 1 edges in the workgroup's LDS: n_k <= LDSIM_RESPONSE_BUILD_MAX_K.
 * LDSIM_EINVAL (with a message naming the entry): pad_size, bin_size, v_drift or sampling not finite and > 0, n_i, n_j or n_k < 1,
 * n_k > LDSIM_RESPONSE_BUILD_MAX_K, n_sub outside 1 .. LDSIM_RESPONSE_BUILD_MAX_NSUB, arrival_tick outside [0, n_k), more than
 * 2^31 - 1 rows. */
#define LDSIM_RESPONSE_BUILD_MAX_K 7679
#define LDSIM_RESPONSE_BUILD_MAX_NSUB 16
typedef struct LdsimResponseBuildParams {   /* 56 bytes */
  double pad_size;               /* offset 0: side of the square pad, cm */
  double bin_size;               /* 8: transverse bin of the table, cm (RESPONSE_BIN_SIZE) */
  double v_drift;                /* 16: cm / us */
  double sampling;               /* 24: tick of the table, us (RESPONSE_SAMPLING) */
  int32_t n_i, n_j, n_k;         /* 32, 36, 40: shape of the table */
  int32_t n_sub;                 /* 44: sub-samples per bin and axis */
  int32_t arrival_tick;          /* 48 */
  int32_t _pad;                  /* 52 */
} LdsimResponseBuildParams;
int ldsim_response_build(ldsim_ctx* ctx, const LdsimResponseBuildParams* params, double* table);
int ldsim_response_build_ms(ldsim_ctx* ctx, double* ms);

/* ---- drift-field map builder: space charge by a Poisson solve, drift paths (csrc/kernels_fmapbuild.hip) ----------------------
 * The producer of the maps ldsim_set_field_map loads (E, dx, dy, dz of one TPC); larndsim_amd/field_map_builder.py restates
 * the model in numpy.
 * Geometry and units.  One TPC is one box in the simulation frame (cm, z the drift coordinate).  Node grid (nx, ny, nz), every
 * dimension >= 2, node (i, j, k) at origin + (i, j, k) * spacing (hx, hy, hz) and at linear index (i ny + j) nz + k; the first
 * and last node of every axis lie on the box faces.  z_anode and z_cathode are the two z faces (TPC_BORDERS[tpc][2][0] and
 * [2][1]); n = sign(z_cathode - z_anode); q = |z - z_anode| is the drift coordinate.  kV, kV/cm, source in kV/cm^2.
 * Potential.  E = e0 n z^ - grad psi, e0 > 0 the nominal field, psi the perturbation: laplace psi = -s inside, s = rho / eps on
 * the nodes, psi given on the six faces (Dirichlet; 0 = conducting anode and cathode and an ideally graded cage, anything else
 * a cage defect).
 * Discretisation.  7-point stencil on the interior nodes,
 *   (A psi)(i, j, k) = sum over the axes a of (2 psi(c) - psi(c - e_a) - psi(c + e_a)) * (1 / h_a^2),
 * the face values moved to the right: A psi = b, A symmetric positive definite.  ldsim_field_map_solve: on entry the face nodes
 * of psi_inout hold the boundary values (its interior nodes are not read; the source's face nodes only have to be finite);
 * conjugate gradients in f64 from psi = 0 inside, ended at the first iteration count at which |r|_2 <= tol |b|_2 for the recurrence's residual, the
 * true residual b - A psi then formed and held to the same rule (missed: the iteration goes on from the true residual).
 * *iterations = the iteration count, *residual = |b - A psi|_2 / |b|_2 of what is returned (0 when b = 0).  b = 0 -- no interior
 * node included -- returns the boundary values and zeros inside with 0 iterations.  Every 2-norm is a sum over fixed chunks of
 * 256 consecutive node indices (inside a chunk: lane l of wave w holds index 64 w + l, a wave's 64 values are folded by
 * halves, 32, 16 .. 1, the four waves added in order) followed by the sum of the chunk partials (thread t adds partials t,
 * t + 256, .. in rising order, then the same fold): one fixed order, so the bytes do not depend on the number of workgroups
 * (option fmap_build_wgs; 0 = the default).  No floating-point atomics.  Missing tol within max_iters: LDSIM_ENOCONV, the
 * message states the residual reached; psi_inout is not written then.
 * Field at the nodes.  -grad psi by central differences inside; along an axis on whose face the node lies the second-order
 * one-sided formula (4 (psi_1 - psi_0) - (psi_2 - psi_0)) / (2 h) (mirrored on the upper face), with 2 nodes the two-point
 * difference.  Ex, Ey, En = e0 - n dpsi/dz,
 * |E| = sqrt(Ex^2 + Ey^2 + En^2) (|En| where Ex = Ey = 0).
 * Paths.  An electron moves with -mu(|E|, T) E,
 *   mu(E, T) = (a0 + a1 E + a2 E sqrt(E) + a3 E^2 sqrt(E)) / (1 + (a1 / a0) E + a4 E^2 + a5 E^3) / (r sqrt(r)) * 1e-3, r = T / 89
 * in cm^2 / kV / us (consts.electron_mobility), v_drift = e0 mu(e0, T).  With s = q_node - q running from 0 at the node to
 * q_node on the anode plane:  dx/ds = -Ex / En,  dy/ds = -Ey / En,  dtau/ds = v_drift / (mu(|E|) En) - 1,  tau = v_drift t - s
 * (so dx/dq = Ex / En, dt/dq = 1 / (mu En): a positive charge cloud pulls the electrons towards it).  The field at a point is the
 * trilinear interpolation of the four node values (Ex, Ey, En, |E|) in fmap_eval's order and form: u = (p - origin) * (1 / h)
 * clamped to [0, n - 1], cell min((int)u, n - 2), a + f (b - a) along z, then y, then x; z = z_anode + n q.  Classical RK4 in
 * N = max(1, ceil(q_node / step)) equal steps q_node / N, stage m + c of step m at q = q_node - (m + c) (q_node / N); a node on
 * the anode plane has a path of length 0.  En <= 0 (or not a number) at any stage: LDSIM_EINVAL "field reverses", naming the
 * lowest such node.
 * Channels, per node: E = |E| at the node; dx, dy = end point minus node; dz = n tau(q_node), so that |z + dz - z_anode| / v_drift
 * is the path's drift time; flags (u8) = 1 where the end point lies outside [origin, origin + (n - 1) h] in x or y (charge that
 * reaches the field cage; the values are kept).  s = 0 with zero boundary gives E == e0 and offsets == 0 bit for bit.
 * ldsim_field_map_trace takes psi (host, [nx][ny][nz]) and fills the five host arrays; ldsim_field_map_build_ms fills ms[3]: the
 * HIP-event times (ms) of the last solve (its kernels from the first to the last launch), of the field kernel and of the trace kernel.
 * LDSIM_EINVAL (with a message naming the entry): spacing, e0, temperature, tol or step not finite and > 0, mobility[0] not
 * finite and non-zero or another mobility parameter not finite, a dimension < 2, more than 2^31 - 1 nodes, z_anode or z_cathode
 * not finite or equal, max_iters or check_every < 1, more than LDSIM_FIELD_MAP_BUILD_MAX_STEPS steps on the longest path, a
 * non-finite source, boundary or psi value, a NULL array. */
#define LDSIM_FIELD_MAP_BUILD_MAX_STEPS 1048576
typedef struct LdsimFieldMapBuildParams {   /* 168 bytes */
  double origin[3];              /* offset 0: node (0, 0, 0), cm */
  double spacing[3];             /* 24: hx, hy, hz, cm */
  double z_anode;                /* 48 */
  double z_cathode;              /* 56 */
  double e0;                     /* 64: nominal field, kV/cm */
  double temperature;            /* 72: K */
  double mobility[6];            /* 80: a0 .. a5 (ELECTRON_MOBILITY_PARAMS) */
  double tol;                    /* 128: relative residual the solve ends at */
  double step;                   /* 136: largest RK4 step in q, cm */
  int32_t n[3];                  /* 144: nx, ny, nz */
  int32_t max_iters;             /* 156 */
  int32_t check_every;           /* 160: iterations between two reads of the residual by the host */
  int32_t _pad;                  /* 164 */
} LdsimFieldMapBuildParams;
int ldsim_field_map_solve(ldsim_ctx* ctx, const LdsimFieldMapBuildParams* params, const double* source, double* psi_inout,
                          int32_t* iterations, double* residual);
int ldsim_field_map_trace(ldsim_ctx* ctx, const LdsimFieldMapBuildParams* params, const double* psi, double* E, double* dx,
                          double* dy, double* dz, uint8_t* flags);
int ldsim_field_map_build_ms(ldsim_ctx* ctx, double* ms);

/* ---- track generator: keyed muon, pion and proton transport in LAr to segments (csrc/kernels_trackgen.hip) -------------------
 * The producer of the edep-sim `segments` the driver starts from; larndsim_amd/track_generator.py restates the walk in numpy
 * (generate_twin), makes the primaries (gun, cosmics) and turns the columns into segments / trajectories / vertices.
 * Units and frame.  cm, MeV, us; positions in the input file's frame (drift axis in x), the medium uniform LAr inside the world
 * box [world_lo, world_hi].  Particles: pdg +-13, +-211, 2212 with the masses LDSIM_TRACK_GEN_M_* and |charge| 1; a pion is a
 * muon of another mass.  No decays, hadronic interactions, bremsstrahlung or separate delta-ray tracks.
 * Kinematics at kinetic energy T of mass M (gen_kin): tau = T / M, (beta gamma)^2 = bg2 = tau (tau + 2), gamma = tau + 1,
 * beta^2 = bg2 / gamma^2, r = me / M, Tmax = 2 me bg2 / (1 + 2 gamma r + r^2).  Density effect (gen_delta), x = log10(bg2) / 2:
 * delta = 2 ln10 x - Cbar for x >= x1, + a (x1 - x)^k for x0 <= x < x1, delta0 10^(2 (x - x0)) below x0.  Rate in MeV / cm of the
 * collisions below Tc (gen_rate):  S_r(T, Tc) = K (Z/A) rho / beta^2 [ 1/2 ln(2 me bg2 Tc / I^2) - (beta^2 / 2)(1 + Tc / Tmax)
 * - delta / 2 ];  S(T) = S_r(T, Tmax) is the unrestricted Bethe mean.
 * One step (gen_step) of a particle at p, unit direction d, kinetic energy T, time t:
 *   h = max(min(step, max_loss_fraction T / S(T)), min_step); d_wall = the smallest distance to a wall along d (never negative;
 *   on a tie the lowest axis); d_wall <= h: h = d_wall and the particle leaves.  With energy_loss: Tm = max(T - S(T) h / 2, t_min)
 *   (the midpoint: the deterministic range converges with step^2); every quantity below is taken at Tm.  Tc' = min(t_cut, Tmax)
 *   with straggling, Tmax without; mean loss dE = S_r(Tm, Tc') h.  With straggling, xi = (K / 2)(Z/A) rho h / beta^2:
 *   soft: dE = max(dE + sqrt(xi Tc' (1 - beta^2 Tc' / (2 Tmax))) z0, 0);
 *   hard, where Tmax > t_cut: the count n is Poisson of mean lambda = xi [(1 / t_cut - 1 / Tmax) - (beta^2 / Tmax) ln(Tmax / t_cut)]
 *   by inversion of u' = u - 2^-25 (p = c = exp(-lambda); for k = 1 .. LDSIM_TRACK_GEN_HARD_CAP while u' > c: n = k,
 *   p = p lambda / k, c = c + p -- the count is capped at LDSIM_TRACK_GEN_HARD_CAP = 8); collision j draws
 *   T_h = 1 / (1 / t_cut - u_e (1 / t_cut - 1 / Tmax)) (the inverse of 1 / T^2 on [t_cut, Tmax]) and keeps it when
 *   u_a > beta^2 T_h / Tmax, else draws again; the LDSIM_TRACK_GEN_HARD_TRIES = 4th draw is kept whatever u_a says.  dE += T_h: a
 *   hard collision's energy is deposited in this segment.  The soft and hard means add up to S(Tm) h.
 *   The walk ends stopped when dE >= T or T - dE < t_min: dE = T, h = min(h, T / S_r(Tm, Tc')); a stopped particle does not leave.
 *   The end point is p + h d, on the wall's coordinate exactly when the particle leaves, clamped into the box always;
 *   t += h / (beta c), c = 29979.2458 cm / us; T -= dE.  With mcs, and the walk going on: theta0 = 13.6 MeV / (beta^2 E)
 *   sqrt(h / X0) max(1 + 0.038 ln(h / (X0 beta^2)), 0), E = Tm + M (beta p = beta^2 E), X0 = rad_length / density in cm; two
 *   plane angles ax = theta0 z2, ay = theta0 z3; the local direction (ax, ay, 1) / nrm = (a, b, mu) is turned into d's frame by
 *   the light LUT builder's rotation with (st cos phi, st sin phi) = (a, b) and renormalised.  Where |d_z| > 0.99999 that
 *   builder replaces d by the local vector, which is right for a photon's wide angles and wrong for milliradians (a track along
 *   z would forget every earlier deflection); here the same rotation is made about the x axis instead, on the cyclically
 *   permuted components (d_y, d_z, d_x) -> (n_y, n_z, n_x).  No lateral displacement inside a step.  After max_steps steps the walk is truncated.  With energy_loss 0 (for
 *   tests of the scattering alone) T stays, dE = 0 and a walk ends at a wall or truncated.
 * Random numbers.  Uniforms are keyed_uniform values (csrc/rng.h; f32 in (0, 1], widened exactly) of the stream (seed, stage tag
 * RNG_TAG_GEN = 7, key_mix(key_mix(RNG_KEY_ROOT, event_id), track_in_event)); the seed is the call's own argument, and a walk
 * depends on nothing else in the call.  Normals take keyed_normal's pairing of two words, sqrt(-2 ln u_a) cos(2 pi u_b) and
 * sqrt(-2 ln u_a) sin(2 pi u_b), evaluated in f64: an f32 libm differs between device and host by 1e-7, which a walk of some
 * hundred steps would carry into its columns.  Step s owns the Philox blocks LDSIM_TRACK_GEN_STEP_BLOCKS s + 0 .. 31, i.e. the
 * draw indices 128 s + i; an index whose branch is not taken stays unused.  In order: i = 0, 1: z0 (cos member); 2, 3: z2 (cos)
 * and z3 (sin member); 4: the Poisson u; collision j, draw r = 0 .. 3: u_e, u_a = 8 + 8 j + 2 r, 9 + 8 j + 2 r.
 * Output.  One segment per step, ordered by (primary index, step index): a count pass writes every primary's number of segments,
 * an exclusive scan gives its offset, the write pass walks again and stores there.  f64 columns [LDSIM_TRACK_GEN_NF64][capacity]:
 * x_start, y_start, z_start, x_end, y_end, z_end, x, y, z (midpoint), dx = h, dE, dEdx = dE / dx (0 where dx is 0), t_start,
 * t_end, t (midpoint); i32 columns [LDSIM_TRACK_GEN_NI32][capacity]: primary index, step index, pdg, event_id.
 * ldsim_track_gen_count: counts [n], end_state [n] (0 stopped, 1 left the box, 2 truncated) and end [n][6] = end point, end
 * time, path length, remaining kinetic energy.  ldsim_track_gen: the columns; it reuses the counts of a count pass over the same
 * (parameters, primaries, seed) when that was the context's last one, and counts itself otherwise.  *n_segments = segments
 * written.  ldsim_track_gen_ms: HIP-event time of the last write pass.  Option track_gen_group_primaries (ldsim_set_option, 64 ..
 * 2^20, or 0, the default: n / 2048 held to 64 .. 1024): primaries one workgroup walks; the bytes do not depend on it.
 * LDSIM_EINVAL (with a message naming the entry): step, min_step, max_loss_fraction, t_cut, t_min, a medium constant or a primary's
 * kinetic energy not finite and > 0, min_step > step, max_loss_fraction > 1, t_cut <= the mean excitation energy, a stopping
 * power that is not positive at t_min, an empty or inverted world box, max_steps outside 1 .. LDSIM_TRACK_GEN_MAX_STEPS, a
 * primary outside the world box, a zero direction, an unknown pdg, more than 2^31 - 1 primaries or segments, a capacity that is
 * too small (the message says how many segments are needed), a NULL array. */
#define LDSIM_TRACK_GEN_ME 0.51099895
#define LDSIM_TRACK_GEN_M_MUON 105.6583755
#define LDSIM_TRACK_GEN_M_PION 139.57039
#define LDSIM_TRACK_GEN_M_PROTON 938.27208816
#define LDSIM_TRACK_GEN_HARD_CAP 8
#define LDSIM_TRACK_GEN_HARD_TRIES 4
#define LDSIM_TRACK_GEN_STEP_BLOCKS 32
#define LDSIM_TRACK_GEN_MAX_STEPS 16777216
#define LDSIM_TRACK_GEN_NF64 15
#define LDSIM_TRACK_GEN_NI32 4
typedef struct LdsimTrackGenParams {   /* 192 bytes */
  double world_lo[3];            /* offset 0: the world box, cm, file frame */
  double world_hi[3];            /* 24 */
  double step;                   /* 48: largest step, cm */
  double min_step;               /* 56 */
  double max_loss_fraction;      /* 64: largest mean loss of a step as a fraction of T, in (0, 1] */
  double t_cut;                  /* 72: MeV; collisions above it are sampled one by one */
  double t_min;                  /* 80: MeV; a walk ends below it */
  double density;                /* 88: g / cm^3 */
  double z_over_a;               /* 96: mol / g */
  double mean_excitation;        /* 104: I, MeV */
  double rad_length;             /* 112: X0, g / cm^2 */
  double k_coeff;                /* 120: K = 4 pi N_A r_e^2 me c^2, MeV cm^2 / mol */
  double sternheimer[6];         /* 128: a, k, x0, x1, Cbar, delta0 */
  int32_t straggling;            /* 176 */
  int32_t mcs;                   /* 180 */
  int32_t energy_loss;           /* 184: 0 keeps T (tests of the scattering alone) */
  int32_t max_steps;             /* 188 */
} LdsimTrackGenParams;
typedef struct LdsimTrackGenPrimary {  /* 80 bytes */
  double pos[3];                 /* offset 0 */
  double dir[3];                 /* 24: any length > 0, normalised by the walk */
  double kinetic_energy;         /* 48: MeV */
  double time;                   /* 56: us */
  int32_t pdg;                   /* 64 */
  int32_t event_id;              /* 68 */
  int32_t track_in_event;        /* 72 */
  int32_t _pad;                  /* 76 */
} LdsimTrackGenPrimary;
int ldsim_track_gen_count(ldsim_ctx* ctx, const LdsimTrackGenParams* params, const LdsimTrackGenPrimary* primaries, int64_t n,
                          uint64_t seed, int32_t* counts, int32_t* end_state, double* end);
int ldsim_track_gen(ldsim_ctx* ctx, const LdsimTrackGenParams* params, const LdsimTrackGenPrimary* primaries, int64_t n,
                    uint64_t seed, int64_t capacity, double* f64_columns, int32_t* i32_columns, int64_t* n_segments);
int ldsim_track_gen_ms(ldsim_ctx* ctx, double* ms);

/* ---- track cascade: delta rays, electrons and muon decays as tracks of their own (csrc/kernels_trackgen.hip) ------------------
 * The walk above, with three additions: electrons are transported, a walk emits further particles, and those are walked in turn,
 * one generation per call; larndsim_amd/track_cascade.py restates it in numpy (walk_generation_twin), loops over the generations
 * (cascade, cascade_twin) and writes the file's parent links.  The entries above are untouched: pdg 11 stays unknown to them.
 * Electrons, pdg +-11, mass LDSIM_TRACK_GEN_ME.  A positron is an electron of the other sign: no annihilation, no Bhabha
 * scattering -- a parameter of the model, as the pion's.  tau = T / me, gamma = tau + 1, bg2 = tau (tau + 2), beta^2 = bg2 / gamma^2,
 * e = I / me, g = (2 gamma - 1) / gamma^2, Tmax = T / 2 (Moller: the two electrons are indistinguishable).  Rate of the collisions
 * below Tc (gen_rate_e), d = min(Tc, T / 2) / me:  S_r = (K / 2)(Z/A) rho / beta^2 [ ln(2 (tau + 2) / e^2) - 1 - beta^2
 * + ln((tau - d) d) + tau / (tau - d) + (d^2 / 2 + (2 tau + 1) ln(1 - d / tau)) / gamma^2 - delta(bg2) ]; d = tau / 2 is the
 * unrestricted ICRU-37 electron stopping power (with the default LAr constants 1.369, 1.473, 1.555 and 1.718 MeV cm^2 / g at 1, 5,
 * 10 and 50 MeV).  Hard collisions above t_cut follow Moller: x = eps / T in [x0, x1] = [t_cut / T,
 * 1/2], d sigma / d eps ~ (1 / T^2) [1 / x^2 + 1 / (1 - x)^2 + (1 - g) - g / (x (1 - x))] with the prefactor (K / 2)(Z/A) rho /
 * beta^2 per cm; Poisson mean of a step (gen_lambda_e) lambda = (xi / T) [(x1 - x0)(1 - g + 1 / (x0 x1) + 1 / ((1 - x0)(1 - x1)))
 * - g ln(x1 (1 - x0) / (x0 (1 - x1)))]; restricted loss plus the hard part's mean is the unrestricted loss identically.  The
 * count is drawn as above (cap LDSIM_TRACK_GEN_HARD_CAP).  Collision j draws x from the proposal 1 / x^2 + 1 / (1 - x)^2 by
 * inversion -- G(x) = (2 x - 1) / (x (1 - x)), c = G(x0)(1 - u_e), x = 2 / ((2 - c) + sqrt(4 + c^2)) -- and keeps it when
 * u_a R <= r(x), r(x) = 1 + ((1 - g) y^2 - g y) / (1 - 2 y) with y = x (1 - x) the ratio of Moller's shape to the proposal and
 * R = max(r(x0), r(1/2)) its largest value on the interval (dr/dy has the sign of 2 (1 - g) y (1 - y) - g, which rises in y: r
 * falls, then rises).  T_h = x Tm.  Try LDSIM_TRACK_GEN_MOLLER_TRIES = 7 is kept whatever (it draws no u_a).  A try is refused
 * with probability 1 - (integral of the shape) / (R integral of the proposal) <= 0.1775 for every g in (0, 1] and x0 in (0, 1/2)
 * (the supremum, found numerically, is 0.17747 at g = 1, x0 = 0.178), so the forced try is reached with probability <= 0.1775^6
 * = 3.13e-5 per collision.  The heavy particles' four-try sampler is the one above.  Soft Gaussian, midpoint rule, step rule, t_min,
 * Highland scattering, walls and truncation are those above, evaluated with the electron's Tmax and S_r.
 * Delta rays (delta_tracks, threshold t_track >= max(t_cut, t_min)), for heavy and electron parents alike.  An accepted hard
 * collision with T_h >= t_track is not added to the segment's dE; the parent's T still falls by it, and an electron (pdg 11) of
 * kinetic energy T_h is emitted.  Collisions between t_cut and t_track are deposited as above.  Direction: polar angle against
 * the parent's direction at the step's start cos theta = T_h (E + me) / (p p_e) <= 1 (clamped), E and p the parent's total
 * energy and momentum at Tm, p_e = sqrt(T_h (T_h + 2 me)); azimuth 2 pi u; turned into the parent's frame by the step's own
 * rotation.  It starts at p + u' h d on the parent's segment as it ended (h after a stop's shortening; held inside the box), at
 * t0 + u' (t1 - t0).  The parent's direction is not changed by the collision.  Stop rule: the walk ends stopped when dE + emitted
 * >= T or T - dE - emitted < t_min, then dE = T - emitted.  A collision is emitted only while emitted + T_h < T, taken in the
 * order j; one that would exhaust T is deposited instead, so dE stays positive.
 * Decay of stopped muons (decays).  A walk of |pdg| 13 that ends in state 0 draws from the step index after its last.  mu+ always
 * decays; mu- is captured where u_c <= capture_fraction (nothing is emitted, the rest energy is not tracked), else decays.  The
 * electron has the muon's sign (13 -> 11, -13 -> -11), starts at the end point at t_end - lifetime ln u_t, isotropically (mu = 1 -
 * 2 u, phi = 2 pi u), with total energy x W, W = (m_mu^2 + me^2) / (2 m_mu), x from the unpolarised Michel spectrum n(x) = 2 x^2
 * (3 - 2 x) on (0, 1] by inversion: F(x) = 2 x^3 - x^4 = u_x solved by LDSIM_TRACK_GEN_MICHEL_NEWTON = 8 Newton steps from
 * cbrt(u_x / 2) (F is convex and rising, so the iterates fall onto the root from the second on; 8 steps reach the last bit; no
 * try is forced).  Nothing is emitted where x W <= me.  mu_plus_lifetime 2.1969811 us; mu_minus_lifetime (0.537 us)
 * and capture_fraction (0.76) are PARAMETERS of the argon medium as recalled from the literature, not measurements of this
 * project; they are consistent with each other (0.537 / 2.197 = 0.244 = 1 - 0.76).
 * Out of scope: pion decay, capture products, bremsstrahlung, photons, annihilation, polarisation.  A Michel electron here loses
 * energy by collisions only, so its track is longer than a real one (a 50 MeV electron's collision-only range is 22 cm).
 * Draws of step s (indices 128 s + i) beyond those above: electron collision j, try r < 4: u_e, u_a = 8 + 8 j + 2 r, 9 + 8 j + 2 r
 * (the heavy sampler's places); tries 4, 5: LDSIM_TRACK_GEN_DRAW_MOLLER + 5 j + 2 (r - 4) and the next; try 6: u_e =
 * LDSIM_TRACK_GEN_DRAW_MOLLER + 5 j + 4; a delta ray of collision j: azimuth LDSIM_TRACK_GEN_DRAW_AZIMUTH + j, place
 * LDSIM_TRACK_GEN_DRAW_PLACE + j.  Decay, at the step index after the last: 0 u_c, 1 u_t, 2 mu, 3 phi, 4 u_x.
 * Generations.  Generation 0 is the caller's list (ldsim_track_cascade_particles fills key as the walk above derives it, parent
 * -1, process 0); generation k + 1 is what generation k emitted, in the order (parent index, step, collision j; the decay
 * product last).  A secondary's stream key is key_mix(key_mix(parent key, 1 + step), 1 + j), the decay's
 * key_mix(key_mix(parent key, 1 + steps), LDSIM_TRACK_GEN_DECAY_KEY): a walk, and so its whole family, is a pure function of
 * (parameters, ancestor record, seed).  The caller loops until nothing is emitted or to its cap, and walks the last generation
 * with emit = 0: hard collisions are deposited and nothing decays, so energy is conserved whatever the cap.
 * ldsim_track_cascade_count: counts [n], secondary_counts [n], end_state [n], end [n][6] as ldsim_track_gen_count.
 * ldsim_track_cascade walks ONE generation: the segments in the columns above, ordered (particle, step), the column "primary"
 * holding the particle's index; the emitted records at (exclusive scan of secondary_counts)[particle] + running index.  It reuses
 * a count pass over the same (parameters, cascade parameters, particles, seed).  ldsim_track_cascade_ms: HIP-event time of the
 * last write pass.  LDSIM_EINVAL, naming the entry: what the entries above refuse of the parameters and of a record (pdg: +-11,
 * +-13, +-211, 2212), an electron stopping power that is not positive at t_min, t_track not finite or below t_cut or t_min,
 * capture_fraction outside [0, 1], a lifetime not finite and > 0, a segment or secondary capacity that is too small (the message
 * says how many are needed), more than 2^31 - 1 segments or secondaries, a NULL array. */
#define LDSIM_TRACK_GEN_MOLLER_TRIES 7
#define LDSIM_TRACK_GEN_MICHEL_NEWTON 8
#define LDSIM_TRACK_GEN_DRAW_AZIMUTH 72
#define LDSIM_TRACK_GEN_DRAW_PLACE 80
#define LDSIM_TRACK_GEN_DRAW_MOLLER 88
#define LDSIM_TRACK_GEN_DECAY_KEY 256
typedef struct LdsimTrackGenParticle { /* 104 bytes */
  double pos[3];                 /* offset 0: LdsimTrackGenPrimary's fields */
  double dir[3];                 /* 24 */
  double kinetic_energy;         /* 48 */
  double time;                   /* 56 */
  int32_t pdg;                   /* 64 */
  int32_t event_id;              /* 68 */
  int32_t track_in_event;        /* 72: the generation-0 ancestor's */
  int32_t _pad;                  /* 76 */
  uint64_t key;                  /* 80: the walk's stream key */
  int32_t parent;                /* 88: index in the previous generation, -1 in generation 0 */
  int32_t generation;            /* 92 */
  int32_t process;               /* 96: 0 primary, 1 delta ray, 2 decay */
  int32_t parent_step;           /* 100: the emitting step; a decay: the parent's number of steps; -1 in generation 0 */
} LdsimTrackGenParticle;
typedef struct LdsimTrackGenCascadeParams { /* 48 bytes */
  double t_track;                /* offset 0: MeV; hard collisions from here on become tracks */
  double mu_plus_lifetime;       /* 8: us */
  double mu_minus_lifetime;      /* 16: us, in argon (a parameter) */
  double capture_fraction;       /* 24: of stopped mu- in argon (a parameter) */
  int32_t delta_tracks;          /* 32 */
  int32_t decays;                /* 36 */
  int32_t emit;                  /* 40: 0 = the last generation: nothing is emitted */
  int32_t _pad;                  /* 44 */
} LdsimTrackGenCascadeParams;
int ldsim_track_cascade_particles(const LdsimTrackGenPrimary* primaries, int64_t n, LdsimTrackGenParticle* particles);
int ldsim_track_cascade_count(ldsim_ctx* ctx, const LdsimTrackGenParams* params, const LdsimTrackGenCascadeParams* cascade,
                              const LdsimTrackGenParticle* particles, int64_t n, uint64_t seed, int32_t* counts,
                              int32_t* secondary_counts, int32_t* end_state, double* end);
int ldsim_track_cascade(ldsim_ctx* ctx, const LdsimTrackGenParams* params, const LdsimTrackGenCascadeParams* cascade,
                        const LdsimTrackGenParticle* particles, int64_t n, uint64_t seed, int64_t capacity, double* f64_columns,
                        int32_t* i32_columns, int64_t* n_segments, int64_t secondary_capacity, LdsimTrackGenParticle* secondaries,
                        int64_t* n_secondaries);
int ldsim_track_cascade_ms(ldsim_ctx* ctx, double* ms);

/* ---- multi-GPU: the one exchange step of the batch-sharded path, RCCL over xGMI -------------------------------
 * One process per GPU; (event, TPC-group) batches are sharded over the ranks and never share a pixel, so the only
 * collective reassembles the output: row counts (all-gather), then the 24-byte hit rows (all-gather-v). */
#define LDSIM_COMM_ID_BYTES 128
/* ncclGetUniqueId on one rank; the host side hands the 128 bytes to every rank (larndsim_amd/comm.py) */
int ldsim_comm_unique_id(void* id);
int ldsim_comm_init(ldsim_ctx* ctx, const void* id, int32_t rank, int32_t world);
int ldsim_comm_destroy(ldsim_ctx* ctx);
/* ranks in the communicator and this rank's index as RCCL reports them (ncclCommCount, ncclCommUserRank); rank may be NULL */
int ldsim_comm_count(ldsim_ctx* ctx, int32_t* n_ranks, int32_t* rank);
/* *value reduced over the ranks (op 0 = sum, 1 = max); also the barrier of the timed region */
int ldsim_comm_allreduce_f64(ldsim_ctx* ctx, double* value, int32_t op);
/* append the last ldsim_charge_chain call's compact hit rows to the pass buffer (reset != 0 empties it first) */
int ldsim_hits_accumulate(ldsim_ctx* ctx, int32_t reset);
/* all-gather-v of the pass buffer: *gathered = device pointer (ctx-owned) to the rows of rank 0, 1, .. back to back,
 * counts[world] (may be NULL) = rows per rank */
int ldsim_comm_allgather_hits(ldsim_ctx* ctx, void** gathered, int64_t* total_rows, int64_t* counts);
int ldsim_comm_gathered_download(ldsim_ctx* ctx, void* rows, int64_t n);

/* ---- the drop-in driver's exchange (cli/simulate_pixels.py --n_gpus): every rank's results to one writer ---------------------
 * ldsim_compact_accumulate: after ldsim_chain_compact_build, append the launch's five compact parts to this rank's stream in HBM
 * (device-to-device on the ctx stream; a launch is appended once).  reset != 0 only empties the stream: call it before the first
 * launch of a pass.  Parts, in this order: hit-pixel rows [5] i32, track segments i64, hit rows (24 B), charges f64, fractions f64.
 * ldsim_comm_gather_compact: collective, one source rank per call.  All-gather of the five element counts of every rank
 * (sizes[world][5], may be NULL), then root receives rank src_rank's parts (ncclSend / ncclRecv, one call per part; a
 * device-to-device copy when src_rank is root) into buffers sized for that rank alone, so root never holds more than one
 * rank's stream: loop src_rank over the ranks and export each before receiving the next.
 * ldsim_comm_gathered_compact_download (root only): the parts of the last gather, from rank src_rank, in the layout of
 * ldsim_chain_compact_download (buffers sized from sizes[src_rank]; any pointer may be NULL).
 * ldsim_comm_gatherv_bytes: collective gather-v of n host bytes per rank to root through device staging (counts[world] = bytes
 * per rank, may be NULL); ldsim_comm_gathered_bytes_download (root only): rank src_rank's bytes.
 * LDSIM_EINVAL: no communicator, root / source rank out of range, an all-gathered size of this rank that differs from the local
 * one; LDSIM_ESTATE: accumulate without a compact build of the last launch, a download of a rank this rank has not gathered as
 * root by the last call. */
int ldsim_compact_accumulate(ldsim_ctx* ctx, int32_t reset);
int ldsim_comm_gather_compact(ldsim_ctx* ctx, int32_t root, int32_t src_rank, int64_t* sizes);
int ldsim_comm_gathered_compact_download(ldsim_ctx* ctx, int32_t src_rank, int32_t* hit_pixels, int64_t* track_segments,
                                         void* hit_rows, double* hit_charge, double* fractions);
int ldsim_comm_gatherv_bytes(ldsim_ctx* ctx, int32_t root, const void* host, int64_t n, int64_t* counts);
int ldsim_comm_gathered_bytes_download(ldsim_ctx* ctx, int32_t src_rank, void* out);

/* ---- fee.export_to_hdf5's hit loop on compact rows (larndsim/fee.py:143-344) -- host code, no ctx, no GPU ---------------------------
 * The LArPix `packets` rows (larpix-control's HDF5 format 2.4: 36-byte packed rows, ldsim_packets_row_bytes) and the
 * `mc_packets_assn` rows (event_ids (1,) i8 | segment_ids (n,) i8 | fraction (n,) f8 | file_traj_ids (n,) i8 | fraction_traj (n,) f8,
 * n = ASSOCIATION_COUNT_TO_STORE: ldsim_packets_assn_row_bytes) of one export, from the rows the reference's loop would enter --
 * the pixels whose first ADC lies above the pedestal code, in export order (batch after batch, pixel after pixel) -- with what is
 * per row precomputed by the caller (larndsim_amd/packets.py: pixel -> io_group / io_channel / chip / channel through tile map,
 * tile orientation and pixel layout, fee.py:150-157,238-255; event start times).  Per hit: clock rollover (:164-183), the packets
 * of a new event (timestamp + sync per io group, the event's light triggers, :187-230), the timestamp packet of a changed tick
 * (:267-277), the data packet with its parity, and the association row (:284-344; equal fractions keep descending slot order --
 * numpy's argsort leaves their order to its build).  Returns the number of rows written, or a negative status. */
typedef struct {
  int64_t n_rows;               /* rows entering the hit loop */
  const int64_t* row_event;     /* [n_rows] event id */
  const int64_t* row_base;      /* [n_rows] int(event_start_time / CLOCK_CYCLE) */
  const int64_t* row_ts_s;      /* [n_rows] int(event_start_time * mus / s): value of the per-event timestamp packets */
  const uint8_t* row_ok;        /* [n_rows] the pixel has a readout address and its channel is not disabled */
  const int32_t* row_io_group;  /* [n_rows] */
  const int32_t* row_io_channel;
  const int32_t* row_chip;
  const int32_t* row_channel;
  const int64_t* row_hit0;      /* [n_rows + 1] offsets into hit_*: the row's slots up to the first ADC <= pedestal */
  const int64_t* row_trk0;      /* [n_rows + 1] offsets into trk_*: the row's filled track slots */
  const int64_t* row_frac0;     /* [n_rows] offset into hit_frac of the row's first hit: [slot][track slot] from there */
  const int32_t* hit_adc;       /* ADC code */
  const double* hit_tick;       /* adc_ticks_list value */
  const double* hit_frac;       /* backtracking fractions */
  const int64_t* trk_segment;   /* segment id of a track slot (track_ids) */
  const int64_t* trk_traj;      /* trajectory id of a track slot (traj_ids) */
  int64_t base0;                /* int(event_start_time / CLOCK_CYCLE) of row 0 of the export's arrays (a row without hits included) */
  int32_t first_row_is_row0;    /* rows[0] is that row 0 */
  int32_t light_trig_mode;      /* light.LIGHT_TRIG_MODE */
  int64_t n_trig;               /* light triggers of the export (fee.py:209-221) */
  const double* trig_time;
  const int64_t* trig_event;
  const int64_t* trig_module;
  int32_t n_io_groups;          /* io groups that get the per-event timestamp / sync packets */
  const int32_t* io_groups;
  int32_t n_modules;            /* MODULE_TO_IO_GROUPS: module ids, and per module its groups module_groups[module_group0[m] .. [m + 1]) */
  const int64_t* module_ids;
  const int32_t* module_group0;
  const int32_t* module_groups;
  int64_t clock_reset_period;   /* detector.CLOCK_RESET_PERIOD */
  double clock_cycle, mus, s;   /* detector.CLOCK_CYCLE, units.mus, units.s */
  int32_t n_keep, max_tracks;   /* sim.ASSOCIATION_COUNT_TO_STORE, sim.MAX_TRACKS_PER_PIXEL */
} LdsimPacketsIn;
int32_t ldsim_packets_row_bytes(void);
int32_t ldsim_packets_assn_row_bytes(int32_t n_keep);
int64_t ldsim_packets_build(const LdsimPacketsIn* in, void* packets_out, void* assn_out, int64_t capacity);

/* ---- output writer helper (host only, no ctx) ----
 * CRC-32 (reflected 0xEDB88320: what a ZIP member carries, = zlib.crc32) of the concatenation of n_parts byte ranges on
 * n_threads host threads (<= 0: all hardware threads).  The driver's .npz writer (cli/simulate_pixels.py OutputFile, the stand-in
 * for the h5py datasets of the reference's cli/simulate_pixels.py:1240-1301) checksums a dataset that exists as the .npy header
 * plus one piece per chain launch without joining the pieces. */
uint32_t ldsim_crc32_parts(const void* const* parts, const uint64_t* sizes, int64_t n_parts, int32_t n_threads);

/* timing of the dominant kernel over the last chain call, measured with HIP events on the ctx stream */
int ldsim_chain_kernel_ms(ldsim_ctx* ctx, double* current_ms, double* adc_ms, double* total_ms);
/* split of current_ms over the tracks_current kernels of the last chain call: weights_kernel, mac_kernel and the
 * monolithic current_kernel (overflow fallback, or the whole stage when the split path is off: then the first two are 0) */
int ldsim_chain_kernel_ms_detail(ldsim_ctx* ctx, double* weights_ms, double* mac_ms, double* fallback_ms);

#ifdef __cplusplus
}
#endif
#endif /* LDSIM_H */
