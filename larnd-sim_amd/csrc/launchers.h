// launchers.h -- every host function that one translation unit defines and another one calls, declared once.  A file that
// defines one of them includes this header, so a changed signature fails to compile instead of linking to a stale copy.
#pragma once
#include "ldsim_args.h"

struct SplitArgs;   // split_common.h
struct GArgs;       // gform.h

// ---- kernels_seg.hip ---------------------------------------------------------------------------------------------------
int seg_launch_unpack(ldsim_ctx* ctx, const LdsimTrackLayout* lay, int64_t n);
int seg_launch_repack(ldsim_ctx* ctx, const LdsimTrackLayout* lay, int64_t n);
int seg_launch_quench_drift(ldsim_ctx* ctx, int mode, int do_q, int do_d, int* d_err);
int seg_launch_quench_drift_map(ldsim_ctx* ctx, int mode, int* d_err);
int seg_launch_quench_drift_stat(ldsim_ctx* ctx, int mode, bool map, const int32_t* d_first, int32_t batch0, int* d_err);
int seg_launch_max_pixels(ldsim_ctx* ctx, int64_t b, int64_t e, int32_t* d_nmax, unsigned long long* d_tranbits);
int seg_launch_front(ldsim_ctx* ctx, int64_t b, int64_t e, int32_t batch0, double* starts, int32_t* d_nmax, int32_t* tmax_b,
                     int32_t* first_b, unsigned long long* tran_b);
int seg_launch_get_pixels(ldsim_ctx* ctx, int64_t b, int64_t e, int radius, int32_t* active, int max_active, int32_t* neigh,
                          int32_t* nrad, int P, double* n_list, const int32_t* radius_b, int32_t batch0);
int seg_launch_time_intervals(ldsim_ctx* ctx, int64_t b, int64_t e, double* starts, int32_t* tmax);

// ---- kernels_trackgen.hip (the entry points of ldsim_abi.hip hand their arguments through) ---------------------------------
int trackgen_count(ldsim_ctx* ctx, const LdsimTrackGenParams* P, const LdsimTrackGenPrimary* prim, int64_t n, uint64_t seed,
                   int32_t* counts, int32_t* end_state, double* end);
int trackgen_generate(ldsim_ctx* ctx, const LdsimTrackGenParams* P, const LdsimTrackGenPrimary* prim, int64_t n, uint64_t seed,
                      int64_t capacity, double* f64_columns, int32_t* i32_columns, int64_t* n_segments);
int trackgen_cascade_count(ldsim_ctx* ctx, const LdsimTrackGenParams* P, const LdsimTrackGenCascadeParams* CP,
                           const LdsimTrackGenParticle* part, int64_t n, uint64_t seed, int32_t* counts, int32_t* secondary_counts,
                           int32_t* end_state, double* end);
int trackgen_cascade(ldsim_ctx* ctx, const LdsimTrackGenParams* P, const LdsimTrackGenCascadeParams* CP,
                     const LdsimTrackGenParticle* part, int64_t n, uint64_t seed, int64_t capacity, double* f64_columns,
                     int32_t* i32_columns, int64_t* n_segments, int64_t secondary_capacity, LdsimTrackGenParticle* secondaries,
                     int64_t* n_secondaries);
int trackgen_cascade_particles(const LdsimTrackGenPrimary* prim, int64_t n, LdsimTrackGenParticle* out);

// ---- kernels_lutbuild.hip (the entry points of ldsim_abi.hip hand their arguments through) ----------------------------------
int lutbuild_build(ldsim_ctx* ctx, const LdsimLutBuildParams* P, const LdsimLutDetector* dets, int32_t ndet, int32_t nx,
                   int32_t ny, int32_t nz, int64_t voxel_begin, int64_t voxel_end, int64_t n_photons, uint64_t seed,
                   uint32_t* counts, uint32_t* hist, float* tmin, uint64_t* tsum, uint64_t* fates);
int lutbuild_trace(ldsim_ctx* ctx, const LdsimLutBuildParams* P, const LdsimLutDetector* dets, int32_t ndet, int32_t nx,
                   int32_t ny, int32_t nz, int64_t voxel, int64_t photon_begin, int64_t photon_end, uint64_t seed, int32_t* fate,
                   int32_t* steps, double* time, double* end);

// ---- kernels_respbuild.hip ---------------------------------------------------------------------------------------------------
int respbuild_build(ldsim_ctx* ctx, const LdsimResponseBuildParams* P, double* table);

// ---- kernels_fmapbuild.hip ---------------------------------------------------------------------------------------------------
int fmapbuild_solve(ldsim_ctx* ctx, const LdsimFieldMapBuildParams* P, const double* source, double* psi_inout, int32_t* iterations,
                    double* residual);
int fmapbuild_trace(ldsim_ctx* ctx, const LdsimFieldMapBuildParams* P, const double* psi, double* E, double* dx, double* dy,
                    double* dz, uint8_t* flags);

// ---- sort.hip ----------------------------------------------------------------------------------------------------------
int sort_select_pairs(ldsim_ctx* ctx, const int32_t* neigh, const int32_t* nrad, int64_t seg_begin, int32_t batch0, int P,
                      int64_t n_entries, unsigned long long* keys_out, int32_t* vals_out, unsigned long long* d_count);
void sort_key_ranges(unsigned long long pixel_max, int64_t n_batches, int r[3]);
int sort_pairs(ldsim_ctx* ctx, unsigned long long* keys_in, unsigned long long* keys_out, int32_t* vals_in, int32_t* vals_out,
               int64_t n);
int sort_pairs_bits(ldsim_ctx* ctx, unsigned long long* keys_in, unsigned long long* keys_out, int32_t* vals_in,
                    int32_t* vals_out, int64_t n, int begin_bit, int end_bit);
int sort_pairs_u32_u64(ldsim_ctx* ctx, unsigned* keys_in, unsigned* keys_out, unsigned long long* vals_in,
                       unsigned long long* vals_out, int64_t n, int bits);
int sort_exclusive_scan_i32(ldsim_ctx* ctx, const int32_t* in, int32_t* out, int64_t n);
int sort_exclusive_scan_u64(ldsim_ctx* ctx, const unsigned long long* in, unsigned long long* out, int64_t n);
int sort_heads(ldsim_ctx* ctx, const unsigned long long* keys, int64_t n_valid, int32_t* heads);
int sort_fill_unique(ldsim_ctx* ctx, const unsigned long long* keys, const int32_t* heads, const int32_t* uidx, int64_t n_valid,
                     int32_t batch0, int32_t* upix, int32_t* ubatch, int64_t* uoff, int64_t U);
struct GInfo;   // gform.h
int sort_scan_record_sizes(ldsim_ctx* ctx, const GInfo* gi, unsigned long long* off, int64_t n);
int sort_batch_first(ldsim_ctx* ctx, int64_t seg_begin, int64_t n, int32_t batch0, int32_t* first);
int sort_compact_hits(ldsim_ctx* ctx, const int32_t* upix, const int32_t* ubatch, const int32_t* hit_count,
                      const int32_t* hit_off, const double* digit, const double* ticks, int A, int64_t U, int32_t* rows);

// ---- induced current: kernels_current.hip, kernels_mc.hip, kernels_split.hip, kernels_qweights.hip, kernels_qsetup.hip,
// kernels_macshift.hip, kernels_gtables.hip, kernels_gcorr.hip -------------------------------------------------------------
int current_launch(ldsim_ctx* ctx, const CurArgs& args);
int current_mc_launch(ldsim_ctx* ctx, const CurArgs& args, int64_t n_seg);
int split_sizes(const ldsim_ctx* ctx, const CurArgs& args, size_t* item_bytes, size_t* hdr_bytes, size_t* corr_bytes);
int split_launch_weights(ldsim_ctx* ctx, const CurArgs& args, void* items, void* hdr, void* corr, double* wbuf,
                         unsigned long long wbuf_cap, unsigned long long* cursor);
int split_launch_mac(ldsim_ctx* ctx, const CurArgs& args, void* items, void* hdr, void* corr, double* wbuf,
                     unsigned long long wbuf_cap, unsigned long long* cursor);
int qweights_launch(ldsim_ctx* ctx, const SplitArgs& S, int M, void* params);
size_t qpair_params_bytes(int64_t n_pairs);
int qpair_setup_launch(ldsim_ctx* ctx, const SplitArgs& S, int M, void* params, void* ginfo, void* maps);
int resp_pad_ensure(ldsim_ctx* ctx, const CurArgs& A, int* k_lo_out, int* k_hi_out, int* nkp_out);
int mac_shift_launch(ldsim_ctx* ctx, SplitArgs S, int M);
int gtables_list_launch(ldsim_ctx* ctx, const GArgs& GA, int32_t* wg_list, unsigned long long* wg_count, int32_t* w2_list,
                        unsigned long long* w2_count);
int gtables_launch_range(ldsim_ctx* ctx, const GArgs& GA, int M, hipStream_t ts, int64_t pair0, int64_t n);
int gtables_launch_lists(ldsim_ctx* ctx, const GArgs& GA, int M, hipStream_t ts, const int32_t* wg_list, int64_t n_wg,
                         const int32_t* w2_list, int64_t n_w2);
int gtables_launch(ldsim_ctx* ctx, const GArgs& GA, int M, const int32_t* wg_list, int64_t n_wg, const int32_t* w2_list,
                   int64_t n_w2);
int gform_launch(ldsim_ctx* ctx, const CurArgs& a, unsigned long long* counters, int32_t** flags_out,
                 const int32_t** flag_list, const unsigned long long** flag_count);
int gform_census(ldsim_ctx* ctx, int64_t* counts, int32_t n_out);
int gform_fused_report(ldsim_ctx* ctx, int64_t* out, int32_t n_out);

// ---- kernels_fee.hip ---------------------------------------------------------------------------------------------------
int fee_launch_chain(ldsim_ctx* ctx, const FeeArgs& F0);
int fee_launch_tables(ldsim_ctx* ctx, double dt, double rt, double* tab);
int fee_clear_unwritten_fractions(ldsim_ctx* ctx, int64_t U, const int32_t* hit_count, const int64_t* tpm, double* fr);
int fee_launch_track_pixel_map(ldsim_ctx* ctx, int64_t* map, const int32_t* upix, int64_t U, const int32_t* pixels,
                               const int32_t* dist, int64_t S, int P, int max_distance, int M);
int fee_launch_sum_pixel_signals(ldsim_ctx* ctx, double* ps, const float* signals, const double* starts, const int64_t* pim,
                                 const int64_t* tpm, double* pts, double* ovf, int64_t S, int P, int T, int NT, int M);
int fee_launch_adc_dense(ldsim_ctx* ctx, const double* ps, const double* pts, int64_t U, int NT, int M, const double* thr,
                         double time_padding, double t_stop, const float* noise_z, int noise_nd, int32_t* n_draws, double* adc,
                         double* ticks, double* frac);
int fee_launch_digitize(ldsim_ctx* ctx, const double* q, const double* gain, double* out, int64_t n);

// ---- the passes that read a chain launch afterwards (pixel truth, pixel waveforms, FEE and charge universes): ldsim_abi.hip -----
// 0 while the scratch buffers hold the last chain launch and its set-up record describes them; else LDSIM_ESTATE, `who` named
int launch_need_record(ldsim_ctx* ctx, const char* who);
// a buffer of the pass `pass`, named in the message with `what`; an allocation that fails leaves the buffer empty and the context
// usable (LDSIM_ENOMEM)
int pass_ensure(DevBuf& b, size_t need, const char* pass, const char* what);

// ---- kernels_rng.hip ---------------------------------------------------------------------------------------------------
int rng_ensure_states(ldsim_ctx* ctx, int64_t n);
int rng_fee_draws_per_pixel(const LdsimConsts& h, int NT);
int rng_launch_fee_noise(ldsim_ctx* ctx, int64_t U, int nd, float* z);
int rng_launch_advance(ldsim_ctx* ctx, int64_t U, const int32_t* n_draws);
int rng_launch_fee_keyed_fill(ldsim_ctx* ctx, const int32_t* ubatch, const int32_t* upix, int64_t U, int nd, float* z);

// ---- light: kernels_light.hip, kernels_light_response.hip, light_wvfm.hip -------------------------------------------------
// light_incidence_kernel / light_incidence4_kernel, or under option light_lut_interp light_incidence_interp_kernel /
// light_incidence_interp4_kernel (trilinear visibility between voxel centres); host-buffer stage call and resident leg alike
int light_launch_incidence(ldsim_ctx* ctx, int64_t seg0, int64_t n, int n_out, float* nph, float* t0det, int32_t* voxel,
                           int fill);
int light_launch_t0_range(ldsim_ctx* ctx, const float* nph, const float* t0det, int64_t total, int* d_res);
// n_rec_out: truth path, the records left sorted in light_tmp[4] (their cells are what was written); act: no truth slots, the
// sum over a device-built list of the lit (detector, tile) cells
int light_launch_sum(ldsim_ctx* ctx, int64_t seg0, int64_t n, const int32_t* voxel, const int64_t* track_id, const float* nph,
                     int n_inc, const int32_t* op_channel, int n_det, const int32_t* sorted_idx, double start_time,
                     int64_t n_ticks, float* out, int64_t* true_id, double* true_ph, int max_truth, int64_t* n_rec_out,
                     const LightAct* act = nullptr);
int light_launch_reset_cells(ldsim_ctx* ctx, int64_t n_rec, int64_t n_ticks, int max_truth, float* out, int64_t* true_id,
                             double* true_ph);
int light_check_emit_overflow(ldsim_ctx* ctx);
// a response stage on the ctx's stream: the plain sum added to `out` (light_plain_kernel), then the Mt truth slots
// (light_truth_lds_kernel, or light_truth_rows_kernel for more than 64 slots / option light_truth_lds 0)
int light_response_launch(ldsim_ctx* ctx, bool response, const float* inc, const int64_t* tid, const double* tph, int D, int T,
                          int Mt, const double* weights, int C, const double* gain, float* out, int64_t* out_tid,
                          double* out_tph);
int light_launch_stat_fluct(ldsim_ctx* ctx, const float* inc, float* out, int64_t n, int64_t ntick);
int light_sipm_check(const LdsimSipmNoise& v, double tick);
// light universes: out = (float)((double)x * scale); K tables over one input by light_plain_kernel (out[k] = a stage's plain sum
// under table k, the launch's bits; what out[k] held is not read)
int light_universes_scale(ldsim_ctx* ctx, const float* x, int64_t n, double scale, float* out);
int light_universes_conv(ldsim_ctx* ctx, bool response, const float* inc, int D, int T, int C, int K, const double* const* w,
                         const double* const* gain, float* const* out);

// ---- chain.hip ---------------------------------------------------------------------------------------------------------
int chain_run(ldsim_ctx* ctx, int64_t seg_begin, int64_t seg_end, int want_fractions);
int chain_tracks_current(ldsim_ctx* ctx, const int32_t* d_pixels, int P, float* d_signals, int T, int mc);
