// ldsim_dev.h -- shared host/device declarations for libldsim_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <exception>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ldsim.h"

#define LDSIM_WAVE 64

// ---- segment store: struct of arrays in HBM, one f64 column per hot-path field -------------------
// Values are held "as stored": after a kernel mutates a field the column holds the value narrowed
// through the record's storage dtype (f4 rounding / u4 truncation), exactly what the next reference
// kernel would read back from the record.
struct SegStore {                // (its columns are aliases into the ctx's seg_block)
  double* f[LDSIM_NFIELDS - 1];  // all float-like fields (index = enum ldsim_field), n_electrons included
  int32_t* pixel_plane;
  int32_t* batch;                // (event, TPC-group, sub-batch) id; <0 = not simulated
  int32_t store_code[LDSIM_NFIELDS];
  int64_t n;
  int64_t cap;
};

// ---- drift-field map of one TPC (ldsim_set_field_map) ----------------------------------------------------
// A regular grid in the simulation frame; every node holds (E, dx, dy, dz) so that one corner is one 32-byte read.
struct alignas(32) FieldMapNode {
  double e, dx, dy, dz;
};
struct FieldMapDesc {
  const FieldMapNode* node;      // [n[0]][n[1]][n[2]] (alias of the ctx's fmap_nodes[tpc]); nullptr: this TPC has no map
  int32_t n[3];
  int32_t has_e;                 // 0: the map carries no E channel (E = the constants' e_field, whatever module is loaded)
  double origin[3], inv_spacing[3];
};
// The anode view: the nine positions (LDSIM_X_START .. LDSIM_Z) where the drifted charge arrives, one column each
#define LDSIM_NVIEW 9

// ---- Python / Numba scalar semantics on device -----------------------------------------------------
__device__ __forceinline__ double py_round(double x) { return rint(x); }  // half-to-even (v_rndne_f64)

// Python float floor division (CPython float_divmod algorithm, which Numba reproduces)
__device__ __forceinline__ double py_floordiv(double vx, double wx) {
  double mod = fmod(vx, wx);
  double div = (vx - mod) / wx;
  if (mod != 0.0) {
    if ((wx < 0) != (mod < 0)) {
      mod += wx;
      div -= 1.0;
    }
  }
  double fd;
  if (div != 0.0) {
    fd = floor(div);
    if (div - fd > 0.5) fd += 1.0;
  } else {
    fd = copysign(0.0, vx / wx);
  }
  return fd;
}

__device__ __forceinline__ int64_t ifloordiv(int64_t a, int64_t b) {
  int64_t q = a / b;
  if ((a % b != 0) && ((a < 0) != (b < 0))) q -= 1;
  return q;
}
__device__ __forceinline__ int64_t ifloormod(int64_t a, int64_t b) { return a - ifloordiv(a, b) * b; }

__device__ __forceinline__ double narrow_store(double v, int code) {
  switch (code) {
    case LDSIM_F4: return (double)(float)v;
    case LDSIM_I4: return (double)(int32_t)v;
    case LDSIM_U4: return (double)(uint32_t)v;
    case LDSIM_I8: return (double)(int64_t)v;
    case LDSIM_U8: return (double)(uint64_t)v;
    default: return v;
  }
}

__device__ __forceinline__ int64_t pixel2id(const LdsimConsts* c, int64_t px, int64_t py, int64_t plane) {
  return px + c->n_pixels[0] * (py + c->n_pixels[1] * plane);
}
__device__ __forceinline__ void id2pixel(const LdsimConsts* c, int64_t pid, int64_t& px, int64_t& py, int64_t& plane) {
  px = ifloormod(pid, c->n_pixels[0]);
  py = ifloormod(ifloordiv(pid, c->n_pixels[0]), c->n_pixels[1]);
  plane = ifloordiv(pid, (int64_t)c->n_pixels[0] * c->n_pixels[1]);
}
__device__ __forceinline__ bool pix_in_range(const LdsimConsts* c, int64_t x, int64_t y, int64_t plane) {
  return 0 <= x && x < c->n_pixels[0] && 0 <= y && y < c->n_pixels[1] && 0 <= plane && plane < c->n_tpc;
}

// ---- host-side context --------------------------------------------------------------------------------
void ldsim_set_error(const char* fmt, ...);
#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      ldsim_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return LDSIM_EHIP;                                                                  \
    }                                                                                     \
  } while (0)
#define CK(x)                \
  do {                       \
    int rc_ = (x);           \
    if (rc_) return rc_;     \
  } while (0)
#define NEED(cond, msg)            \
  do {                             \
    if (!(cond)) {                 \
      ldsim_set_error("%s", msg);  \
      return LDSIM_EINVAL;         \
    }                              \
  } while (0)

// ---- owners of device objects ------------------------------------------------------------------------------------------
// Every device allocation, stream and event of the library is held by one of the three types below: they alone call the
// HIP create / destroy functions, and they alone move ldsim_live (device buffers, streams, events held process-wide:
// ldsim_debug_live_objects).  All three are move-only; a pointer or handle copied out of one is an alias and is marked so.
extern std::atomic<int64_t> ldsim_live[3];

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p; bytes = o.bytes;
      o.p = nullptr; o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) {
      (void)hipFree(p);
      ldsim_live[0]--;
    }
    p = nullptr;
    bytes = 0;
  }
  // kept when it holds `need` bytes, else freed and allocated again with headroom (contents lost); an empty buffer always
  // allocates, so ensure(0) still gives a valid pointer
  int ensure(size_t need) {
    if (need <= bytes && p) return 0;
    reset();
    const size_t want = need + need / 8 + 256;
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, want));
    p = q;
    bytes = want;
    ldsim_live[0]++;
    return 0;
  }
  // grown to hold at least `need` bytes, its first `keep` bytes kept (copied on `st`, which is drained before the old
  // allocation goes); untouched on failure
  int grow_keep(hipStream_t st, size_t keep, size_t need) {
    if (need <= bytes && p) return 0;
    DevBuf nb;
    CK(nb.ensure(need * 2));
    if (keep) HIPCHK(hipMemcpyAsync(nb.p, p, keep, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    *this = std::move(nb);
    return 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

// Page-locked host memory that device-to-host copies of a few words land in (a copy into pageable memory is staged by the
// runtime).  Host memory: not one of the ldsim_live counts.  Grown like a DevBuf, contents lost; no copy may be in flight then.
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { reset(); }
  void reset() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
  int ensure(size_t need) {
    if (need <= bytes && p) return 0;
    reset();
    const size_t want = need + need / 8 + 256;
    void* q = nullptr;
    HIPCHK(hipHostMalloc(&q, want, hipHostMallocDefault));
    p = q;
    bytes = want;
    return 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s) {
      (void)hipStreamDestroy(s);
      ldsim_live[1]--;
    }
  }
  // created on first use (priority 0: the default one)
  int ensure(unsigned flags = hipStreamDefault, int priority = 0) {
    if (s) return 0;
    if (priority) HIPCHK(hipStreamCreateWithPriority(&s, flags, priority));
    else HIPCHK(hipStreamCreateWithFlags(&s, flags));
    ldsim_live[1]++;
    return 0;
  }
  operator hipStream_t() const { return s; }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e) {
      (void)hipEventDestroy(e);
      ldsim_live[2]--;
    }
  }
  int ensure(unsigned flags = hipEventDefault) {   // created on first use
    if (e) return 0;
    HIPCHK(hipEventCreateWithFlags(&e, flags));
    ldsim_live[2]++;
    return 0;
  }
  operator hipEvent_t() const { return e; }
};

// photon sum without truth slots over a device-built list of the lit (detector, tick tile) cells (kernels_light.hip)
#define LIGHT_TILE 2048      // ticks of a tile (16 KB of f64 sums in LDS: the sum kernel finds room beside the charge chain's workgroups)
struct LightAct {
  unsigned long long* dmask;    // [n_det] tiles of a detector row already listed
  unsigned* count;              // entries in `list`
  int32_t* list;                // idet * ntile + tile
  int ntile;
  // the sum before this one into the same array (the other half of the buffer): its listed tiles are zeroed again, its masks
  // and its count reset, by the kernels of this sum (clear = 0: nothing to undo, the array was cleared whole)
  int clear, p_ntile;
  long long p_nticks;
  unsigned long long* p_dmask;
  unsigned* p_count;
  const int32_t* p_list;
};

struct ldsim_ctx {
  // The thread inside an entry point of this ctx (CtxEnter below): a ctx is thread-compatible, not thread-safe -- a second
  // thread entering while a call is in progress gets LDSIM_ESTATE before it touches any buffer (two threads in one ctx once
  // freed the same scratch buffer twice under running kernels: GPU memory access fault, gpurun_out/r03_h25.log).
  std::atomic<std::thread::id> owner{};
  int owner_depth = 0;          // entry points call each other (ldsim_ctx_create -> ldsim_set_consts ...): re-entrant for the owner
  int device = 0;
  // the streams come first: members go in reverse order, so every buffer and event is gone before the streams are
  hipStream_t stream = nullptr;              // the current stream (not owned): main_stream, or light_stream inside ldsim_dev_sum_light
  Stream main_stream, copy_stream, light_stream, tab_stream;
  LdsimConsts h_consts;
  DevBuf d_consts;
  // response table
  DevBuf d_resp;
  int32_t ni = 0, nj = 0, nk = 0;
  int32_t resp_k_first = 0, resp_k_last = -1;  // support of the table over all cells (exact zeros outside)
  // per-pixel discrimination thresholds / gains of the fused chain: dense tables indexed by pixel id (NULL = constant)
  DevBuf d_pix_thr, d_pix_gain;
  int64_t pix_table_n = 0;      // n_pixels[0] * n_pixels[1] * n_tpc the tables were built for
  // light
  DevBuf d_eff, d_ch2tpc;                    // f64, i32 per channel
  int32_t n_light_ch = 0;
  DevBuf resp_pad;                           // zero-padded copy of the response rows for mac_shift_kernel
  int32_t resp_pad_lo = 0, resp_pad_hi = -2; // staged range it was built for (-2: not built)
  double quad_n0 = 3.4, quad_slope = 1.38;   // Gauss-Legendre node rule N = ceil(n0 + slope * r): 1e-7 of the peak weight (option quad_accuracy_log10, tools/quad_sweep.py; 6 = 3.0 + 1.3 r is 3.7 % faster and fails the 2e-8 charge tests against the closed form)
  // overlapped download of the chain's results (ldsim_chain_download_async): a second stream copies launch k's per-pixel
  // arrays to the host while launch k + 1 computes into the other set of output buffers
  DevBuf light_wtid, light_wtph, light_wtid2;            // slot-major working copies of a response stage's output truth rows
  DevBuf light_xd;                           // a SiPM stage's input samples widened to doubles (light_widen_kernel): the launch's and the universes' passes, one after the other on the stream
  DevBuf light_env;                          // per offset of a wave's first tick from an input tick: the largest weight its 64 ticks meet it with (light_env_kernel)
  int light_truth_lds = 1;                   // truth slots of the light response stages by light_truth_lds_kernel (0, or more than 64 slots: light_truth_rows_kernel, slot-major copies in memory)
  DevBuf light_tmax;                         // per (detector, tick) bound on the truth slots' photons (light_truth_max_kernel)
  DevBuf out_alt[7];                         // the other set of SB_UPIX, SB_UBATCH, SB_ADC, SB_TICKS, SB_DIGIT, SB_TPM, SB_FRAC
  int async_out = 0;                         // alternate the output buffers from launch to launch (set by the first async download)
  int copy_pending = 0;
  int64_t out_gen = 0, pending_gen = 0;      // chain launches so far; the launch whose results the pending copy reads
  int light_eff_plain = 0;                   // every OP_CHANNEL_EFFICIENCY finite and >= 0
  int light_incidence_scalar = 0;            // 1 = the one-channel-per-lane light_incidence_kernel (A/B checks)
  int light_lut_interp = 0;                  // 1 = visibility interpolated trilinearly between voxel centres (light_incidence_interp*_kernel)
  int mac_mode = 1;                          // M = 1 correlation: 1 = mac_shift_kernel (DPP window), 0 = mac_kernel<1> (LDS rows)
  DevBuf d_lut_vis, d_lut_t0, d_lut_t0avg, d_lut_td;   // f32 planes
  int32_t lut_nx = 0, lut_ny = 0, lut_nz = 0, lut_ndet = 0, lut_nprof = 0;
  // options
  double prune_log = 23.0;                   // exp(-23) = 1e-10 of the pair's peak weight, the accuracy the node rule is fitted for
  double tail_log = 14.0;
  int trim_response = 1;
  double trim_response_log = 23.0;           // response ticks below exp(-v) of the table's largest entry are not read (0: exact zeros only)
  std::vector<double> h_resp_kmax;           // largest |entry| of every response tick over all cells (host)
  int debug_phases = 15;
  int debug_lds_b1_kb = 0;                   // timing tools: LDS budget of gcorr_kernel's second class in KB (0 = 32)
  int debug_lds_pad_kb = 0;                  // timing tools: KB taken off the LDS budget of gcorr_kernel's small class
  long long frac_clean_gen = -1;             // out_gen of the output set whose dense fractions array has been completed with zeros
  // launch constants of the FEE kernels (kernels_fee.hip fee_tables_kernel): wtap[64] | G[64], built for (fee_tab_dt, fee_tab_rt)
  DevBuf d_fee_tab;
  double fee_tab_dt = 0, fee_tab_rt = -1;
  int fee_one_class = 0;                     // option: 1 = pixel_adc_kernel with 256 threads and the whole tick axis for every pixel (A/B checks)
  int gform_chunks = 1;                      // tables and correlation of the node-separable form in this many pair ranges, the tables of range c + 1 on a second stream beside the correlation of range c (1: one after the other)
  Event tab_ev[34];                          // per-range events of that second stream (tab_stream)
  int gform_wave_tables = 1;                 // 1: gtables_wave_kernel (a wave per pair) for the pairs that fit it, 0: gtables_kernel for all
  int debug_gform = 0;                       // timing tools: parts of gtables_kernel / gcorr_kernel switched off (tools/gform_phases.py)
  // what gform_launch decided for the last current stage (ldsim_debug_gform_census counts the pairs from it); valid = 0 once
  // another current path ran: its GInfo array (SB_GINFO) and flags (SB_GFLAGS) are that path's then
  struct GformRecord {
    int valid = 0, M = 0, TT = 0, b0 = 0, b1 = 0, b2 = 0, Mz = 0, qb[3] = {0, 0, 0}, wave_tables = 1;
    int64_t n = 0;
    unsigned long long n_wg = 0, n_w2 = 0, n_cls[3] = {0, 0, 0};
    unsigned long long n_fused[2] = {0, 0};          // pairs gcorr_fused_kernel<1> / <2> were launched over
    const void *gi = nullptr, *flags = nullptr;      // (aliases of the two scratch buffers, compared only)
    const void* rec = nullptr;                       // (the record pool, SB_GREC: ldsim_debug_gform_fused reads the cell lists from it)
  } gform_rec;
  int split_kernels = 1;            // 1: weights_kernel + mac_kernel (default), 0: monolithic current_kernel
  int wbuf_doubles_per_pair = 6144; // initial average budget of the split path's weight pool, doubles per pair
  int split_max_items = 0;          // validation knob, see CurArgs
  int weights_mode = 2;             // split path: 2 = node-separable form (gtables_kernel + gcorr_kernel, gform.h), 1 = qweights_kernel (Gauss-Legendre along the segment) + mac kernel, 0 = weights_kernel (per-sample closed form) + mac kernel
  int gform_max_support = 1000000000;   // staged response support (ticks) up to which weights_mode 2 runs the node-separable form (round 4: every table -- with the 1e-7 node rule
                                        // the matrix form is ahead on full-support tables too, profiles/r04_dense_handover.log; 768 until then: wider tables took the shifted-window kernels)
  int mc_current = 0;               // 1: the chain's induced currents come from current_mc_kernel (tracks_current_mc) instead of tracks_current
  int numba_f32 = 0;                // 1: evaluate the sub-expressions Numba types f32 for f4 record fields in float
  DevBuf d_glx;                     // Gauss-Legendre nodes / weights on [-1, 1] for every N <= gl_nmax, rule N at N(N-1)/2
  DevBuf d_glw;
  int gl_nmax = 0;
  double wbuf_learned = 0;          // high-water demand per pair seen so far (x1.25): later calls size the pool with it
  int64_t n_fallback = 0;   // bit0: weights phase, bit1: correlation phase (timing experiments only)
  // resident segments
  SegStore seg{};
  DevBuf seg_block;
  DevBuf raw;          // AoS staging (H2D/D2H)
  LdsimTrackLayout seg_layout{};
  DevBuf scratch[40];  // named scratch buffers, grown on demand
  PinnedBuf readback;  // the words a launch reads back from the device between its stages (ChainReadback, ldsim_args.h)
  std::vector<int32_t> h_batch;   // host copy of the resident segments' batch ids (validated non-decreasing at upload)
  int seg_owner = 0;   // who filled the segment store last: 1 = ldsim_segments_upload (resident chain), 2 = a host-buffer stage call
  // device-resident light leg (ldsim_dev_light_incidence / ldsim_dev_sum_light)
  DevBuf light_nph, light_t0, light_vox;       // [n][light_n_out] f32, f32 (trigger mode 0 only), [n][3] i32 over all resident segments
  int32_t light_n_out = 0;
  int64_t light_n = -1;                        // resident segment count the incidence was computed for (-1 = not computed)
  DevBuf light_out, light_tid, light_tph, light_opc, light_trk;   // last photon sum: [n_det][n_ticks] f32, truth ids / photons
  int32_t light_sum_ndet = 0, light_sum_nticks = 0, light_sum_truth = 0;
  DevBuf light_tmp[9];
  // lazy clear of the resident photon-sum arrays (ldsim_dev_sum_light): valid = the arrays are clean over `light_clean_cells`
  // (detector, tick) cells except where the records still sorted in light_tmp[4] fell
  int light_lazy_valid = 0, light_lazy_mt = 0, light_lazy_tick_bits = 16;
  long long light_lazy_nrec = 0, light_lazy_nticks = 0;
  DevBuf light_flag_dev;                 // 8 bytes of device memory for that flag (sticky until read)
  unsigned* light_emit_flag = nullptr;   // (alias of light_flag_dev) device word of the last compact photon sum: a pair ran out of record slots (checked at the next synchronising light call)
  size_t light_clean_cells = 0, light_lazy_cap[3] = {0, 0, 0};
  void *light_lazy_out = nullptr, *light_lazy_tid = nullptr, *light_lazy_tph = nullptr;   // (aliases of light_out / light_tid / light_tph, compared only)
  // the same for a sum without truth slots: clean except the tiles in light_act's list (LightAct; geometry of that sum below)
  DevBuf light_act;                            // two halves (this sum's, the previous one's) of: [cap] u64 masks, count u32, list i32
  int light_nt_valid = 0, light_nt_ntile = 0, light_nt_ndet_cap = 0, light_nt_half = 0, light_nt_list_cap = 0;
  long long light_nt_nticks = 0;
  void* light_nt_out = nullptr;                // (alias of light_out, compared only)
  size_t light_nt_cap = 0;
  int32_t h_opc_n_out = 0;
  int light_sum_no_list = 0;                   // option: 1 = the grid over every (detector, tile) and a full clear (A/B checks)
  std::vector<int32_t> h_opc;                  // host copy of light_opc's contents (validated once, re-sent only when it changes)
  // option light_sum_async: the sums without truth slots run on a stream of their own, beside whatever the ctx's stream carries
  // next (the charge chain).  light_pending: the last such sum has not been joined into ctx->stream yet (light_join, ldsim_abi.hip)
  Event ev_light_in, ev_light_done;
  int light_async = 0, light_pending = 0;
  int light_sum_timed = 1;                     // 0: evl[2..3] of the last sum not yet read into ms_light_sum
  // resident waveform stages on the last photon sum (ldsim_dev_light_response): scintillation profile (+ truth), Poisson
  // fluctuated rate, detector response (+ truth), all [light_sum_ndet][light_sum_nticks]
  DevBuf light_scint, light_scint_tid, light_scint_tph, light_disc, light_resp, light_resp_tid, light_resp_tph, light_w[2],
      light_gain;
  int light_resp_valid = 0;
  uint64_t light_noise_calls = 0;
  double ms_light_resp[3] = {0, 0, 0};
  double ms_light_inc = 0, ms_light_sum = 0;
  Event evl[4];
  // light universes (ldsim_dev_light_universes): the photon sum under varied light constants.  Universes are grouped on the host
  // (lu_in / lu_sc / lu_rs: per universe the index of its scaled input, its scintillation + fluctuation stage and its response;
  // equal constants share one), every distinct array is [lu_D][lu_T] f32 at a stride of lu_bo elements
  DevBuf lu_x;                   // inputs scaled by a photon_scale other than 1.0 (1.0 reads light_out itself)
  DevBuf lu_scint, lu_disc;      // distinct scintillation profiles and their fluctuated counts (lu_disc unused without fluctuations)
  DevBuf lu_resp;                // distinct detector responses
  DevBuf lu_tab;                 // weight tables f64 [n_sc + n_rs][C + 1] | row gains f64 [n_rs][lu_D]
  DevBuf lu_digit;               // waveforms of the last ldsim_dev_light_universe_waveforms, f64 [n_trig][n_det_trig][samples]
  int lu_valid = 0, lu_keep = 0, lu_fluct = 0;
  int32_t lu_n = 0, lu_D = 0, lu_T = 0;
  size_t lu_bo = 0;
  std::vector<int32_t> lu_in, lu_sc, lu_rs;
  int lu_nu = 4;                 // option light_universes_nu: tables per launch of light_plain_kernel, 1 .. 4
  Event lu_ev[4];                // around the scintillation, fluctuation and response stages of the last pass
  double ms_lu[3] = {0, 0, 0};
  // light LUT builder (ldsim_light_lut_build / _trace, kernels_lutbuild.hip): staged rectangles, the tallies of the last build's
  // voxel range, the last trace's photons
  DevBuf lb_dets;                // LutRect [ndet] grouped by wall | i32 [ndet] their indices in the caller's list
  DevBuf lb_counts, lb_hist, lb_tmin, lb_tsum, lb_fates;   // u32 [nv][ndet] | u32 [nv][ndet][nprof] | f32 bits [nv][ndet] | u64 [nv][ndet] | u64 [nv][3]
  DevBuf lb_trace;               // fate i32 [n] | steps i32 [n] | time f64 [n] | end f64 [n][3]
  int lb_group = 4096;           // option lut_build_group_photons: photons a workgroup walks
  int lb_tile = 1;               // option lut_build_lds_tile: 0 sends every arrival to global atomics (the path of a tile too big for LDS)
  Event lb_ev[2];                // around lut_build_kernel of the last build (ldsim_light_lut_build_ms)
  double ms_lb = 0;
  // field-response builder (ldsim_response_build, kernels_respbuild.hip): the last build's table
  DevBuf rb_table;               // f64 [n_i][n_j][n_k]
  Event rb_ev[2];                // around response_build_kernel of the last build (ldsim_response_build_ms)
  double ms_rb = 0;
  // drift-field map builder (ldsim_field_map_solve / _trace, kernels_fmapbuild.hip)
  DevBuf fb_vec;                 // the solve's vectors, f64 [6][nodes]: source | psi | r | A p | p of even | p of odd iterations
  DevBuf fb_part;                // chunk partials f64 [2][chunks]: |r|^2 | p . A p
  DevBuf fb_state;               // FbState: the CG scalars, which stay on the device between the host's reads
  DevBuf fb_field;               // the trace's node field, 32-byte (Ex, Ey, En, |E|) [nodes]; psi f64 [nodes] behind it
  DevBuf fb_out;                 // the trace's results: E | dx | dy | dz f64 [4][nodes] | the reversal word u32 (+ pad) | flags u8 [nodes]
  int fb_wgs = 0;                // option fmap_build_wgs: workgroups of the solve's kernels (0: one per chunk, 1024 at the most)
  Event fb_ev[6];                // around the solve, the field kernel and the trace kernel of the last calls (ldsim_field_map_build_ms)
  double ms_fb[3] = {0, 0, 0};
  // track generator (ldsim_track_gen_count / ldsim_track_gen, kernels_trackgen.hip): the primaries and per-primary results of the
  // last count pass (kept for the write pass over the same input: tg_hash), the last write pass's columns
  DevBuf tg_prim;                // LdsimTrackGenPrimary [n]
  DevBuf tg_counts, tg_off;      // u64 [n] segments per primary | their exclusive scan
  DevBuf tg_state, tg_end;       // i32 [n] end states | f64 [n][6] end point, end time, path, remaining T
  DevBuf tg_f64, tg_i32;         // f64 [LDSIM_TRACK_GEN_NF64][total] | i32 [LDSIM_TRACK_GEN_NI32][total]
  int tg_group = 0;              // option track_gen_group_primaries: primaries a workgroup walks (0: chosen from the list's length)
  int tg_valid = 0;              // the count pass's results belong to (tg_hash, tg_n)
  uint64_t tg_hash = 0;          // fold of (parameters, primaries, seed) of the last count pass
  int64_t tg_n = 0, tg_total = 0;
  Event tg_ev[2];                // around gen_kernel<true> of the last write pass (ldsim_track_gen_ms)
  double ms_tg = 0;
  // track cascade (ldsim_track_cascade_count / ldsim_track_cascade, kernels_trackgen.hip): one generation's particles and the
  // per-particle results of the last count pass (kept for the write pass over the same input: tc_hash), the last write pass's output
  DevBuf tc_part;                // LdsimTrackGenParticle [n]
  DevBuf tc_counts, tc_off;      // u64 [2][n] segments | secondaries per particle, and the exclusive scan of each row
  DevBuf tc_state, tc_end;       // i32 [n] end states | f64 [n][6] end point, end time, path, remaining T
  DevBuf tc_f64, tc_i32;         // f64 [LDSIM_TRACK_GEN_NF64][total] | i32 [LDSIM_TRACK_GEN_NI32][total]
  DevBuf tc_sec;                 // LdsimTrackGenParticle [secondaries]
  int tc_valid = 0;              // the count pass's results belong to (tc_hash, tc_n)
  uint64_t tc_hash = 0;          // fold of (parameters, cascade parameters, particles, seed) of the last count pass
  int64_t tc_n = 0, tc_total = 0, tc_stotal = 0;
  Event tc_ev[2];                // around cas_kernel<true> of the last write pass (ldsim_track_cascade_ms)
  double ms_tc = 0;
  // random streams (kernels_rng.hip): numba-style table of xoroshiro128p states, grown on demand
  DevBuf d_rng;
  int64_t rng_n = 0;
  uint64_t rng_seed = 0, rng_last_init[2] = {0, 0};
  int rng_seeded = 0;
  // keyed mode (ldsim_rng_keyed_seed, rng.h): no table; every draw is Philox of (rng_seed, stage, identity key, index).
  // rng_batch_keys: one key per batch id of the upload (ldsim_chain_set_batch_keys); rng_call_key: identity of the light calls
  int rng_keyed = 0;
  uint64_t rng_call_key = 0;
  DevBuf d_batch_keys;
  int64_t rng_batch_keys_n = 0;
  int debug_rng_materialize = 0;     // option: keyed FEE normals written to the noise table and read by the table scan (tests)
  // drift-field maps (ldsim_set_field_map), keyed by the global TPC index: they outlive ldsim_set_consts
  FieldMapDesc h_fmap[LDSIM_MAX_TPC] = {};
  DevBuf fmap_nodes[LDSIM_MAX_TPC];
  DevBuf d_fmap;                         // device copy of h_fmap (while a map is set)
  int n_fmap = 0;                        // TPCs with a map
  int64_t fmap_gen = 0;                  // advances on every set / clear
  int64_t drift_map_gen = -1;            // fmap_gen of the mapped quench_drift whose results the store holds (-1: none)
  DevBuf fmap_view;                      // [LDSIM_NVIEW][fmap_view_cap] anode-view columns (allocated while a map is set)
  int64_t fmap_view_cap = 0;
  // charge statistics (ldsim_set_charge_statistics): counted ion pairs, binomial recombination and attachment in the
  // resident quench_drift (quench_drift_stat_kernel); needs keyed mode and batch keys
  int charge_stat = 0;
  double charge_stat_fano = 0.107;
  int drift_stat_on = -1;                // setting of the quench_drift whose results the store holds (-1: none since the upload)
  double drift_stat_fano = 0;
  DevBuf d_stat_first;                   // [batches of the upload] i32 first segment index of every batch over the whole store
  // SiPM correlated noise (ldsim_set_sipm_noise): cross-talk, after-pulses and dark counts in the keyed fluctuation stage
  // (light_sipm_count_kernel, light_wvfm.hip)
  int sipm_on = 0;
  LdsimSipmNoise sipm = {0, 0, 0.1, 0};
  DevBuf sipm_counts;                    // i32 avalanche counts of the array being fluctuated (zeroed, summed by atomics, converted)
  // multi-GPU exchange (comm.hip): RCCL communicator, rows accumulated over the chain calls of a pass, gathered rows
  void* comm = nullptr;
  int comm_rank = 0, comm_world = 0;
  DevBuf comm_tmp, hits_acc, hits_all;
  int64_t hits_acc_rows = 0;
  // compact results of a rank's launches (ldsim_compact_accumulate) and root's gather of them; gather-v of host bytes
  DevBuf cpt_acc[5], cpt_all[5], gv_send, gv_all;
  int64_t cpt_acc_n[5] = {0, 0, 0, 0, 0};
  int64_t cpt_acc_gen = -1;                   // chain launch whose compact parts were appended last
  int64_t cpt_all_n[5] = {0, 0, 0, 0, 0};     // element counts of the one rank's stream root holds
  std::vector<int64_t> gv_all_n;              // [world] bytes of the last gather-v
  int cpt_all_root = -1, cpt_all_src = -1;    // root and source rank of the last compact gather (-1: none)
  int gv_all_root = -1;                       // root of the last gather-v (-1: none)
  // chain results
  LdsimChainStats stats{};
  LdsimChainStats stage_stats{};   // counters of the last ldsim_tracks_current stage call (ldsim_tracks_current_stats)
  int64_t chain_U = 0, chain_hits = 0;
  int64_t cpt_n[4] = {0, 0, 0, 0};   // compact result of the last ldsim_chain_compact_build: hit pixels, hits, track entries, fraction entries
  int64_t cpt_gen = -1;              // chain launch it was built for
  int want_fractions = 0;
  // pixel charge truth (ldsim_chain_pixel_truth, kernels_pixtruth.hip) reads what the last chain launch left in the scratch
  // buffers, through chain_view: the current rows, the FEE set-up record (headers, slot rows), upix, ubatch, adc, tpm and the
  // hit counts.  launch_stale = nullptr while all of them are that launch's: set by a
  // successful ldsim_charge_chain, and named again (launch_invalidate) by every entry point that may rewrite or regrow one
  const char* launch_stale = "no ldsim_charge_chain has run on this context";
  struct FeeRecord {             // the set-up record fee_launch_chain left (fee_record.h) and the sizes the launch ran with
    int lists;                   // 0: headers [U], header u at index u; 1: lists [2][U] | counts u64 [2] behind them
    int64_t U, n_pairs;
    int32_t T, NT, M, A;
    double dt;
  } fee_rec{};
  DevBuf pt_dense;               // last pass: q_induced f64 [U] | q_abs f64 [U] | q_track f64 [U][M] | n_slots i32 [U]
  DevBuf pt_sel;                 // keep flags, entry counts and their exclusive scans, i32 [4][U] | the u64 of the sample count
  DevBuf pt_out;                 // compact form: pixel rows (LdsimPixelTruthRow) | track entries (LdsimPixelTruthTrack)
  int64_t pt_gen = -1;           // chain launch (out_gen) the last pass ran on (-1: none)
  int64_t pt_U = 0, pt_n[2] = {0, 0};   // rows of the dense arrays; kept pixels and track entries of the compact form
  int32_t pt_M = 0;
  // pixel current waveforms (ldsim_chain_pixel_waveforms, kernels_pixwave.hip) read the same launch under the same rule
  DevBuf pw_sel;                 // u64 [4][U + 1]: span counts | sample counts | their exclusive scans (place U: the totals)
  DevBuf pw_out;                 // compact form: span rows (LdsimPixelWaveSpan) | samples f32
  DevBuf pw_dense;               // rows of the last ldsim_chain_pixel_waveforms_dense, f32 [u_end - u_begin][N_t]
  int64_t pw_gen = -1;           // chain launch (out_gen) the last pass ran on (-1: none)
  int64_t pw_n[2] = {0, 0};      // spans and samples of the compact form
  Event pw_ev[4];                // around the count kernel and around the fill kernel of the last pass (ldsim_chain_pixel_waveforms_ms)
  bool pw_filled = false;        // the last pass launched its fill kernel
  // FEE universes (ldsim_chain_fee_universes, kernels_feeuni.hip) read the same launch under the same rule
  DevBuf fu_dense;               // adc_list | adc_ticks | adc_digit, each f64 [n][U][A]
  DevBuf fu_cnt;                 // hit_count i32 [n][U] | hit_off i32 [n][U] | totals i64 [n] | error word
  DevBuf fu_uni;                 // the universes' constants [n] | their tap tables f64 [n][128]
  DevBuf fu_rows;                // compact form: 24-byte hit rows of all universes, universe after universe | their charges f64
  int64_t fu_gen = -1;           // chain launch (out_gen) the last pass ran on (-1: none)
  int32_t fu_n = 0, fu_A = 0;    // universes and MAX_ADC_VALUES of the last pass
  int64_t fu_U = 0;              // rows of its dense arrays
  std::vector<int64_t> fu_hits, fu_row0;   // [n] hits of every universe; [n + 1] its first row in fu_rows
  Event fu_ev[2];                // around pixel_adc_universes_kernel of the last pass (ldsim_chain_fee_universes_ms)
  bool fu_timed = false;         // the last pass launched the kernel
  // charge universes (ldsim_chain_universes with charge variations, kernels_feeuni.hip): the same pass with per-segment weights
  int drift_mode = 0;            // recombination mode of the ldsim_dev_quench_drift whose charge the store holds (0: none recorded)
  int64_t launch_seg[2] = {0, 0};   // segment range of the last ldsim_charge_chain
  DevBuf cu_w;                   // weights f64 [groups][segments of the launch] | unweightable counts | constants | grouping (cu_parts_of)
  DevBuf cu_S;                   // rows of the last ldsim_chain_universe_waveforms_dense, f64 [u_end - u_begin][N_t]
  std::vector<int32_t> cu_group; // [n] the charge group of every universe of the last pass (empty: it had no charge variations)
  std::vector<unsigned long long> cu_unw;   // [groups] segments with n_res == 0 and n_k != 0
  int64_t cu_nseg = 0;           // segments the weights cover
  Event cu_ev[2];                // around charge_weights_kernel of the last pass (ldsim_chain_universes_weights_ms)
  bool cu_timed = false;
  Event ev[8];
  double ms_current = 0, ms_adc = 0, ms_total = 0;
  double ms_weights = 0, ms_mac = 0, ms_fallback = 0;   // split path: per-kernel share of ms_current
};

// scratch slots, named for what they hold.  A slot shared by two paths that never run in the same stage carries both names
// (one index, one buffer); the layouts inside a slot are in ldsim_args.h (ChainMisc, batch_block, hit_counts) and
// fee_record.h (fee_hdr_view), and chain_view (ldsim_args.h) gives what a chain launch left as typed pointers.
enum {
  SB_ACTIVE = 0, SB_NEIGH, SB_NRAD,
  SB_NLIST,                          // get_pixels stage call: n_list f64 [n]
  SB_STARTS,
  SB_MISC,                           // ChainMisc, and behind it the chain's per-batch block (batch_block)
  SB_KEYS, SB_KEYS2, SB_VALS, SB_VALS2, SB_SORTTMP,
  SB_PIXOFF,                         // uoff i64 [U + 1]: a unique pixel's first pair in the sorted list
  SB_HITCNT,                         // hit_count i32 [U] | hit_off i32 [U] (hit_counts)
  SB_HEADS,
  SB_UIDX,                           // exclusive scan of the heads: a pair's unique-pixel index
  SB_UPIX, SB_UBATCH, SB_WAVES, SB_ADC, SB_TICKS, SB_DIGIT, SB_TPM, SB_FRAC, SB_HITS,
  // shifted-window split path | node-separable form (gform_launch):
  SB_ITEMS, SB_GFLAGS = SB_ITEMS,    //   items                | fallback flags i32 [n]
  SB_HDR, SB_GINFO = SB_HDR,         //   pair headers         | GInfo [n]
  SB_CORR, SB_GSIZES = SB_CORR,      //   corrections          | record offsets, class counts and lists
  SB_WBUF, SB_GREC = SB_WBUF,        //   weight pool          | table records
  SB_NOISE, SB_NDRAWS, SB_PPAR, SB_CPT, SB_CPO, SB_WIN,
  SB_FEEHDR,                         // FEE set-up record: headers (fee_hdr_view)
  SB_GMAPS,
  SB_FEESLOT                         // FEE set-up record: slot rows, indexed like the sorted pair list
};

// the segment store the charge kernels read: after a mapped quench_drift its nine position columns are the anode view
static inline SegStore charge_store(const ldsim_ctx* ctx) {
  SegStore s = ctx->seg;
  if (ctx->drift_map_gen >= 0)
    for (int k = 0; k < LDSIM_NVIEW; k++) s.f[k] = (double*)ctx->fmap_view.p + (size_t)k * ctx->fmap_view_cap;
  return s;
}
// the scratch buffers no longer hold (or may no longer hold) the last chain launch: `by` names the call, for the refusal
static inline void launch_invalidate(ldsim_ctx* ctx, const char* by) { ctx->launch_stale = by; }
// refusal of a host-array stage call that draws random numbers while the ctx is in keyed mode (its rows have no identity)
#define LDSIM_KEYED_STAGE_MSG \
  "%s draws random numbers, but the context is in keyed mode and this stage call carries no identity for its rows: " \
  "call ldsim_rng_seed for table mode"


// Claims the ctx for the calling thread for the duration of an extern "C" entry point.
struct CtxEnter {
  ldsim_ctx* c;
  bool ok;
  explicit CtxEnter(ldsim_ctx* ctx) : c(ctx), ok(true) {
    if (!c) return;                                  // (the entry point's own argument check reports a null ctx)
    const std::thread::id me = std::this_thread::get_id();
    if (c->owner.load(std::memory_order_acquire) == me) {
      c->owner_depth++;
      return;
    }
    std::thread::id none{};
    ok = c->owner.compare_exchange_strong(none, me, std::memory_order_acq_rel);
    if (ok) c->owner_depth = 1;
  }
  ~CtxEnter() {
    if (c && ok && --c->owner_depth == 0) c->owner.store(std::thread::id{}, std::memory_order_release);
  }
  CtxEnter(const CtxEnter&) = delete;
  CtxEnter& operator=(const CtxEnter&) = delete;
};
#define LDSIM_ENTER(ctx)                                                                                      \
  CtxEnter enter_(ctx);                                                                                       \
  if (!enter_.ok) {                                                                                           \
    ldsim_set_error("ctx in use by another thread (a ctx is thread-compatible, not thread-safe: one per thread)"); \
    return LDSIM_ESTATE;                                                                                      \
  }
