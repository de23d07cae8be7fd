// kernels_feeuni.hip -- FEE universes: the last chain launch digitised again under varied front-end constants
// (include/ldsim.h, "FEE universes"; the Python side: larndsim_amd/fee_universes.py).
//
// A sibling of kernels_pixtruth.hip and kernels_pixwave.hip: it reads what the launch left in HBM -- the per-pair current rows
// (f32 [n_pairs][T]) and the FEE set-up record (fee_record.h, through fee_reader.h) -- and changes nothing of the chain.  A launch spends its time on
// those rows; the front end (fee_setup_kernel + the pixel_adc kernels) only reads them, so a variation of the front end needs
// no second launch.
//
// pixel_adc_universes_kernel, one 256-thread workgroup per unique pixel:
//   sum    S[t] over the whole tick axis in LDS, once, exactly as pixel_adc_body's 256-thread form: f64, the slots' f32 rows
//          added in slot order, each over its window clipped to [0, N_t), a thread owning the ticks t = tid mod 256
//   scan   where pixel_adc_body scans on wave 0 while three waves wait, wave w scans universe 4 g + w (groups g = 0, 1, ...)
//          over the same S with the same adc_scan (fee_scan.h): its own FeeK through a pointer, its own taps, its own HitRec [A],
//          its own threshold and gain.  adc_scan holds no workgroup barrier and S is read-only from here on, so the waves run
//          their groups independently: a universe with noise (every tick walked) does not hold up its neighbours.
//   noise  the inline keyed source only (KeyedNoise of the pixel's stream): all universes of a pixel see the same normals and
//          scale them by their own charges
//   write  adc_list / adc_ticks / adc_digit [n][U][A] and hit_count [n][U] in buffers of the pass; nothing else -- not the
//          launch's output slots, not track_pixel_map, not the launch counters, not the launch's tap table
// then per universe the launch's own exclusive scan and compact_hits_kernel (sort.hip) make the 24-byte hit rows.
//
// Charge universes (include/ldsim.h, "charge universes"; larndsim_amd/charge_universes.py) are the same pass with one weight per
// segment: charge enters a current row as one linear factor, so a universe that only changes how many electrons a segment
// delivers is the launch's rows times w = n_k / n_res.  charge_weights_kernel replays the quench/drift's two truncating stores of
// n_electrons under every distinct charge variation of the call (seg_charge.h); pixel_adc_universes_kernel<true> forms one
// weighted S per group of equal charge variations and scans the group's universes on it.  Not varied: e_field and v_drift (they
// set the drift times: where the rows sit on the time axis), the diffusion constants (the rows' shapes), lar_density (redundant
// with birks_kb and box_beta), w_ph and the light leg (n_photons is not re-weighted).
#include <math.h>
#include <string.h>

#include <vector>

#include "launchers.h"
#include "fee_reader.h"
#include "fee_scan.h"
#include "seg_charge.h"

#define FU_THREADS 256
#define FU_WAVES 4
#define FU_NT_MAX 4096   // ticks of S in LDS (32 KB)
#define FU_A_MAX 64
#define FU_M_MAX 64      // (fee_rec_header refuses a header with more slots)

// one universe on the device: the constants the scan and the digitisation read, and what the pixel tables are transformed by
struct FuUni {
  FeeK k;
  double threshold;                         // DISCRIMINATION_THRESHOLD * e
  double thr_scale, thr_offset, gain_scale; // pixel tables: thr_table[pix] * thr_scale + thr_offset, gain_table[pix] * gain_scale
  int32_t noisy, pad;                       // a noise charge is non-zero: the scan draws
};

struct FuArgs {
  FeeRecArgs rec;                           // the launch's record
  const int32_t* upix;
  int32_t A;
  // the universes
  int32_t n;
  const FuUni* uni;                         // [n]
  const double* tabs;                       // [n][128]: fee_tables_kernel's wtap[64] | G[64] of the universe's rise time
  const double* thr_table;                  // [n_pix_ids] or NULL, as the launch read them
  const double* gain_table;
  int64_t n_pix_ids;
  const uint64_t* batch_keys;               // [n_keys]; read by universes with noise only
  int64_t n_keys;
  uint64_t seed;
  double time_padding;
  // outputs, all buffers of the pass
  double *adc_list, *adc_ticks, *adc_digit; // [n][U][A]
  int32_t* hit_count;                       // [n][U]
  int32_t* err;                             // sticky: 1 = a header does not describe the launch's buffers, 2 = a pixel id outside the
                                            // tables, 3 = a batch without key
  // charge universes (the WEIGHTED instance only)
  const double* w;                          // [n_groups][n_seg] segment weights of the distinct charge variations
  const int32_t* grp;                       // group begins [n_groups + 1] | universes ordered by group [n]
  int64_t n_seg;                            // segments of the launch's range
  int32_t n_groups, pad2;
};

__device__ __forceinline__ void fu_wave_sync() {      // (LDS traffic of one wave is in order: only the compiler has to be held)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---- the pixel of a workgroup, in the scan kernel and in fu_dense_kernel: its header by fee_rec_header, its slots' windows by
// fee_slot_window (fee_reader.h) into LDS ---------------------------------------------------------------------------------------
// S[t] over the whole tick axis, by all 256 threads: each thread owns ticks tid, tid + 256, ... and adds the slots' rows in slot
// order.  WEIGHTED: every sample times its slot's weight s_wt[k], the product rounded before it is added.  s_start / s_lo / s_hi
// (and s_wt) may have been written just before the call: the first barrier orders them.  The workgroup-level LDS form of this
// file: one row per trip to memory; pixel_adc_body's grouped row loads (fee_row_load, FEE_LG) and its LDS form are not shared
// with it, which would change speed and wants a measurement of its own.
template <bool WEIGHTED>
__device__ __forceinline__ void fu_form_S(double* S, const float* waves, int64_t p0, int T, int NT, int n_slots, const int* s_start,
                                          const int* s_lo, const int* s_hi, const double* s_wt, int tid) {
  for (int t = tid; t < NT; t += FU_THREADS) S[t] = 0;
  __syncthreads();
  for (int k = 0; k < n_slots; k++) {
    const int lo = s_lo[k], hi = s_hi[k];
    const float* wf = waves + (p0 + k) * (int64_t)T - s_start[k];
    if constexpr (WEIGHTED) {
      const double wk = s_wt[k];
      for (int t = lo + ((tid - lo) & (FU_THREADS - 1)); t < hi; t += FU_THREADS) S[t] += __dmul_rn(wk, (double)wf[t]);
    } else {
      for (int t = lo + ((tid - lo) & (FU_THREADS - 1)); t < hi; t += FU_THREADS) S[t] += (double)wf[t];
    }
  }
  __syncthreads();
}

// WEIGHTED = false: the FEE universes of one S.  WEIGHTED = true (charge universes): the universes come in groups of equal
// charge variation (F.grp: group g holds the universes order[gb[g]] .. order[gb[g + 1] - 1]); per group the workgroup forms S_g
// from the rows times the group's segment weights, and wave w scans the group's universes w, w + 4, ...  Both barriers of a
// group (the one that closes fu_form_S, the one before the next group overwrites S) sit outside the waves' scan loops.
template <bool WEIGHTED>
__global__ void __launch_bounds__(FU_THREADS) pixel_adc_universes_kernel(FuArgs F) {
  extern __shared__ double S[];             // [N_t]: sized at launch
  __shared__ HitRec hits[FU_WAVES][FU_A_MAX];
  __shared__ double taps[FU_WAVES][64];
  __shared__ int s_start[FU_M_MAX], s_lo[FU_M_MAX], s_hi[FU_M_MAX];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NT = F.rec.NT, A = F.A, T = F.rec.T;
  const int64_t U = F.rec.U;
  const int64_t w = blockIdx.x;
  if (w >= U) return;
  FeeHdr H;
  int n_slots;
  if (!fee_rec_header(F.rec, w, H, n_slots)) {      // (nothing outside the buffers is touched; the host refuses the result)
    if (tid == 0) *F.err = 1;
    return;
  }
  const int64_t u = H.u, p0 = H.p0;
  [[maybe_unused]] int64_t my_seg = 0;      // WEIGHTED: the segment of slot tid, relative to the launch's range
  if (tid < n_slots) {
    const FeeSlot sl = F.rec.slots[p0 + tid];
    const FeeWindow W = fee_slot_window(sl, T, NT);
    s_start[tid] = W.st;
    s_lo[tid] = W.lo;
    s_hi[tid] = W.hi;
    if constexpr (WEIGHTED) my_seg = (int64_t)H.bfirst + sl.track;
  }
  if constexpr (WEIGHTED) {                 // a segment outside the launch's range: the record does not fit.  Nothing is indexed
    if (my_seg < 0 || my_seg >= F.n_seg) {  // with it (weight 0 of the range's first segment instead), the host refuses the result
      *F.err = 1;
      my_seg = 0;
    }
  }
  const int32_t pix = F.upix[u];
  const bool tabled = F.thr_table || F.gain_table;
  const bool pix_ok = !tabled || (pix >= 0 && pix < F.n_pix_ids);
  const double thr_pix = F.thr_table && pix_ok ? F.thr_table[pix] : 0.0;
  const double gain_pix = F.gain_table && pix_ok ? F.gain_table[pix] : 0.0;
  const bool key_ok = H.ubatch >= 0 && H.ubatch < F.n_keys;
  double* wtap = taps[wv];
  HitRec* my_hits = hits[wv];
  // ---- per group (one, without weights): S by the workgroup; then the scans: wave wv takes the group's universes wv, wv + 4, ... --
  [[maybe_unused]] double* s_wt = nullptr;
  if constexpr (WEIGHTED) {
    __shared__ double wt[FU_M_MAX];
    s_wt = wt;
  }
  const int n_groups = WEIGHTED ? F.n_groups : 1;
  for (int g = 0; g < n_groups; g++) {
    int j0 = 0, j1 = F.n;
    if constexpr (WEIGHTED) {
      j0 = F.grp[g];
      j1 = F.grp[g + 1];
      if (tid < n_slots) s_wt[tid] = F.w[(int64_t)g * F.n_seg + my_seg];
    }
    fu_form_S<WEIGHTED>(S, F.rec.waves, p0, T, NT, n_slots, s_start, s_lo, s_hi, s_wt, tid);
    for (int j = j0 + wv; j < j1; j += FU_WAVES) {
      const int k = WEIGHTED ? F.grp[F.n_groups + 1 + j] : j;   // (results are written at the caller's universe index)
      const FuUni* V = F.uni + k;
      const FeeK* c = &V->k;
      if (!pix_ok || (V->noisy && !key_ok)) {
        if (lane == 0) *F.err = pix_ok ? 3 : 2;
        continue;                           // (no workgroup barrier inside this loop: the group's barrier is behind it)
      }
      const double dt = c->time_sampling, rt = c->buffer_risetime;
      const int ntap = rt > 0 ? (int)ceil(10 * rt / dt) : 0;  // floor(ic - 10*rt/dt) == ic - ceil(10*rt/dt)
      wtap[lane] = F.tabs[(int64_t)k * 128 + lane];
      fu_wave_sync();
      // (two roundings each, as the same transformation of the tables on the host has; the tables are optional and marked
      // unlikely: a non-null pointer counts as the likely side, and the path without tables then sits out of line, which cost
      // 0.04 ms per universe and wave at 195 k pixels)
      const double thr = __builtin_expect(F.thr_table != nullptr, 0) ? __dadd_rn(__dmul_rn(thr_pix, V->thr_scale), V->thr_offset) : V->threshold;
      const double gain = __builtin_expect(F.gain_table != nullptr, 0) ? __dmul_rn(gain_pix, V->gain_scale) : c->gain * (1e-3 * (1e-6 * 1.0)) / 1.0;   // GAIN * mV / e
      int nd = 0, nh;
      // S holds every tick (s_lo = 0, s_hi = N_t); idle skipping by the header's [t_lo, t_hi) is adc_scan's own rule, per universe
      if (V->noisy) {
        const KeyedNoise zs{F.seed, key_mix(F.batch_keys[H.ubatch], (uint64_t)(int64_t)pix)};
        nh = adc_scan(c, S, NT, 1 * c->time_interval1, thr, F.time_padding, lane, my_hits, wtap, ntap, zs, &nd, H.t_lo, H.t_hi, 0, NT);
      } else {
        const TableNoise zs{nullptr};
        nh = adc_scan(c, S, NT, 1 * c->time_interval1, thr, F.time_padding, lane, my_hits, wtap, ntap, zs, &nd, H.t_lo, H.t_hi, 0, NT);
      }
      fu_wave_sync();
      const int64_t row = ((int64_t)k * U + u) * A;
      for (int h = lane; h < A; h += 64) {
        const double q = h < nh ? my_hits[h].q : 0.0;
        F.adc_list[row + h] = q;
        F.adc_ticks[row + h] = h < nh ? my_hits[h].tick : 0.0;
        F.adc_digit[row + h] = digitize_one(c, q, gain);
      }
      if (lane == 0) F.hit_count[(int64_t)k * U + u] = nh;
      fu_wave_sync();                       // (the next universe's scan writes the same HitRec and taps)
    }
    if constexpr (WEIGHTED) __syncthreads();   // (the next group overwrites S and the weights)
  }
}

// f64 S of the rows [u_begin, u_end), formed by fu_form_S as the scan kernel forms it: plain (w = NULL), or with the weights of
// one charge group.  A workgroup per header; the headers outside the range leave at once.
template <bool WEIGHTED>
__global__ void __launch_bounds__(FU_THREADS) fu_dense_kernel(FuArgs F, const double* __restrict__ wts, int64_t u_begin,
                                                              int64_t u_end, double* __restrict__ out) {
  extern __shared__ double S[];
  __shared__ int s_start[FU_M_MAX], s_lo[FU_M_MAX], s_hi[FU_M_MAX];
  __shared__ double s_wt[FU_M_MAX];
  const int tid = threadIdx.x;
  const int64_t w = blockIdx.x;
  const int T = F.rec.T, NT = F.rec.NT;
  if (w >= F.rec.U) return;
  FeeHdr H;
  int n_slots;
  if (!fee_rec_header(F.rec, w, H, n_slots)) {
    if (tid == 0) *F.err = 1;
    return;
  }
  if (H.u < u_begin || H.u >= u_end) return;
  int64_t my_seg = 0;
  if (tid < n_slots) {
    const FeeSlot sl = F.rec.slots[H.p0 + tid];
    const FeeWindow W = fee_slot_window(sl, T, NT);
    s_start[tid] = W.st;
    s_lo[tid] = W.lo;
    s_hi[tid] = W.hi;
    my_seg = (int64_t)H.bfirst + sl.track;
  }
  if constexpr (WEIGHTED) {
    if (my_seg < 0 || my_seg >= F.n_seg) {  // (as in the scan kernel)
      *F.err = 1;
      my_seg = 0;
    }
    if (tid < n_slots) s_wt[tid] = wts[my_seg];
  }
  fu_form_S<WEIGHTED>(S, F.rec.waves, H.p0, T, NT, n_slots, s_start, s_lo, s_hi, s_wt, tid);
  for (int t = tid; t < NT; t += FU_THREADS) out[(H.u - u_begin) * (int64_t)NT + t] = S[t];
}

// ---- charge universes: the segment weights ------------------------------------------------------------------------------------
struct CwArgs {
  SegStore s;                               // the store the launch read (charge_store: the anode view's positions with a map)
  const double* true_pos[3];                // x, y, z of the true midpoint (the store's own columns): where a map's E is read
  const LdsimConsts* c;
  const FieldMapDesc* maps;                 // or NULL
  int64_t seg_begin, n_seg;                 // the launch's range
  int32_t n_groups, pad;
  const ChargeK* k;                         // [n_groups]
  double* w;                                // [n_groups][n_seg]
  unsigned long long* unweightable;         // [n_groups]
  int32_t* err;                             // 4 = a universe's recombination is NaN or its mode unknown
};

// One thread per segment of the launch; per distinct charge variation g: n_g = what ldsim_dev_quench_drift would have stored in
// n_electrons (charge_replay, seg_charge.h), w[g][i] = n_g / n_res in f64.  n_res == 0: weight 0, counted when n_g != 0.
// Segments outside every TPC and segments that are not simulated have no pairs: weight 1.
__global__ void __launch_bounds__(256) charge_weights_kernel(CwArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n_seg) return;
  const int64_t i = a.seg_begin + r;
  const LdsimConsts* __restrict__ c = a.c;
  const int32_t plane = a.s.pixel_plane[i];
  const bool simulated = a.s.batch[i] >= 0 && plane != c->default_plane_index && plane >= 0 && plane < c->n_tpc;
  if (!simulated) {
    for (int g = 0; g < a.n_groups; g++) a.w[(int64_t)g * a.n_seg + r] = 1.0;
    return;
  }
  double e_field = c->e_field;
  const FieldMapDesc* m = (a.maps && a.maps[plane].node) ? &a.maps[plane] : nullptr;
  if (m && m->has_e) {
    const double p[3] = {a.true_pos[0][i], a.true_pos[1][i], a.true_pos[2][i]};
    double v[4];
    fmap_eval(*m, p, true, v);
    e_field = v[0];
  }
  const double dE = a.s.f[LDSIM_DE][i], dEdx = a.s.f[LDSIM_DEDX][i], z = a.s.f[LDSIM_Z][i];
  const double z_anode = c->tpc_borders[plane][2][0], n_res = a.s.f[LDSIM_N_ELECTRONS][i];
  const int code = a.s.store_code[LDSIM_N_ELECTRONS];
  for (int g = 0; g < a.n_groups; g++) {
    double n_k = 0;
    if (!charge_replay(a.k + g, e_field, dE, dEdx, z, z_anode, code, n_k)) {
      *a.err = 4;
      n_k = 0;
    }
    double wt = 0;
    if (n_res != 0)
      wt = n_k / n_res;
    else if (n_k != 0)
      atomicAdd(a.unweightable + g, 1ull);
    a.w[(int64_t)g * a.n_seg + r] = wt;
  }
}

// totals[k] = hits of universe k (place U - 1 of its counts and of their exclusive scan)
__global__ void fu_totals_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ off, int64_t U, int n,
                                 int64_t* __restrict__ totals) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) totals[k] = (int64_t)cnt[(int64_t)k * U + U - 1] + off[(int64_t)k * U + U - 1];
}

// hit_charge of one universe, in the order of its hit rows (compact_fill_kernel's charge column)
__global__ void __launch_bounds__(256) fu_charge_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                                                        const double* __restrict__ adc_list, int A, int64_t U, int64_t n_rows,
                                                        double* __restrict__ charge) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= U) return;
  const int nh = cnt[u];
  const int64_t o = off[u];
  for (int h = 0; h < nh && h < A; h++)
    if (o + h < n_rows) charge[o + h] = adc_list[u * A + h];
}

static LdsimFeeVariation fu_nominal(const LdsimConsts& h) {
  LdsimFeeVariation v{};
  v.discrimination_threshold = h.discrimination_threshold;
  v.gain = h.gain;
  v.v_cm = h.v_cm;
  v.v_ref = h.v_ref;
  v.v_pedestal = h.v_pedestal;
  v.buffer_risetime = h.buffer_risetime;
  v.reset_noise_charge = h.reset_noise_charge;
  v.uncorrelated_noise_charge = h.uncorrelated_noise_charge;
  v.discriminator_noise = h.discriminator_noise;
  v.threshold_table_scale = 1.0;
  v.threshold_table_offset = 0.0;
  v.gain_table_scale = 1.0;
  v.adc_hold_delay = h.adc_hold_delay;
  v.adc_busy_delay = h.adc_busy_delay;
  v.reset_cycles = h.reset_cycles;
  v.pad = 0;
  return v;
}

extern "C" int ldsim_fee_variation_nominal(ldsim_ctx* ctx, LdsimFeeVariation* out) {
  LDSIM_ENTER(ctx);
  if (!ctx || !out) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
  *out = fu_nominal(ctx->h_consts);
  return 0;
}

static bool fu_noisy(const LdsimFeeVariation& v) {
  return v.reset_noise_charge != 0 || v.uncorrelated_noise_charge != 0 || v.discriminator_noise != 0;
}

// LDSIM_EINVAL with the universe and the field named, before anything of the context is touched
static int fu_validate(const ldsim_ctx* ctx, const LdsimFeeVariation* v, int32_t n) {
  if (n < 1 || n > LDSIM_FEE_UNIVERSES_MAX) {
    ldsim_set_error("FEE universes: n = %d universes, must lie in [1, %d]", (int)n, LDSIM_FEE_UNIVERSES_MAX);
    return LDSIM_EINVAL;
  }
  static const char* const names[12] = {"discrimination_threshold", "gain", "v_cm", "v_ref", "v_pedestal", "buffer_risetime",
                                        "reset_noise_charge", "uncorrelated_noise_charge", "discriminator_noise",
                                        "threshold_table_scale", "threshold_table_offset", "gain_table_scale"};
  const double dt = ctx->h_consts.time_sampling;
  for (int k = 0; k < n; k++) {
    const LdsimFeeVariation& x = v[k];
    const double f[12] = {x.discrimination_threshold, x.gain, x.v_cm, x.v_ref, x.v_pedestal, x.buffer_risetime,
                          x.reset_noise_charge, x.uncorrelated_noise_charge, x.discriminator_noise,
                          x.threshold_table_scale, x.threshold_table_offset, x.gain_table_scale};
    for (int i = 0; i < 12; i++)
      if (!isfinite(f[i])) {
        ldsim_set_error("FEE universes: universe %d: %s is not finite", k, names[i]);
        return LDSIM_EINVAL;
      }
    if (x.v_ref == x.v_cm) {
      ldsim_set_error("FEE universes: universe %d: v_ref == v_cm (%g): the ADC has no range", k, x.v_ref);
      return LDSIM_EINVAL;
    }
    if (x.adc_hold_delay < 0 || x.adc_busy_delay < 0 || x.reset_cycles < 0) {
      ldsim_set_error("FEE universes: universe %d: negative adc_hold_delay, adc_busy_delay or reset_cycles (%d, %d, %d)", k,
                      (int)x.adc_hold_delay, (int)x.adc_busy_delay, (int)x.reset_cycles);
      return LDSIM_EINVAL;
    }
    if (x.reset_noise_charge < 0 || x.uncorrelated_noise_charge < 0 || x.discriminator_noise < 0) {
      ldsim_set_error("FEE universes: universe %d: negative noise charge (%g, %g, %g)", k, x.reset_noise_charge,
                      x.uncorrelated_noise_charge, x.discriminator_noise);
      return LDSIM_EINVAL;
    }
    if (x.buffer_risetime > 0 && 10 * x.buffer_risetime / dt > 62) {      // (fee_launch_chain's check)
      ldsim_set_error("FEE universes: universe %d: buffer_risetime %g exceeds the kernel's 62 taps at time_sampling %g", k,
                      x.buffer_risetime, dt);
      return LDSIM_EINVAL;
    }
    if (x.pad != 0) {
      ldsim_set_error("FEE universes: universe %d: pad must be 0", k);
      return LDSIM_EINVAL;
    }
  }
  return 0;
}

// the launch's record in the kernels' argument block
static FuArgs fu_record_args(const ldsim_ctx* ctx, const ChainView& cv) {
  FuArgs F{};
  F.rec = fee_rec_args(ctx, cv);
  F.upix = cv.upix;
  F.A = ctx->fee_rec.A;
  return F;
}

// the parts of ctx->fu_cnt for n universes of U pixels: hit_count i32 [n][U] | hit_off i32 [n][U] | totals i64 [n] | err i32
struct FuCounts {
  int32_t *cnt, *off;
  int64_t* totals;
  int32_t* err;
};
static size_t fu_counts_part(int n, int64_t U) { return (((size_t)n * (size_t)U * 4) + 15) & ~(size_t)15; }
static size_t fu_counts_bytes(int n, int64_t U) { return 2 * fu_counts_part(n, U) + (size_t)n * 8 + 16; }
static FuCounts fu_counts_of(void* p, int n, int64_t U) {
  FuCounts c;
  c.cnt = (int32_t*)p;
  c.off = (int32_t*)((char*)p + fu_counts_part(n, U));
  c.totals = (int64_t*)((char*)p + 2 * fu_counts_part(n, U));
  c.err = (int32_t*)(c.totals + n);
  return c;
}

// ---- charge universes: validation, grouping, the weights pass -------------------------------------------------------------------
static LdsimChargeVariation cu_nominal(const LdsimConsts& h, int mode) {
  LdsimChargeVariation v{};
  v.electron_lifetime = h.electron_lifetime;
  v.w_ion = h.w_ion;
  v.box_alpha = h.box_alpha;
  v.box_beta = h.box_beta;
  v.birks_ab = h.birks_ab;
  v.birks_kb = h.birks_kb;
  v.recomb_mode = mode;
  v.pad = 0;
  return v;
}

static int cu_need_mode(const ldsim_ctx* ctx, const char* who) {
  if (ctx->drift_mode != 1 && ctx->drift_mode != 2) {
    ldsim_set_error("%s: no recorded recombination mode: the resident charge does not come from ldsim_dev_quench_drift (segments "
                    "uploaded already quenched cannot be replayed)", who);
    return LDSIM_ESTATE;
  }
  return 0;
}

extern "C" int ldsim_charge_variation_nominal(ldsim_ctx* ctx, LdsimChargeVariation* out) {
  LDSIM_ENTER(ctx);
  if (!ctx || !out) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
  CK(cu_need_mode(ctx, "ldsim_charge_variation_nominal"));
  *out = cu_nominal(ctx->h_consts, ctx->drift_mode);
  return 0;
}

// LDSIM_EINVAL with the universe and the field named, before anything of the context is touched
static int cu_validate(const LdsimChargeVariation* v, int32_t n) {
  static const char* const names[6] = {"electron_lifetime", "w_ion", "box_alpha", "box_beta", "birks_ab", "birks_kb"};
  for (int k = 0; k < n; k++) {
    const LdsimChargeVariation& x = v[k];
    const double f[6] = {x.electron_lifetime, x.w_ion, x.box_alpha, x.box_beta, x.birks_ab, x.birks_kb};
    for (int i = 0; i < 6; i++)
      if (!isfinite(f[i])) {
        ldsim_set_error("charge universes: universe %d: %s is not finite", k, names[i]);
        return LDSIM_EINVAL;
      }
    if (!(x.electron_lifetime > 0)) {
      ldsim_set_error("charge universes: universe %d: electron_lifetime %g must be > 0", k, x.electron_lifetime);
      return LDSIM_EINVAL;
    }
    if (!(x.w_ion > 0)) {
      ldsim_set_error("charge universes: universe %d: w_ion %g must be > 0", k, x.w_ion);
      return LDSIM_EINVAL;
    }
    if (x.recomb_mode != 1 && x.recomb_mode != 2) {
      ldsim_set_error("charge universes: universe %d: recomb_mode %d must be 1 (box) or 2 (Birks)", k, (int)x.recomb_mode);
      return LDSIM_EINVAL;
    }
    if (x.pad != 0) {
      ldsim_set_error("charge universes: universe %d: pad must be 0", k);
      return LDSIM_EINVAL;
    }
  }
  return 0;
}

// the parts of ctx->cu_w for G distinct charge variations, n universes and n_seg segments:
// w f64 [G][n_seg] | unweightable u64 [G] | error word (8 bytes) | ChargeK [G] | group begins i32 [G + 1], order i32 [n]
struct CuParts {
  double* w;
  unsigned long long* unw;
  int32_t* err;
  ChargeK* k;
  int32_t* grp;
  size_t bytes;
};
static CuParts cu_parts_of(void* p, int G, int n, int64_t n_seg) {
  CuParts c;
  char* q = (char*)p;
  c.w = (double*)q;
  q += (size_t)G * (size_t)n_seg * 8;
  c.unw = (unsigned long long*)q;
  q += (size_t)G * 8;
  c.err = (int32_t*)q;
  q += 8;
  c.k = (ChargeK*)q;
  q += (size_t)G * sizeof(ChargeK);
  c.grp = (int32_t*)q;
  q += (size_t)(G + 1 + n) * 4;
  c.bytes = (size_t)(q - (char*)p);
  return c;
}
static_assert(sizeof(ChargeK) % 8 == 0, "cu_w layout");

// the universes pass.  charge == NULL: the FEE universes of the launch's own S.  fee == NULL: nominal FEE for every universe.
static int fu_run(ldsim_ctx* ctx, const LdsimFeeVariation* v, const LdsimChargeVariation* charge, int32_t n, int64_t* n_hits,
                  const char* who) {
  std::vector<LdsimFeeVariation> own_fee;
  if (!v) {
    if (n < 1 || n > LDSIM_FEE_UNIVERSES_MAX) {
      ldsim_set_error("FEE universes: n = %d universes, must lie in [1, %d]", (int)n, LDSIM_FEE_UNIVERSES_MAX);
      return LDSIM_EINVAL;
    }
    own_fee.assign((size_t)n, fu_nominal(ctx->h_consts));
    v = own_fee.data();
  }
  CK(fu_validate(ctx, v, n));
  if (charge) CK(cu_validate(charge, n));
  CK(launch_need_record(ctx, who));
  // ---- charge universes: the state the replay needs, and the groups of byte-equal charge variations ---------------------------
  std::vector<int32_t> group_of, grp;        // [n]; group begins [G + 1] | universes ordered by group [n]
  std::vector<ChargeK> hk;
  int G = 0;
  if (charge) {
    CK(cu_need_mode(ctx, who));
    if (ctx->charge_stat || ctx->drift_stat_on != 0) {
      ldsim_set_error("%s: charge statistics are on: binomial draws are not linear in the constants, the launch cannot be "
                      "re-weighted", who);
      return LDSIM_ESTATE;
    }
    if (ctx->mc_current) {
      ldsim_set_error("%s: the launch's currents come from tracks_current_mc (option mc_current): its rows are not re-weighted", who);
      return LDSIM_ESTATE;
    }
    group_of.assign((size_t)n, 0);
    std::vector<int> first;                  // first universe of every group
    for (int k = 0; k < n; k++) {
      int g = 0;
      while (g < G && memcmp(&charge[first[(size_t)g]], &charge[k], sizeof(LdsimChargeVariation)) != 0) g++;
      if (g == G) {
        first.push_back(k);
        G++;
      }
      group_of[(size_t)k] = g;
    }
    grp.assign((size_t)(G + 1 + n), 0);
    for (int k = 0; k < n; k++) grp[(size_t)group_of[(size_t)k] + 1]++;
    for (int g = 0; g < G; g++) grp[(size_t)g + 1] += grp[(size_t)g];
    std::vector<int> fill(grp.begin(), grp.begin() + G);
    for (int k = 0; k < n; k++) grp[(size_t)(G + 1 + fill[(size_t)group_of[(size_t)k]]++)] = k;
    for (int g = 0; g < G; g++) {
      const LdsimChargeVariation& x = charge[first[(size_t)g]];
      hk.push_back(ChargeK{x.box_alpha, x.box_beta, x.birks_ab, x.birks_kb, x.w_ion, x.electron_lifetime,
                           ctx->h_consts.lar_density, ctx->h_consts.v_drift, x.recomb_mode, 0});
    }
  }
  bool any_noisy = false;
  for (int k = 0; k < n; k++) any_noisy = any_noisy || fu_noisy(v[k]);
  if (any_noisy && !(ctx->rng_keyed && ctx->rng_batch_keys_n > 0)) {
    ldsim_set_error("FEE universes: a universe has a non-zero noise charge, and its normals come from the keyed streams of the "
                    "launch's pixels only: call ldsim_rng_keyed_seed and ldsim_chain_set_batch_keys before the launch (in table "
                    "mode the pass never draws)");
    return LDSIM_ESTATE;
  }
  const LdsimConsts& h = ctx->h_consts;
  const bool tables_fit = ctx->pix_table_n == (int64_t)h.n_pixels[0] * h.n_pixels[1] * h.n_tpc;
  if (!tables_fit && (ctx->d_pix_thr.p || ctx->d_pix_gain.p)) {
    ldsim_set_error("pixel threshold/gain tables were set for another pixel geometry: set them again after set_consts");
    return LDSIM_ESTATE;
  }
  HIPCHK(hipSetDevice(ctx->device));
  const ChainView cv = chain_view(ctx);     // (the pass grows its own buffers and SB_SORTTMP only)
  const int64_t U = cv.U;
  ctx->fu_gen = -1;                         // (until the pass is complete)
  ctx->fu_n = 0;
  ctx->fu_hits.assign((size_t)n, 0);
  ctx->fu_row0.assign((size_t)n + 1, 0);
  ctx->fu_timed = false;
  ctx->cu_group.clear();
  ctx->cu_unw.clear();
  ctx->cu_timed = false;
  if (n_hits)
    for (int k = 0; k < n; k++) n_hits[k] = 0;
  // ---- the weights of the launch's segments, one row per distinct charge variation ---------------------------------------------
  const int64_t n_seg = ctx->launch_seg[1] - ctx->launch_seg[0];
  CuParts P{};
  if (charge) {
    if (ctx->launch_seg[0] < 0 || n_seg < 0 || ctx->launch_seg[1] > ctx->seg.n) {
      ldsim_set_error("%s: the launch's segment range lies outside the resident store", who);
      return LDSIM_ESTATE;
    }
    const size_t need = cu_parts_of(nullptr, G, n, n_seg).bytes;
    CK(pass_ensure(ctx->cu_w, need, "FEE universes", "the segment weights"));
    P = cu_parts_of(ctx->cu_w.p, G, n, n_seg);
    hipStream_t st0 = ctx->stream;
    HIPCHK(hipMemsetAsync(P.unw, 0, (size_t)G * 8 + 8, st0));
    HIPCHK(hipMemcpyAsync(P.k, hk.data(), (size_t)G * sizeof(ChargeK), hipMemcpyHostToDevice, st0));
    HIPCHK(hipMemcpyAsync(P.grp, grp.data(), grp.size() * 4, hipMemcpyHostToDevice, st0));
    if (n_seg > 0) {
      CwArgs a{};
      a.s = charge_store(ctx);
      for (int d = 0; d < 3; d++) a.true_pos[d] = ctx->seg.f[LDSIM_X + d];
      a.c = ctx->d_consts.as<LdsimConsts>();
      a.maps = ctx->drift_map_gen >= 0 ? (const FieldMapDesc*)ctx->d_fmap.as<FieldMapDesc>() : nullptr;
      a.seg_begin = ctx->launch_seg[0];
      a.n_seg = n_seg;
      a.n_groups = G;
      a.k = P.k;
      a.w = P.w;
      a.unweightable = P.unw;
      a.err = P.err;
      for (int k = 0; k < 2; k++) CK(ctx->cu_ev[k].ensure());
      HIPCHK(hipEventRecord(ctx->cu_ev[0], st0));
      hipLaunchKernelGGL(charge_weights_kernel, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, st0, a);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(ctx->cu_ev[1], st0));
      ctx->cu_timed = true;
    }
    std::vector<unsigned long long> unw((size_t)G + 1);
    HIPCHK(hipMemcpyAsync(unw.data(), P.unw, (size_t)G * 8 + 8, hipMemcpyDeviceToHost, st0));
    HIPCHK(hipStreamSynchronize(st0));      // (hk and grp are read by the copies above until here)
    if ((int32_t)(unw[(size_t)G] & 0xffffffffu) != 0) {
      ldsim_set_error("charge universes: Invalid recombination value under a universe's constants");
      return LDSIM_EINVAL;
    }
    ctx->cu_unw.assign(unw.begin(), unw.begin() + G);
    ctx->cu_group = group_of;
    ctx->cu_nseg = n_seg;
  }
  if (U == 0) {
    ctx->fu_n = n;
    ctx->fu_U = 0;
    ctx->fu_A = h.max_adc_values;
    ctx->fu_gen = ctx->out_gen;
    return 0;
  }
  const ldsim_ctx::FeeRecord& R = ctx->fee_rec;
  if (R.NT > FU_NT_MAX || R.A > FU_A_MAX || R.M > FU_M_MAX) {
    ldsim_set_error("FEE constants exceed the kernel's static tiles");
    return LDSIM_EINVAL;
  }
  hipStream_t st = ctx->stream;
  const int A = R.A;
  // ---- every buffer of the dense result first: a result that does not fit is refused before anything is written ---------------
  const size_t plane = (size_t)n * (size_t)U * (size_t)A * 8;      // one of adc_list, adc_ticks, adc_digit
  CK(pass_ensure(ctx->fu_dense, 3 * plane, "FEE universes", "the per-universe ADC arrays"));
  CK(pass_ensure(ctx->fu_cnt, fu_counts_bytes(n, U), "FEE universes", "the hit counts"));
  const size_t b_uni = (((size_t)n * sizeof(FuUni)) + 15) & ~(size_t)15;
  CK(pass_ensure(ctx->fu_uni, b_uni + (size_t)n * 128 * 8, "FEE universes", "the universes' constants"));
  const FuCounts C = fu_counts_of(ctx->fu_cnt.p, n, U);
  double* d_tabs = (double*)((char*)ctx->fu_uni.p + b_uni);
  // ---- the universes' constants and tap tables ----------------------------------------------------------------------------
  std::vector<FuUni> hu((size_t)n);
  for (int k = 0; k < n; k++) {
    const LdsimFeeVariation& x = v[k];
    FuUni& q = hu[(size_t)k];
    q.k = FEEK_FROM(h);
    q.k.buffer_risetime = x.buffer_risetime;
    q.k.adc_hold_delay = (double)x.adc_hold_delay;
    q.k.reset_cycles = (double)x.reset_cycles;
    q.k.adc_busy_delay = (double)x.adc_busy_delay;
    q.k.reset_noise_charge = x.reset_noise_charge;
    q.k.uncorrelated_noise_charge = x.uncorrelated_noise_charge;
    q.k.discriminator_noise = x.discriminator_noise;
    q.k.v_pedestal = x.v_pedestal;
    q.k.v_cm = x.v_cm;
    q.k.v_ref = x.v_ref;
    q.k.gain = x.gain;
    q.threshold = x.discrimination_threshold * 1.0;   // DISCRIMINATION_THRESHOLD * units.e
    q.thr_scale = x.threshold_table_scale;
    q.thr_offset = x.threshold_table_offset;
    q.gain_scale = x.gain_table_scale;
    q.noisy = fu_noisy(x) ? 1 : 0;
    q.pad = 0;
    CK(fee_launch_tables(ctx, h.time_sampling, x.buffer_risetime, d_tabs + (size_t)k * 128));
  }
  HIPCHK(hipMemcpyAsync(ctx->fu_uni.p, hu.data(), (size_t)n * sizeof(FuUni), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(ctx->fu_cnt.p, 0, fu_counts_bytes(n, U), st));
  FuArgs F = fu_record_args(ctx, cv);
  F.n = n;
  F.uni = ctx->fu_uni.as<FuUni>();
  F.tabs = d_tabs;
  F.thr_table = tables_fit ? ctx->d_pix_thr.as<double>() : nullptr;
  F.gain_table = tables_fit ? ctx->d_pix_gain.as<double>() : nullptr;
  F.n_pix_ids = ctx->pix_table_n;
  F.batch_keys = any_noisy ? (const uint64_t*)ctx->d_batch_keys.p : nullptr;
  F.n_keys = any_noisy ? ctx->rng_batch_keys_n : 0;
  F.seed = ctx->rng_seed;
  F.time_padding = 0.0;                     // cli/simulate_pixels.py:1092, as chain_run
  F.adc_list = ctx->fu_dense.as<double>();
  F.adc_ticks = F.adc_list + (size_t)n * U * A;
  F.adc_digit = F.adc_ticks + (size_t)n * U * A;
  F.hit_count = C.cnt;
  F.err = C.err;
  const size_t lds_S = (size_t)((R.NT + 1) & ~1) * 8;
  for (int k = 0; k < 2; k++) CK(ctx->fu_ev[k].ensure());
  HIPCHK(hipEventRecord(ctx->fu_ev[0], st));
  if (charge) {
    F.w = P.w;
    F.grp = P.grp;
    F.n_seg = n_seg;
    F.n_groups = G;
    hipLaunchKernelGGL(pixel_adc_universes_kernel<true>, dim3((unsigned)U), dim3(FU_THREADS), lds_S, st, F);
  } else {
    hipLaunchKernelGGL(pixel_adc_universes_kernel<false>, dim3((unsigned)U), dim3(FU_THREADS), lds_S, st, F);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->fu_ev[1], st));
  ctx->fu_timed = true;
  // ---- compact rows per universe: the launch's own scan and compact_hits_kernel ------------------------------------------------
  for (int k = 0; k < n; k++) CK(sort_exclusive_scan_i32(ctx, C.cnt + (size_t)k * U, C.off + (size_t)k * U, U));
  hipLaunchKernelGGL(fu_totals_kernel, dim3(1), dim3(64), 0, st, C.cnt, C.off, U, (int)n, C.totals);
  HIPCHK(hipGetLastError());
  std::vector<int64_t> tot((size_t)n);
  int32_t err = 0;
  HIPCHK(hipMemcpyAsync(tot.data(), C.totals, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&err, C.err, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (err == 3) {
    ldsim_set_error("FEE universes: a batch of the launch has no key (ldsim_chain_set_batch_keys holds %lld): the keys must be "
                    "those the launch ran with", (long long)ctx->rng_batch_keys_n);
    return LDSIM_ESTATE;
  }
  if (err == 2) {
    ldsim_set_error("FEE universes: a pixel of the launch lies outside the pixel threshold/gain tables");
    return LDSIM_ESTATE;
  }
  int64_t rows = 0;
  for (int k = 0; k < n; k++) {
    if (err || tot[(size_t)k] < 0 || tot[(size_t)k] > U * (int64_t)A) {
      ldsim_set_error("FEE universes: the set-up record of the last chain launch does not describe its buffers");
      return LDSIM_ESTATE;
    }
    ctx->fu_row0[(size_t)k] = rows;
    rows += tot[(size_t)k];
  }
  ctx->fu_row0[(size_t)n] = rows;
  // rows: [rows] 24-byte hit rows | [rows] f64 charges
  CK(pass_ensure(ctx->fu_rows, (size_t)rows * 32 + 32, "FEE universes", "the hit rows"));
  char* d_rows = ctx->fu_rows.as<char>();
  double* d_chg = (double*)(d_rows + (size_t)rows * 24);
  for (int k = 0; k < n; k++) {
    if (!tot[(size_t)k]) continue;
    const int64_t r0 = ctx->fu_row0[(size_t)k];
    const size_t o = (size_t)k * U * A;
    CK(sort_compact_hits(ctx, cv.upix, cv.ubatch, C.cnt + (size_t)k * U, C.off + (size_t)k * U, F.adc_digit + o, F.adc_ticks + o, A, U,
                         (int32_t*)(d_rows + (size_t)r0 * 24)));
    hipLaunchKernelGGL(fu_charge_kernel, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, st, C.cnt + (size_t)k * U,
                       C.off + (size_t)k * U, F.adc_list + o, A, U, tot[(size_t)k], d_chg + r0);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < n; k++) {
    ctx->fu_hits[(size_t)k] = tot[(size_t)k];
    if (n_hits) n_hits[k] = tot[(size_t)k];
  }
  ctx->fu_n = n;
  ctx->fu_U = U;
  ctx->fu_A = A;
  ctx->fu_gen = ctx->out_gen;
  return 0;
}

extern "C" int ldsim_chain_fee_universes(ldsim_ctx* ctx, const LdsimFeeVariation* v, int32_t n, int64_t* n_hits) {
  LDSIM_ENTER(ctx);
  if (!ctx || !v) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
  return fu_run(ctx, v, nullptr, n, n_hits, "ldsim_chain_fee_universes");
}

extern "C" int ldsim_chain_universes(ldsim_ctx* ctx, const LdsimFeeVariation* fee, const LdsimChargeVariation* charge, int32_t n,
                                     int64_t* n_hits) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
  if (!charge) {                            // exactly ldsim_chain_fee_universes
    if (!fee) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
    return fu_run(ctx, fee, nullptr, n, n_hits, "ldsim_chain_fee_universes");
  }
  return fu_run(ctx, fee, charge, n, n_hits, "ldsim_chain_universes");
}

static int fu_need_pass(ldsim_ctx* ctx, int32_t k) {
  if (ctx->fu_gen < 0 || ctx->fu_gen != ctx->out_gen) {
    ldsim_set_error("ldsim_chain_fee_universes has not run for the last chain launch");
    return LDSIM_ESTATE;
  }
  if (k < 0 || k >= ctx->fu_n) {
    ldsim_set_error("FEE universes: universe %d of the %d the last pass ran", (int)k, (int)ctx->fu_n);
    return LDSIM_EINVAL;
  }
  return 0;
}

extern "C" int ldsim_chain_fee_universe_download(ldsim_ctx* ctx, int32_t k, int64_t capacity, double* adc_list, double* adc_ticks,
                                                 double* adc_digit, int32_t* hit_count) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(fu_need_pass(ctx, k));
  const int64_t U = ctx->fu_U;
  if (capacity < U) {
    ldsim_set_error("capacity %lld < required %lld rows", (long long)capacity, (long long)U);
    return LDSIM_ENOSPC;
  }
  if (U == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int n = ctx->fu_n, A = ctx->fu_A;
  const size_t plane = (size_t)n * U * A, o = (size_t)k * U * A, b = (size_t)U * A * 8;
  const double* base = ctx->fu_dense.as<double>();
  const FuCounts C = fu_counts_of(ctx->fu_cnt.p, n, U);
  if (adc_list) HIPCHK(hipMemcpyAsync(adc_list, base + o, b, hipMemcpyDeviceToHost, st));
  if (adc_ticks) HIPCHK(hipMemcpyAsync(adc_ticks, base + plane + o, b, hipMemcpyDeviceToHost, st));
  if (adc_digit) HIPCHK(hipMemcpyAsync(adc_digit, base + 2 * plane + o, b, hipMemcpyDeviceToHost, st));
  if (hit_count) HIPCHK(hipMemcpyAsync(hit_count, C.cnt + (size_t)k * U, (size_t)U * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int ldsim_chain_fee_universe_hits_download(ldsim_ctx* ctx, int32_t k, void* hit_rows, double* hit_charge) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(fu_need_pass(ctx, k));
  const int64_t nh = ctx->fu_hits[(size_t)k], r0 = ctx->fu_row0[(size_t)k], rows = ctx->fu_row0[(size_t)ctx->fu_n];
  if (nh == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const char* d_rows = ctx->fu_rows.as<const char>();
  if (hit_rows) HIPCHK(hipMemcpyAsync(hit_rows, d_rows + (size_t)r0 * 24, (size_t)nh * 24, hipMemcpyDeviceToHost, st));
  if (hit_charge)
    HIPCHK(hipMemcpyAsync(hit_charge, (const double*)(d_rows + (size_t)rows * 24) + r0, (size_t)nh * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int ldsim_chain_fee_universes_ms(ldsim_ctx* ctx, double* scan_ms) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(fu_need_pass(ctx, 0));
  if (scan_ms) *scan_ms = 0;
  if (!ctx->fu_timed) return 0;             // (no kernel ran)
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->fu_ev[0], ctx->fu_ev[1]));
  if (scan_ms) *scan_ms = ms;
  return 0;
}

// ---- charge universes: what tests and tools read ------------------------------------------------------------------------------
extern "C" int ldsim_chain_universe_weights_download(ldsim_ctx* ctx, int32_t k, double* w, int64_t n_segments,
                                                     int64_t* n_unweightable) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(fu_need_pass(ctx, k));
  if (ctx->cu_group.empty()) {
    ldsim_set_error("the last universes pass had no charge variations (ldsim_chain_universes with charge)");
    return LDSIM_ESTATE;
  }
  if (n_segments != ctx->cu_nseg) {
    ldsim_set_error("charge universes: %lld weights asked for, the launch has %lld segments", (long long)n_segments,
                    (long long)ctx->cu_nseg);
    return LDSIM_EINVAL;
  }
  const int g = ctx->cu_group[(size_t)k];
  if (n_unweightable) *n_unweightable = (int64_t)ctx->cu_unw[(size_t)g];
  if (!w || n_segments == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const CuParts P = cu_parts_of(ctx->cu_w.p, (int)ctx->cu_unw.size(), ctx->fu_n, ctx->cu_nseg);
  HIPCHK(hipMemcpyAsync(w, P.w + (size_t)g * (size_t)n_segments, (size_t)n_segments * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int ldsim_chain_universes_weights_ms(ldsim_ctx* ctx, double* weights_ms) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(fu_need_pass(ctx, 0));
  if (weights_ms) *weights_ms = 0;
  if (!ctx->cu_timed) return 0;             // (no kernel ran)
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->cu_ev[0], ctx->cu_ev[1]));
  if (weights_ms) *weights_ms = ms;
  return 0;
}

extern "C" int ldsim_chain_universe_waveforms_dense(ldsim_ctx* ctx, int32_t k, int64_t u_begin, int64_t u_end, double* S) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(fu_need_pass(ctx, k));
  CK(launch_need_record(ctx, "ldsim_chain_universe_waveforms_dense"));
  const int64_t U = ctx->fu_U;
  if (u_begin < 0 || u_end < u_begin || u_end > U) {
    ldsim_set_error("rows [%lld, %lld) are no range of [0, %lld]", (long long)u_begin, (long long)u_end, (long long)U);
    return LDSIM_EINVAL;
  }
  if (u_end == u_begin) return 0;
  if (!S) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
  HIPCHK(hipSetDevice(ctx->device));
  const ChainView cv = chain_view(ctx);
  const ldsim_ctx::FeeRecord& R = ctx->fee_rec;
  if (cv.U != U || R.NT > FU_NT_MAX || R.M > FU_M_MAX) {
    ldsim_set_error("the universes pass and the launch's record disagree");
    return LDSIM_ESTATE;
  }
  hipStream_t st = ctx->stream;
  const size_t bytes = (size_t)(u_end - u_begin) * (size_t)R.NT * 8;
  CK(pass_ensure(ctx->cu_S, bytes, "FEE universes", "the dense waveforms"));
  HIPCHK(hipMemsetAsync(ctx->cu_S.p, 0, bytes, st));
  FuArgs F = fu_record_args(ctx, cv);
  const FuCounts C = fu_counts_of(ctx->fu_cnt.p, ctx->fu_n, U);
  F.err = C.err;                            // (the pass left it 0; a record that does not fit sets it again)
  const size_t lds_S = (size_t)((R.NT + 1) & ~1) * 8;
  if (!ctx->cu_group.empty()) {
    const CuParts P = cu_parts_of(ctx->cu_w.p, (int)ctx->cu_unw.size(), ctx->fu_n, ctx->cu_nseg);
    F.n_seg = ctx->cu_nseg;
    hipLaunchKernelGGL(fu_dense_kernel<true>, dim3((unsigned)U), dim3(FU_THREADS), lds_S, st, F,
                       (const double*)(P.w + (size_t)ctx->cu_group[(size_t)k] * (size_t)ctx->cu_nseg), u_begin, u_end,
                       ctx->cu_S.as<double>());
  } else {
    hipLaunchKernelGGL(fu_dense_kernel<false>, dim3((unsigned)U), dim3(FU_THREADS), lds_S, st, F, (const double*)nullptr, u_begin,
                       u_end, ctx->cu_S.as<double>());
  }
  HIPCHK(hipGetLastError());
  int32_t err = 0;
  HIPCHK(hipMemcpyAsync(S, ctx->cu_S.p, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&err, C.err, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (err) {
    ldsim_set_error("charge universes: the set-up record of the last chain launch does not describe its buffers");
    return LDSIM_ESTATE;
  }
  return 0;
}
