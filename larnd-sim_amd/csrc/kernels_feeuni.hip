// kernels_feeuni.hip -- FEE universes: the last chain launch digitised again under varied front-end constants
// (include/ldsim.h, "FEE universes"; the Python side: larndsim_amd/fee_universes.py).
//
// A sibling of kernels_pixtruth.hip and kernels_pixwave.hip: it reads what the launch left in HBM -- the per-pair current rows
// (f32 [n_pairs][T]) and the FEE set-up record (fee_record.h) -- and changes nothing of the chain.  A launch spends its time on
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
#include <math.h>

#include <vector>

#include "launchers.h"
#include "fee_record.h"
#include "fee_scan.h"

#define FU_THREADS 256
#define FU_WAVES 4
#define FU_NT_MAX 4096   // ticks of S in LDS (32 KB)
#define FU_A_MAX 64
#define FU_M_MAX 64

// one universe on the device: the constants the scan and the digitisation read, and what the pixel tables are transformed by
struct FuUni {
  FeeK k;
  double threshold;                         // DISCRIMINATION_THRESHOLD * e
  double thr_scale, thr_offset, gain_scale; // pixel tables: thr_table[pix] * thr_scale + thr_offset, gain_table[pix] * gain_scale
  int32_t noisy, pad;                       // a noise charge is non-zero: the scan draws
};

struct FuArgs {
  // the launch's record
  const FeeHdr* hdr;
  const unsigned long long* counts;         // [2] with lists, else NULL
  const FeeSlot* slots;
  const float* waves;
  const int32_t* upix;
  int64_t U, n_pairs;
  int32_t T, NT, M, A;
  // the universes
  int32_t n, pad;
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
};

__device__ __forceinline__ void fu_wave_sync() {      // (LDS traffic of one wave is in order: only the compiler has to be held)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(FU_THREADS) pixel_adc_universes_kernel(FuArgs F) {
  extern __shared__ double S[];             // [N_t]: sized at launch
  __shared__ HitRec hits[FU_WAVES][FU_A_MAX];
  __shared__ double taps[FU_WAVES][64];
  __shared__ int s_start[FU_M_MAX], s_lo[FU_M_MAX], s_hi[FU_M_MAX];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NT = F.NT, A = F.A, T = F.T;
  const int64_t U = F.U;
  // ---- the pixel's header: header w, or (two lists) the w-th of list 0 followed by list 1 (kernels_pixwave.hip pw_pixel) -------
  const int64_t w = blockIdx.x;
  if (w >= U) return;
  int64_t idx = w;
  bool ok = true;
  if (F.counts) {
    const int64_t c0 = (int64_t)F.counts[0], c1 = (int64_t)F.counts[1];
    ok = c0 >= 0 && c0 <= U && c1 >= 0 && c0 + c1 == U;
    if (ok && w >= c0) idx = U + (w - c0);
  }
  FeeHdr H{};
  if (ok) H = F.hdr[idx];
  const int64_t u = H.u, p0 = H.p0;
  const int n_slots = H.n_slots < F.M ? H.n_slots : F.M;
  ok = ok && u >= 0 && u < U && n_slots >= 0 && n_slots <= FU_M_MAX && p0 >= 0 && p0 + n_slots <= F.n_pairs;
  if (!ok) {                                // (nothing outside the buffers is touched; the host refuses the result)
    if (tid == 0) *F.err = 1;
    return;
  }
  if (tid < n_slots) {
    const FeeSlot sl = F.slots[p0 + tid];
    s_start[tid] = sl.start;
    s_lo[tid] = max(sl.start + max(sl.w0, 0), 0);       // (pixel_adc_body: detsim.py:516-520; a row has T elements)
    s_hi[tid] = min(sl.start + min(sl.w1, T), NT);
  }
  // ---- S, once: each thread owns ticks tid, tid + 256, ... and adds the slots' rows in slot order -----------------------------
  for (int t = tid; t < NT; t += FU_THREADS) S[t] = 0;
  __syncthreads();
  for (int k = 0; k < n_slots; k++) {
    const int lo = s_lo[k], hi = s_hi[k];
    const float* wf = F.waves + (p0 + k) * (int64_t)T - s_start[k];
    for (int t = lo + ((tid - lo) & (FU_THREADS - 1)); t < hi; t += FU_THREADS) S[t] += (double)wf[t];
  }
  __syncthreads();
  // ---- the scans: wave wv takes the universes wv, wv + 4, ... -------------------------------------------------------------
  const int32_t pix = F.upix[u];
  const bool tabled = F.thr_table || F.gain_table;
  const bool pix_ok = !tabled || (pix >= 0 && pix < F.n_pix_ids);
  const double thr_pix = F.thr_table && pix_ok ? F.thr_table[pix] : 0.0;
  const double gain_pix = F.gain_table && pix_ok ? F.gain_table[pix] : 0.0;
  const bool key_ok = H.ubatch >= 0 && H.ubatch < F.n_keys;
  double* wtap = taps[wv];
  HitRec* my_hits = hits[wv];
  for (int k = wv; k < F.n; k += FU_WAVES) {
    const FuUni* V = F.uni + k;
    const FeeK* c = &V->k;
    if (!pix_ok || (V->noisy && !key_ok)) {
      if (lane == 0) *F.err = pix_ok ? 3 : 2;
      continue;
    }
    const double dt = c->time_sampling, rt = c->buffer_risetime;
    const int ntap = rt > 0 ? (int)ceil(10 * rt / dt) : 0;  // floor(ic - 10*rt/dt) == ic - ceil(10*rt/dt)
    wtap[lane] = F.tabs[(int64_t)k * 128 + lane];
    fu_wave_sync();
    // (two roundings each, as the same transformation of the tables on the host has)
    const double thr = F.thr_table ? __dadd_rn(__dmul_rn(thr_pix, V->thr_scale), V->thr_offset) : V->threshold;
    const double gain = F.gain_table ? __dmul_rn(gain_pix, V->gain_scale) : c->gain * (1e-3 * (1e-6 * 1.0)) / 1.0;   // GAIN * mV / e
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
    fu_wave_sync();                         // (the next universe's scan writes the same HitRec and taps)
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

// a buffer of the pass; an allocation that fails leaves the buffer empty and the context usable
static int fu_ensure(DevBuf& b, size_t need, const char* what) {
  if (need <= b.bytes && b.p) return 0;
  if (b.ensure(need)) {
    (void)hipGetLastError();
    ldsim_set_error("FEE universes: no device memory for %s (%zu bytes)", what, need);
    return LDSIM_ENOMEM;
  }
  return 0;
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

extern "C" int ldsim_chain_fee_universes(ldsim_ctx* ctx, const LdsimFeeVariation* v, int32_t n, int64_t* n_hits) {
  LDSIM_ENTER(ctx);
  if (!ctx || !v) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
  CK(fu_validate(ctx, v, n));
  CK(pt_need_launch(ctx, "ldsim_chain_fee_universes"));
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
  if (n_hits)
    for (int k = 0; k < n; k++) n_hits[k] = 0;
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
  CK(fu_ensure(ctx->fu_dense, 3 * plane, "the per-universe ADC arrays"));
  CK(fu_ensure(ctx->fu_cnt, fu_counts_bytes(n, U), "the hit counts"));
  const size_t b_uni = (((size_t)n * sizeof(FuUni)) + 15) & ~(size_t)15;
  CK(fu_ensure(ctx->fu_uni, b_uni + (size_t)n * 128 * 8, "the universes' constants"));
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
  FuArgs F{};
  F.hdr = cv.fee.hdr;
  F.counts = cv.fee.counts;
  F.slots = cv.fee_slots;
  F.waves = cv.waves;
  F.upix = cv.upix;
  F.U = U;
  F.n_pairs = R.n_pairs;
  F.T = R.T;
  F.NT = R.NT;
  F.M = R.M;
  F.A = A;
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
  hipLaunchKernelGGL(pixel_adc_universes_kernel, dim3((unsigned)U), dim3(FU_THREADS), lds_S, st, F);
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
  CK(fu_ensure(ctx->fu_rows, (size_t)rows * 32 + 32, "the hit rows"));
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
