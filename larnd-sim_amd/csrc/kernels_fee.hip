// kernels_fee.hip -- a13-a16: per-pixel summation, LArPix self-trigger / ADC scan, digitisation.
// Reference: larndsim/detsim.py:468-607 (sum_pixel_signals, get_track_pixel_map2),
//            larndsim/fee.py:499-655 (digitize, get_adc_values).
//
// Chain form: one workgroup per unique (batch, pixel).  The pairs of a pixel are contiguous in the
// sorted pair list in exactly the slot order get_track_pixel_map2 produces (ring distance, then
// segment index), so the pixel's waveform is a register-owned sum over <= 50 compact f32 waveforms
// (no atomics, no [U][N_t][50] slab), the trigger scan is a wave-64 prefix scan + ballot over
// 64-tick chunks, and the per-hit backtracking fractions are wave reductions over the hit spans.
#include <algorithm>
#include "launchers.h"
#include "fee_record.h"
#include "rng.h"
#include "fee_scan.h"

#define FEE_THREADS 256
#define FEE_SPAN 512     // ticks of LDS of the one-wave instantiation of pixel_adc_kernel
#define NT_MAX 4096   // max len(TIME_TICKS) held in LDS
#define A_MAX 64      // max MAX_ADC_VALUES
#define M_MAX 64      // max MAX_TRACKS_PER_PIXEL handled by the chain kernel


// ---- chain kernel ----------------------------------------------------------------------------------------------------
// Timing switches (tools/adc_phases.py): read only by a library built with make DEBUG_FEE=1; loop-invariant tests otherwise gone
#ifdef LDSIM_FEE_DEBUG
#define FEEDBG(bit) ((F.debug & (bit)) != 0)
#else
#define FEEDBG(bit) false
#endif

// Launch constants of the kernel: wtap[d] = exp(-d dt/rt) (1 - exp(-dt/rt)), the buffer's taps (fee.py:569), and
// G[n] = dt * sum_{d=0..n} w(d), the weight of a tick n ticks before the end of a hit span, in this summation order.  One wave,
// once per (time_sampling, buffer_risetime): tab = wtap[64] | G[64].  (Every pixel used to compute both: two f64 exp per thread and
// a serial prefix on one lane between barriers.)  The device's exp and the prefix order decide the scan's taps and the fractions,
// so the tables are built here with the expressions the pixel kernel had, not on the host.
__global__ void __launch_bounds__(64) fee_tables_kernel(double dt, double rt, double* __restrict__ tab) {
  __shared__ double wtap[64];
  const int tid = threadIdx.x;
  const int ntap = rt > 0 ? (int)ceil(10 * rt / dt) : 0;  // floor(ic - 10*rt/dt) == ic - ceil(10*rt/dt)
  wtap[tid] = 0;
  if (tid <= ntap && rt > 0) wtap[tid] = exp((-tid) * dt / rt) * (1 - exp(-dt / rt));
  __syncthreads();
  tab[tid] = wtap[tid];
  tab[64 + tid] = 0;
  __syncthreads();
  if (tid == 0) {
    double acc = 0;
    for (int d = 0; d <= ntap; d++) {
      acc += (rt > 0 ? wtap[d] : 1.0) * dt;
      tab[64 + d] = acc;
    }
  }
}

template <int THREADS>
__device__ __forceinline__ void fee_sync() {
  // a workgroup of one wave: LDS traffic is in order, nothing to wait for but the compiler's own reordering
  if (THREADS == 64) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// How a pixel's rows are requested.  The rows of a pixel are known once its slot rows have arrived and depend on nothing else, so
// the loads of a group of slots are issued together, ahead of one wait, with addresses clamped into the slot's own row [0, T)
// (every load is valid) and the window test at the add.  A term outside its window adds a literal +0.0: a sum that starts at +0.0
// and only adds is never -0.0, so x + (+0.0) == x to the bit and the result is S[t] += (double)wf[t] over the windows, in slot order.
#define FEE_RG 5      // one-wave form: slots per group ...
#define FEE_RS 4      // ... and 64-tick stripes per slot held in registers (a window of <= 193 ticks touches at most four)
#define FEE_LG 4      // LDS form: slots per pass over a thread's ticks
#define FEE_FT 2      // fractions: terms of a lane per slot and pass, over 4 slots per group (one-wave form) or 2
static_assert(FEE_SPAN == 512 && FEE_RS == 4, "pixel_adc_body's register form: eight stripes, a slot's first one of 0..4");

// element it of a row of T = Tm1 + 1 elements, the index clamped into the row; the byte offset in 32 bits, so the load takes the
// row's address from scalar registers and one VGPR
__device__ __forceinline__ float fee_row_load(const float* row, int it, int Tm1) {
  return *(const float*)((const char*)row + ((unsigned)min(max(it, 0), Tm1) << 2));
}
// the term of stripe m of a slot: rel0 = the lane's tick of the slot's first stripe minus the window's first tick, wd = its width
__device__ __forceinline__ double fee_term(float x, int rel0, int m, unsigned wd) {
  return (double)((unsigned)(rel0 + 64 * m) < wd ? x : 0.0f);
}

// Two instantiations.  THREADS = 256, the whole tick axis in LDS (16-26 KB: eight pixels per CU), for every pixel when noise is on
// (the scan then walks every tick) and for pixels whose slots' windows span more than FEE_SPAN ticks.  THREADS = 64 -- a wave per
// pixel, FEE_SPAN ticks of LDS starting at the pixel's first written tick -- for the others, over a list (fee_setup_kernel).  The
// kernel is a chain of dependent trips to memory per pixel, so what counts is pixels in flight -- a CU holds 2048 threads: 8
// pixels of 256 threads, 20 of 64 at 7.9 KB and at most 96 VGPRs each -- and the length of the chain: header (scalar loads; the
// list form fetches the next pixel's while this one is worked on) -> slot rows, launch constants and pixel id, one trip -> waveform
// rows, a group of slots per trip (above).  Counting the keys, the slots' starts and windows, the tick range and the batch are the
// set-up pass's work, done once per pixel there.
template <int THREADS, bool KEYED = false>
__device__ __forceinline__ void pixel_adc_body(const FeeArgs& F, const FeeHdr& H, const FeeSlot* __restrict__ slots, const bool windowed,
                                               const int s_cap) {
  const FeeK* c = &F.k;          // (kernel arguments: scalar registers, no loads)
  // (the thread index taken anew per pixel: what follows from it -- a dozen LDS and row addresses -- is a few instructions to form and
  // would otherwise sit in VGPRs across the list kernel's loop over pixels, beside the rows in flight)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, wv = THREADS == 64 ? 0 : tid >> 6;
  const int NT = c->n_time_ticks;
  const int A = c->max_adc_values, M = c->max_tracks_per_pixel;
  const double dt = c->time_sampling, rt = c->buffer_risetime;

  extern __shared__ double S[];          // [n_time_ticks]: sized at launch, so LDS (not VGPRs) stops at 8 pixels per CU
  __shared__ HitRec hits[A_MAX];
  __shared__ int s_start[M_MAX], s_w0[M_MAX], s_w1[M_MAX];
  __shared__ double wtap[64], G[64];
  __shared__ int s_nh;

  const int64_t u = H.u, p0 = H.p0;
  const int n_slots = H.n_slots;
  const int ntap = rt > 0 ? (int)ceil(10 * rt / dt) : 0;  // floor(ic - 10*rt/dt) == ic - ceil(10*rt/dt)
  // the pixel id goes with the pixel's first loads, the two table entries as soon as it is there: not a trip each ahead of the
  // scan and of the stores
  // (read through a lane offset of 0 the compiler cannot see through: taken for wave-uniform, the id would be moved to a scalar
  // register on the spot, which waits for the load; always read -- a branch around it put the wait inside the branch)
  // (the keyed instance does want it scalar: its stream key is 64-bit integer arithmetic on the id)
  int lane0 = 0;
  if (!KEYED) asm volatile("" : "+v"(lane0));
  const int32_t pix = F.upix[u + lane0];
  // slots: pairs whose ring code is valid, at most M (detsim.py:582-607), in the order of the sorted pair list
  FeeSlot sl{0, 0, 0, 0};
  if (tid < n_slots) {
    sl = slots[p0 + tid];
    s_start[tid] = sl.start;
    s_w0[tid] = sl.w0;
    s_w1[tid] = sl.w1;
    F.tpm[u * M + tid] = sl.track;
  } else if (tid < M) {
    F.tpm[u * M + tid] = -1;
  }
  if (tid <= ntap) {
    wtap[tid] = F.tab[tid];
    G[tid] = F.tab[64 + tid];
  }
  // ---- summed waveform: each thread owns ticks of the pixel's time axis and adds the slots' rows in slot order, each over the
  // ticks its window puts there (detsim.py:516-520); two forms, the same sums to the bit ----------------------------------------
  // the ticks S holds: all of them, or the pixel's window from the set-up pass (every slot's ticks lie inside it)
  const int s_lo = windowed ? H.s_lo : 0;
  const int s_hi = windowed ? min(s_lo + s_cap, NT) : NT;
  const double thr = F.thr_table ? F.thr_table[pix] : F.threshold;
  const double gain = F.gain_table ? F.gain_table[pix] : c->gain * (1e-3 * (1e-6 * 1.0)) / 1.0;   // GAIN * mV / e
  const int Tm1 = F.T - 1;
  // one-wave form, registers: lane l owns the ticks s_lo + l + 64 j, j < 8, of the FEE_SPAN ticks S holds, and keeps their sums in
  // registers: no clear pass, no read-modify-write of LDS, one LDS store per tick for the scan.  A slot's rows are loaded over
  // FEE_RS stripes from the one its window starts in (at most the fifth, so that they end inside the eight); the slot rows stay in
  // the lanes that loaded them (v_readlane).  Not for a pixel with a window over more than FEE_RS stripes: the LDS form takes it.
  bool in_regs = false;
  if (THREADS == 64 && windowed && s_cap == FEE_SPAN) {
    const int lo = max(sl.start + sl.w0, 0), hi = min(sl.start + sl.w1, NT);
    in_regs = __ballot(tid < n_slots && hi > lo && ((hi - 1 - s_lo) >> 6) > min((lo - s_lo) >> 6, 4) + FEE_RS - 1) == 0;
  }
  if (THREADS == 64 && in_regs) {
    // (eight named sums, not an array: indexed by a slot's first stripe the array would leave the registers)
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0;
    for (int k0 = 0; k0 < n_slots && !FEEDBG(0x10000); k0 += FEE_RG) {
      float x[FEE_RG][FEE_RS];
      int rel0[FEE_RG], j0[FEE_RG];
      unsigned wd[FEE_RG];
      // every load of the group, then the adds in slot order
#pragma unroll
      for (int g = 0; g < FEE_RG; g++) {
        const int k = min(k0 + g, n_slots - 1);      // (past the last slot: its row again, no width)
        const int st = __builtin_amdgcn_readlane(sl.start, k);
        const int lo = max(st + __builtin_amdgcn_readlane(sl.w0, k), 0), hi = min(st + __builtin_amdgcn_readlane(sl.w1, k), NT);
        const float* wf = F.waves + (p0 + k) * (int64_t)F.T;
        wd[g] = (k0 + g < n_slots && hi > lo) ? hi - lo : 0;
        j0[g] = min(max((lo - s_lo) >> 6, 0), FEE_SPAN / 64 - FEE_RS);
        const int t0 = s_lo + 64 * j0[g] + lane;
        rel0[g] = t0 - lo;
#pragma unroll
        for (int m = 0; m < FEE_RS; m++) x[g][m] = fee_row_load(wf, t0 + 64 * m - st, Tm1);
      }
#pragma unroll
      for (int g = 0; g < FEE_RG; g++) {
#define FEE_ADD4(A, B, C, D)                  \
  A += fee_term(x[g][0], rel0[g], 0, wd[g]);  \
  B += fee_term(x[g][1], rel0[g], 1, wd[g]);  \
  C += fee_term(x[g][2], rel0[g], 2, wd[g]);  \
  D += fee_term(x[g][3], rel0[g], 3, wd[g]);
        switch (j0[g]) {
          case 0: FEE_ADD4(a0, a1, a2, a3) break;
          case 1: FEE_ADD4(a1, a2, a3, a4) break;
          case 2: FEE_ADD4(a2, a3, a4, a5) break;
          case 3: FEE_ADD4(a3, a4, a5, a6) break;
          default: FEE_ADD4(a4, a5, a6, a7) break;
        }
#undef FEE_ADD4
      }
    }
    const double acc[FEE_SPAN / 64] = {a0, a1, a2, a3, a4, a5, a6, a7};
#pragma unroll
    for (int j = 0; j < FEE_SPAN / 64; j++) S[lane + 64 * j] = acc[j];
  } else {
    // LDS form (256 threads: thread t owns ticks t, t + 256, ...): each thread adds into its own ticks of S, FEE_LG slots per
    // pass over the ticks the group's windows cover, their loads ahead of the pass's one read and write of S
    for (int t = tid; t < s_hi - s_lo; t += THREADS) S[t] = 0;
    fee_sync<THREADS>();
    for (int k0 = 0; k0 < n_slots && !FEEDBG(0x10000); k0 += FEE_LG) {
      const float* wf[FEE_LG];
      int st[FEE_LG], lo[FEE_LG];
      unsigned wd[FEE_LG];
      int g_lo = NT, g_hi = 0;
#pragma unroll
      for (int g = 0; g < FEE_LG; g++) {
        const int k = min(k0 + g, n_slots - 1);      // (past the last slot: its row again, no width)
        st[g] = s_start[k];
        lo[g] = max(st[g] + s_w0[k], 0);
        const int hi = min(st[g] + s_w1[k], NT);
        wd[g] = (k0 + g < n_slots && hi > lo[g]) ? hi - lo[g] : 0;
        wf[g] = F.waves + (p0 + k) * (int64_t)F.T;
        if (wd[g]) { g_lo = min(g_lo, lo[g]); g_hi = max(g_hi, hi); }
      }
      for (int t = g_lo + ((tid - g_lo) & (THREADS - 1)); t < g_hi; t += THREADS) {
        float x[FEE_LG];
#pragma unroll
        for (int g = 0; g < FEE_LG; g++) x[g] = fee_row_load(wf[g], t - st[g], Tm1);
        double s = S[t - s_lo];
#pragma unroll
        for (int g = 0; g < FEE_LG; g++) s += (double)((unsigned)(t - lo[g]) < wd[g] ? x[g] : 0.0f);
        S[t - s_lo] = s;
      }
    }
  }
  fee_sync<THREADS>();
  // ---- trigger scan on wave 0 ----------------------------------------------------------------------------------------
  int nh = 0;
  if (wv == 0) {
    int nd = 0;
    if (FEEDBG(0x20000)) {
    } else if (KEYED) {
      const KeyedNoise zs{F.rng_seed, key_mix(F.batch_keys[H.ubatch], (uint64_t)(int64_t)pix)};
      nh = adc_scan(c, S, NT, 1 * c->time_interval1, thr, F.time_padding, lane, hits, wtap, ntap, zs, &nd, H.t_lo, H.t_hi, s_lo, s_hi);
    } else {
      const TableNoise zs{F.noise_z ? F.noise_z + u * (int64_t)F.noise_nd : nullptr};
      nh = adc_scan(c, S, NT, 1 * c->time_interval1, thr, F.time_padding, lane, hits, wtap, ntap, zs, &nd, H.t_lo, H.t_hi, s_lo, s_hi);
    }
    if (lane == 0) {
      if (THREADS != 64) s_nh = nh;
      if (F.n_draws) F.n_draws[u] = nd;
    }
  }
  fee_sync<THREADS>();
  if (THREADS != 64) nh = s_nh;
  for (int h = tid; h < A; h += THREADS) {
    double q = h < nh ? hits[h].q : 0.0;
    F.adc_list[u * A + h] = q;
    F.adc_ticks[u * A + h] = h < nh ? hits[h].tick : 0.0;
    F.adc_digit[u * A + h] = digitize_one(c, q, gain);
  }
  if (tid == 0) {
    F.hit_count[u] = nh;
    if (H.overflow) stat_add(F.counters, ST_OVERFLOW_PIXELS, 1ull);
    if (nh) stat_add(F.counters, ST_HITS, (unsigned long long)nh);
  }
  // ---- backtracking fractions (fee.py:572-573, 633-635): sum_jc sig_k[jc]*G[min(ntap, b-jc)] / true_q ------------
  if (F.fractions && !FEEDBG(0x40000)) {
    double* fr = F.fractions + u * (int64_t)A * M;       // zero on entry (one memset of the whole array by the launcher)
    // a wave per slot, FEE_FG slots of the wave per group: for a hit, FEE_FT terms of a lane in each of the group's slots are loaded
    // together (the rows are warm in L2 from the sum), then multiplied and added -- the lane's terms in ascending order, the test at
    // the multiply-add -- before the wave sums
    constexpr int NW = THREADS / 64, FEE_FG = THREADS == 64 ? 4 : 2;
    for (int k0 = wv; k0 < n_slots; k0 += FEE_FG * NW) {
      const float* wf[FEE_FG];
      int st[FEE_FG], w0[FEE_FG], w1[FEE_FG];
#pragma unroll
      for (int g = 0; g < FEE_FG; g++) {
        const int k = min(k0 + g * NW, n_slots - 1);      // (past the last slot: its row again, no terms)
        wf[g] = F.waves + (p0 + k) * (int64_t)F.T;
        st[g] = s_start[k];
        w0[g] = st[g] + s_w0[k];
        w1[g] = k0 + g * NW < n_slots ? st[g] + s_w1[k] - 1 : -(1 << 30);
      }
      for (int h = 0; h < nh; h++) {
        const int lr = hits[h].lr, b = hits[h].b;
        const int hi = b < NT - 1 ? b : NT - 1;
        // (the ticks of the hit span the slot's window covers: a first hit's span starts at tick 0, a thousand ticks before
        // any window; same terms in the same lane-strided order)
        int jc0[FEE_FG], j1[FEE_FG];
        double acc[FEE_FG];
        int span = -1;
#pragma unroll
        for (int g = 0; g < FEE_FG; g++) {
          const int j0 = max(lr, w0[g]);
          j1[g] = min(hi, w1[g]);
          jc0[g] = j0 + ((lr + lane - j0) & 63);
          span = max(span, j1[g] - j0);
          acc[g] = 0;
        }
        for (int o = 0; o <= span; o += 64 * FEE_FT) {
          float x[FEE_FG][FEE_FT];
#pragma unroll
          for (int g = 0; g < FEE_FG; g++)
#pragma unroll
            for (int i = 0; i < FEE_FT; i++) x[g][i] = fee_row_load(wf[g], jc0[g] + o + 64 * i - st[g], Tm1);
#pragma unroll
          for (int g = 0; g < FEE_FG; g++)
#pragma unroll
            for (int i = 0; i < FEE_FT; i++) {
              const int jc = jc0[g] + o + 64 * i;
              const int d = min(max(b - jc, 0), ntap);
              const double w = G[d];      // (buffer_risetime 0: ntap = 0 and G[0] = dt)
              // (a term past the span adds +0.0, as in the sum: acc starts at +0.0 and is never -0.0)
              const double term = (double)x[g][i] * w;
              acc[g] += jc <= j1[g] ? term : 0.0;
            }
        }
#pragma unroll
        for (int g = 0; g < FEE_FG; g++) {
          if (k0 + g * NW >= n_slots) break;
          const double a = wave_sum(acc[g]);
          if (lane == 0) fr[h * M + k0 + g * NW] = hits[h].tq > 0 ? a / hits[h].tq : a;
        }
      }
    }
  }
}

// one workgroup per unique pixel, header u of the set-up pass.  KEYED: the FEE noise is drawn inline from the row's keyed stream
// (a separate instance, no runtime branch in the scan)
template <int THREADS, bool KEYED = false>
__global__ void __launch_bounds__(THREADS) pixel_adc_kernel(FeeArgs F, const FeeHdr* __restrict__ hdr, const FeeSlot* __restrict__ slots) {
  if ((int64_t)blockIdx.x < F.U) pixel_adc_body<THREADS, KEYED>(F, hdr[blockIdx.x], slots, false, 0);
}
// a fixed grid walks a device-built list of pixels' headers (its length stays on the device: no host round trip to size the
// launch); the next pixel's header is on its way while this one is worked on
// (waves per SIMD asked of the register allocator: the five one-wave workgroups per SIMD that 7.9 KB of LDS allow, <= 96 VGPRs; the
// seven of the 256-thread form before its loads were grouped, <= 72)
template <int THREADS, bool KEYED = false>
__global__ void __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(THREADS == 64 ? 5 : 7)))
pixel_adc_list_kernel(FeeArgs F, const FeeHdr* __restrict__ list,
                                                                const unsigned long long* __restrict__ count,
                                                                const FeeSlot* __restrict__ slots, bool windowed, int s_cap) {
  const int64_t n = (int64_t)*count;
  int64_t i = blockIdx.x;
  if (i >= n) return;
  FeeHdr H = list[i];
  while (true) {
    const int64_t nx = i + gridDim.x;
    const FeeHdr Hn = list[nx < n ? nx : i];
    pixel_adc_body<THREADS, KEYED>(F, H, slots, windowed, s_cap);
    if (nx >= n) break;
    fee_sync<THREADS>();          // (the next pixel reuses the workgroup's LDS)
    H = Hn;
    i = nx;
  }
}

// zero every entry of fractions [U][A][M] that pixel_adc_kernel did not write: rows past the pixel's last hit, slots past its last track
__global__ void __launch_bounds__(256) fee_clear_fractions_kernel(int64_t U, const int32_t* __restrict__ hit_count,
                                                                 const int64_t* __restrict__ tpm, int A, int M, double* __restrict__ fr) {
  const int64_t u = blockIdx.x;
  if (u >= U) return;
  __shared__ int s_ns;
  if (threadIdx.x == 0) s_ns = 0;
  __syncthreads();
  if ((int)threadIdx.x < M && tpm[u * M + threadIdx.x] != -1) atomicAdd(&s_ns, 1);      // (filled slots come first)
  __syncthreads();
  const int nh = hit_count[u], ns = s_ns;
  double* row = fr + u * (int64_t)A * M;
  for (int h = 0; h < A; h++)
    for (int k = threadIdx.x; k < M; k += 256)
      if (!(h < nh && k < ns)) row[h * M + k] = 0.0;
}

int fee_clear_unwritten_fractions(ldsim_ctx* ctx, int64_t U, const int32_t* hit_count, const int64_t* tpm, double* fr) {
  if (U == 0) return 0;
  const LdsimConsts& h = ctx->h_consts;
  hipLaunchKernelGGL(fee_clear_fractions_kernel, dim3((unsigned)U), dim3(256), 0, ctx->stream, U, hit_count, tpm,
                     h.max_adc_values, h.max_tracks_per_pixel, fr);
  HIPCHK(hipGetLastError());
  return 0;
}

// The set-up pass, a thread per unique pixel: counts the pixel's slots (valid keys come first in its group), resolves each slot's
// start tick, window and track index into the slot pool, the batch and the ticks the slots write, [t_lo, t_hi), into the header.
// With lists: the pixels whose window fits FEE_SPAN ticks go to list 0, the others to list 1 (one atomic per wave and list), each
// list holding its pixels' headers; without: header u at index u.
__global__ void __launch_bounds__(256) fee_setup_kernel(FeeArgs F, FeeSlot* __restrict__ slots, FeeHdr* __restrict__ hdr /* [2][U] or [U] */,
                                                        unsigned long long* __restrict__ counts /* [2] or NULL */) {
  const FeeK* c = &F.k;
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int cls = -1;
  FeeHdr H{};
  if (u < F.U) {
    const int NT = c->n_time_ticks, M = c->max_tracks_per_pixel;
    const double dt = c->time_sampling;
    const int64_t p0 = F.uoff[u], p1 = F.uoff[u + 1];
    const int ubatch = F.ubatch[u];
    const int bfirst = F.batch_first[ubatch - F.batch0];
    int n_slots = 0;
    for (int64_t p = p0; p < p1 && n_slots < M; p++) n_slots += (F.pair_key[p] & 15ull) != 15ull;      // (valid ones come first)
    int t_lo = NT, t_hi = 0;
    for (int k = 0; k < n_slots; k++) {
      const int r = F.pair_val[p0 + k] / F.P;
      const int st = (int)py_round(F.track_starts[r] / dt);   // detsim.py:506
      const int w0 = F.win ? F.win[2 * (p0 + k)] : 0, w1 = F.win ? F.win[2 * (p0 + k) + 1] : F.T;
      const int lo = max(st + w0, 0), hi = min(st + w1, NT);
      if (hi > lo) { t_lo = min(t_lo, lo); t_hi = max(t_hi, hi); }
      slots[p0 + k] = FeeSlot{st, w0, w1, r - bfirst};
    }
    H.u = (int32_t)u;
    H.n_slots = n_slots;
    H.overflow = (p1 - p0) > n_slots;
    H.t_lo = t_lo;
    H.t_hi = t_hi;
    H.s_lo = t_hi <= t_lo ? 0 : t_lo;
    H.bfirst = bfirst;
    H.ubatch = ubatch;
    H.p0 = p0;
    if (!counts) hdr[u] = H;
    else cls = (t_hi <= t_lo || t_hi - t_lo <= FEE_SPAN) ? 0 : 1;
  }
  if (!counts) return;
  for (int cc = 0; cc < 2; cc++) {
    const unsigned long long m = __ballot(cls == cc);
    if (!m) continue;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&counts[cc], (unsigned long long)__popcll(m));
    base = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    if (cls == cc) hdr[(int64_t)cc * F.U + (int64_t)base + __popcll(m & ((1ull << lane) - 1ull))] = H;
  }
}

// the same tables for another rise time into a buffer of the caller's (128 doubles): the FEE universes pass, which leaves
// ctx->d_fee_tab and its (fee_tab_dt, fee_tab_rt) cache to the launch
int fee_launch_tables(ldsim_ctx* ctx, double dt, double rt, double* tab) {
  hipLaunchKernelGGL(fee_tables_kernel, dim3(1), dim3(64), 0, ctx->stream, dt, rt, tab);
  HIPCHK(hipGetLastError());
  return 0;
}

int fee_launch_chain(ldsim_ctx* ctx, const FeeArgs& F0) {
  if (F0.U == 0) return 0;
  const LdsimConsts& h = ctx->h_consts;
  if (h.n_time_ticks > NT_MAX || h.max_adc_values > A_MAX || h.max_tracks_per_pixel > M_MAX ||
      (h.buffer_risetime > 0 && 10 * h.buffer_risetime / h.time_sampling > 62)) {
    ldsim_set_error("FEE constants exceed the kernel's static tiles");
    return LDSIM_EINVAL;
  }
  // the launch constants: built when the two constants they depend on change, not per launch
  CK(ctx->d_fee_tab.ensure(128 * sizeof(double)));
  if (ctx->fee_tab_dt != h.time_sampling || ctx->fee_tab_rt != h.buffer_risetime) {
    hipLaunchKernelGGL(fee_tables_kernel, dim3(1), dim3(64), 0, ctx->stream, h.time_sampling, h.buffer_risetime, ctx->d_fee_tab.as<double>());
    HIPCHK(hipGetLastError());
    ctx->fee_tab_dt = h.time_sampling;
    ctx->fee_tab_rt = h.buffer_risetime;
  }
  FeeArgs F = F0;
  F.tab = ctx->d_fee_tab.as<double>();
  // (the kernel writes the (hit, slot) entries that exist; everything else of `fractions` reads 0 like the reference's array once
  // fee_clear_unwritten_fractions has run: the dense downloads call it -- clearing 12 KB per pixel in every launch cost 0.45 ms per
  // 100 k segments, and the compact download reads the written entries only)
  const size_t full = (size_t)((h.n_time_ticks + 1) & ~1) * 8;
  // noise: every tick is walked (no idle skipping), so the whole tick axis goes in LDS; a threshold table may hold non-positive
  // entries -- the scan decides per pixel, so the table case keeps the windows only when the constant path would; complete rows: no
  // windows to go by
  const bool skip_idle = !F.batch_keys && !F.noise_z && ((F.thr_table != nullptr) || F.threshold > 0);
  const bool one_class = !skip_idle || !F.win || ctx->fee_one_class || h.n_time_ticks <= FEE_SPAN;
  int rc;
  // (headers [U] or lists [2][U] | counts [2]: fee_hdr_view; the counts sit in the 64 bytes of slack)
  if ((rc = ctx->scratch[SB_FEEHDR].ensure(fee_hdr_view(nullptr, !one_class, F.U).hdr_bytes + 64))) return rc;
  if ((rc = ctx->scratch[SB_FEESLOT].ensure((size_t)F.n_pairs * sizeof(FeeSlot) + 16))) return rc;
  const FeeHdrView V = fee_hdr_view(ctx->scratch[SB_FEEHDR].p, !one_class, F.U);
  FeeHdr* d_hdr = V.hdr;
  FeeSlot* d_slots = ctx->scratch[SB_FEESLOT].as<FeeSlot>();
  unsigned long long* d_counts = V.counts;
  // what ldsim_chain_pixel_truth needs to read this record after the launch: the layout of the headers, and the rows
  ctx->fee_rec = ldsim_ctx::FeeRecord{one_class ? 0 : 1, F.U, F.n_pairs, F.T, h.n_time_ticks, h.max_tracks_per_pixel, h.max_adc_values,
                                      h.time_sampling};
  if (d_counts) HIPCHK(hipMemsetAsync(d_counts, 0, 16, ctx->stream));
  hipLaunchKernelGGL(fee_setup_kernel, dim3((unsigned)((F.U + 255) / 256)), dim3(256), 0, ctx->stream, F, d_slots, d_hdr, d_counts);
  HIPCHK(hipGetLastError());
  if (one_class) {
    if (F.batch_keys)
      hipLaunchKernelGGL((pixel_adc_kernel<FEE_THREADS, true>), dim3((unsigned)F.U), dim3(FEE_THREADS), full, ctx->stream, F, d_hdr, d_slots);
    else
      hipLaunchKernelGGL(pixel_adc_kernel<FEE_THREADS>, dim3((unsigned)F.U), dim3(FEE_THREADS), full, ctx->stream, F, d_hdr, d_slots);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // both launches over the whole grid: a workgroup past its list's count leaves at once (the counts stay on the device: no
  // host round trip); the one-wave launch first
  const unsigned g_small = (unsigned)std::min<int64_t>(F.U, 256 * 24), g_big = (unsigned)std::min<int64_t>(F.U, 256 * 8);
  hipLaunchKernelGGL(pixel_adc_list_kernel<64>, dim3(g_small), dim3(64), (size_t)FEE_SPAN * 8, ctx->stream, F, d_hdr,
                     d_counts, d_slots, true, FEE_SPAN);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(pixel_adc_list_kernel<FEE_THREADS>, dim3(g_big), dim3(FEE_THREADS), full, ctx->stream, F,
                     d_hdr + F.U, d_counts + 1, d_slots, false, 0);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- materialising forms (parity API) ----------------------------------------------------------------------------------
// get_track_pixel_map2, literal (detsim.py:564-607): one thread per unique pixel
__global__ void track_pixel_map_kernel(int64_t* map, const int32_t* unique_pix, int64_t U, const int32_t* pixels,
                                       const int32_t* dist, int64_t S, int P, int max_distance, int M) {
  int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  int32_t upix = unique_pix[u];
  int64_t* row = map + u * M;
  for (int target = 0; target < max_distance; target++)
    for (int64_t itrk = 0; itrk < S; itrk++)
      for (int ipix = 0; ipix < P; ipix++) {
        if (upix != pixels[itrk * P + ipix]) continue;
        if (dist[itrk * P + ipix] == target) {
          int imap = 0;
          while (imap < M) {
            if (row[imap] == itrk) { imap = -1; break; }
            if (row[imap] == -1) break;
            imap++;
          }
          if (imap >= 0 && imap < M) row[imap] = itrk;
        }
        break;
      }
}

// sum_pixel_signals, literal incl. f64 atomics (detsim.py:468-527): thread per (itrk, ipix, itick)
__global__ void sum_pixel_signals_kernel(double* pixels_signals, const float* signals, const double* track_starts,
                                         const int64_t* pim, const int64_t* tpm, double* pts, double* overflow,
                                         int64_t S, int P, int T, int NT, int M, double dt) {
  int64_t pairi = blockIdx.x;
  int64_t itrk = pairi / P;
  int64_t pidx = pim[pairi];
  if (pidx < 0) return;
  int start_tick = (int)py_round(track_starts[itrk] / dt);
  int counter = -99;
  for (int k = 0; k < M; k++)
    if (itrk == tpm[pidx * M + k]) { counter = k; break; }
  if (counter < 0) {
    if (threadIdx.x == 0) overflow[pidx] = 1;
    return;
  }
  for (int itick = threadIdx.x; itick < T; itick += blockDim.x) {
    int itime = start_tick + itick;
    if (itime < NT && itime > -1) {
      double v = signals[pairi * T + itick];
      atomicAdd(&pixels_signals[pidx * NT + itime], v);
      if (pts) atomicAdd(&pts[(pidx * NT + itime) * M + counter], v);
    }
  }
}

// get_adc_values on dense arrays (fee.py:517-655): workgroup per pixel, same scan as the chain
__global__ void __launch_bounds__(FEE_THREADS) adc_dense_kernel(const LdsimConsts* c, const double* pixels_signals,
                                                                const double* pts, int64_t U, int NT, int M,
                                                                const double* thresholds, double time_padding,
                                                                double t_stop, const float* noise_z, int noise_nd,
                                                                int32_t* n_draws, double* adc_list, double* adc_ticks,
                                                                double* fractions) {
  const int64_t u = blockIdx.x;
  if (u >= U) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int A = c->max_adc_values;
  const double dt = c->time_sampling, rt = c->buffer_risetime;
  __shared__ double S[NT_MAX];
  __shared__ HitRec hits[A_MAX];
  __shared__ double wtap[64], G[64];
  __shared__ int s_nh;
  const int ntap = rt > 0 ? (int)ceil(10 * rt / dt) : 0;  // floor(ic - 10*rt/dt) == ic - ceil(10*rt/dt)
  if (tid <= ntap && rt > 0) wtap[tid] = exp((-tid) * dt / rt) * (1 - exp(-dt / rt));
  for (int t = tid; t < NT; t += FEE_THREADS) S[t] = pixels_signals[u * NT + t];
  __syncthreads();
  if (tid == 0) {
    double acc = 0;
    for (int d = 0; d <= ntap; d++) {
      acc += (rt > 0 ? wtap[d] : 1.0) * dt;
      G[d] = acc;
    }
  }
  if (wv == 0) {
    int nd = 0;
    int nh = adc_scan(c, S, NT, t_stop, thresholds[u], time_padding, lane, hits, wtap, ntap,
                      TableNoise{noise_z ? noise_z + u * (int64_t)noise_nd : nullptr}, &nd);
    if (lane == 0) {
      s_nh = nh;
      if (n_draws) n_draws[u] = nd;
    }
  }
  __syncthreads();
  const int nh = s_nh;
  for (int h = tid; h < A; h += FEE_THREADS) {
    adc_list[u * A + h] = h < nh ? hits[h].q : 0.0;
    adc_ticks[u * A + h] = h < nh ? hits[h].tick : 0.0;
  }
  if (fractions && pts) {
    double* fr = fractions + u * (int64_t)A * M;
    for (int i = tid; i < A * M; i += FEE_THREADS) fr[i] = 0;
    __syncthreads();
    for (int k = wv; k < M; k += FEE_THREADS / 64)
      for (int h = 0; h < nh; h++) {
        int lr = hits[h].lr, b = hits[h].b;
        int hi = b < NT - 1 ? b : NT - 1;
        double acc = 0;
        for (int jc = lr + lane; jc <= hi; jc += 64) {
          int d = b - jc;
          acc += pts[(u * NT + jc) * M + k] * (rt > 0 ? G[d < ntap ? d : ntap] : dt);
        }
        acc = wave_sum(acc);
        if (lane == 0) fr[h * M + k] = hits[h].tq > 0 ? acc / hits[h].tq : acc;
      }
  }
}

__global__ void digitize_kernel(const LdsimConsts* c, const double* q, const double* gain_list, double* out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double gain = gain_list ? gain_list[i] : c->gain * (1e-3 * (1e-6 * 1.0)) / 1.0;
  out[i] = digitize_one(c, q[i], gain);
}

int fee_launch_track_pixel_map(ldsim_ctx* ctx, int64_t* map, const int32_t* upix, int64_t U, const int32_t* pixels,
                               const int32_t* dist, int64_t S, int P, int max_distance, int M) {
  if (U == 0) return 0;
  hipLaunchKernelGGL(track_pixel_map_kernel, dim3((unsigned)((U + 63) / 64)), dim3(64), 0, ctx->stream, map, upix, U,
                     pixels, dist, S, P, max_distance, M);
  HIPCHK(hipGetLastError());
  return 0;
}
int fee_launch_sum_pixel_signals(ldsim_ctx* ctx, double* ps, const float* signals, const double* starts,
                                 const int64_t* pim, const int64_t* tpm, double* pts, double* ovf, int64_t S, int P,
                                 int T, int NT, int M) {
  if (S * P == 0) return 0;
  hipLaunchKernelGGL(sum_pixel_signals_kernel, dim3((unsigned)(S * P)), dim3(256), 0, ctx->stream, ps, signals, starts,
                     pim, tpm, pts, ovf, S, P, T, NT, M, ctx->h_consts.time_sampling);
  HIPCHK(hipGetLastError());
  return 0;
}
int fee_launch_adc_dense(ldsim_ctx* ctx, const double* ps, const double* pts, int64_t U, int NT, int M,
                         const double* thr, double time_padding, double t_stop, const float* noise_z, int noise_nd,
                         int32_t* n_draws, double* adc, double* ticks, double* frac) {
  if (U == 0) return 0;
  const LdsimConsts& h = ctx->h_consts;
  if (NT > NT_MAX || h.max_adc_values > A_MAX || (h.buffer_risetime > 0 && 10 * h.buffer_risetime / h.time_sampling > 62)) {
    ldsim_set_error("FEE constants exceed the kernel's static tiles");
    return LDSIM_EINVAL;
  }
  hipLaunchKernelGGL(adc_dense_kernel, dim3((unsigned)U), dim3(FEE_THREADS), 0, ctx->stream, ctx->d_consts.as<LdsimConsts>(), ps, pts, U,
                     NT, M, thr, time_padding, t_stop, noise_z, noise_nd, n_draws, adc, ticks, frac);
  HIPCHK(hipGetLastError());
  return 0;
}
int fee_launch_digitize(ldsim_ctx* ctx, const double* q, const double* gain, double* out, int64_t n) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(digitize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_consts.as<LdsimConsts>(), q,
                     gain, out, n);
  HIPCHK(hipGetLastError());
  return 0;
}
