// fee_reader.h -- the one reader of the FEE set-up record (fee_record.h) for the passes that run after a chain launch: pixel
// truth (kernels_pixtruth.hip), pixel waveforms (kernels_pixwave.hip), FEE and charge universes (kernels_feeuni.hip).  The
// record as the kernels take it, the w-th header under one rule of refusal, a slot's window, and the wave-level form: a pixel
// with slot k's window in lane k and S of a 64-tick chunk.  Whatever the record holds, nothing outside the launch's buffers is
// touched.  kernels_fee.hip does not include this: pixel_adc_body reads the record it has just written, unclipped.
#pragma once
#include "ldsim_args.h"
#include "wave_ops.h"

struct FeeRecArgs {
  const FeeHdr* hdr;                        // [U], or [2][U] with counts
  const unsigned long long* counts;         // [2] with lists, else NULL
  const FeeSlot* slots;                     // [n_pairs]
  const float* waves;                       // [n_pairs][T]
  int64_t U, n_pairs;
  int32_t T, NT, M;
};
static inline FeeRecArgs fee_rec_args(const ldsim_ctx* ctx, const ChainView& cv) {
  const ldsim_ctx::FeeRecord& R = ctx->fee_rec;
  return FeeRecArgs{cv.fee.hdr, cv.fee.counts, cv.fee_slots, cv.waves, cv.U, R.n_pairs, R.T, R.NT, R.M};
}

// The w-th header, 0 <= w < U: header w, or (two lists, the second behind the first's U places) the w-th of list 0 followed by
// list 1; n_slots clipped to M.  false: the record does not describe the launch's buffers.  No lane operations: a thread, a wave
// or a workgroup may call it (a wave-level caller makes what it needs uniform itself).  No return between the checks, and & for
// && on the counts: the two counts come in one trip to memory and the header's fields in one more, not one trip per check
// (measured: a return after each check cost pixel_adc_universes_kernel 0.08 ms per 195 k pixels).
__device__ __forceinline__ bool fee_rec_header(const FeeRecArgs& R, int64_t w, FeeHdr& H, int& n_slots) {
  const int64_t U = R.U;
  int64_t idx = w;
  bool ok = true;
  if (R.counts) {
    const int64_t c0 = (int64_t)R.counts[0], c1 = (int64_t)R.counts[1];
    ok = (c0 >= 0) & (c0 <= U) & (c1 >= 0) & (c0 + c1 == U);
    if (ok && w >= c0) idx = U + (w - c0);
  }
  H = FeeHdr{};
  if (ok) H = R.hdr[idx];
  n_slots = H.n_slots < R.M ? H.n_slots : R.M;
  return ok && H.u >= 0 && H.u < U && n_slots >= 0 && n_slots <= 64 && H.p0 >= 0 && H.p0 <= R.n_pairs - n_slots;
}

// A slot's window: the row's element 0 sits at tick st, and the ticks [lo, hi) of the pixel's axis are the ones its row is
// summed over (pixel_adc_body: detsim.py:516-520), clipped to the row's T elements and to the axis.
struct FeeWindow {
  int st, lo, hi;
};
__device__ __forceinline__ FeeWindow fee_slot_window(const FeeSlot& sl, int T, int NT) {
  return FeeWindow{sl.start, max(sl.start + max(sl.w0, 0), 0), min(sl.start + min(sl.w1, T), NT)};
}

// What a wave needs of its pixel: the header resolved, slot k's window in lane k (M <= 64 = the wave).
struct FeeWavePixel {
  int64_t u, p0;
  int n_slots, t_lo, t_hi;                  // (wave-uniform) the slots; the ticks their windows cover, inside the axis
  FeeWindow win;                            // lane k: slot k's; empty behind the last slot
};
// w is wave-uniform.  false: the wave has no pixel, or the record is refused
__device__ __forceinline__ bool fee_wave_pixel(const FeeRecArgs& R, int64_t w, int lane, FeeWavePixel& P) {
  if (w >= R.U) return false;
  FeeHdr H;
  int n_slots;
  if (!fee_rec_header(R, w, H, n_slots)) return false;
  P.u = H.u;
  P.p0 = H.p0;
  P.n_slots = __builtin_amdgcn_readfirstlane(n_slots);
  P.t_lo = __builtin_amdgcn_readfirstlane(max(H.t_lo, 0));
  P.t_hi = __builtin_amdgcn_readfirstlane(min(H.t_hi, R.NT));
  P.win = FeeWindow{0, 0, 0};
  if (lane < P.n_slots) P.win = fee_slot_window(R.slots[P.p0 + lane], R.T, R.NT);
  return true;
}

// S[base + lane]: the slots that cover the tick, added in slot order in f64 (0 where no window reaches, and behind N_t), as
// pixel_adc_body forms it.  The one place a wave forms S.  One row and one trip to memory per slot: pixel_adc_body's grouped row
// loads (fee_row_load, FEE_LG) are not carried over; that changes speed and wants a measurement of its own.
__device__ __forceinline__ double fee_wave_chunk_sum(const float* __restrict__ waves, const FeeWavePixel& P, int T, int base, int lane) {
  const int t = base + lane;
  double S = 0;
  for (int k = 0; k < P.n_slots; k++) {
    const int lo_k = wave_lane_i32(P.win.lo, k), hi_k = wave_lane_i32(P.win.hi, k);
    if (hi_k <= base || lo_k >= base + 64) continue;           // (wave-uniform)
    const int64_t row = (P.p0 + k) * (int64_t)T - wave_lane_i32(P.win.st, k);      // element of tick 0 (the ticks [lo_k, hi_k) lie inside the row)
    if (t >= lo_k && t < hi_k) S += (double)waves[row + t];
  }
  return S;
}
