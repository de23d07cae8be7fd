// fee_record.h -- the set-up record of a chain launch's FEE stage: written by fee_setup_kernel, read by the pixel_adc kernels
// (kernels_fee.hip) and, after the launch, through the one reader of fee_reader.h by pixel truth (kernels_pixtruth.hip), the
// pixel waveforms (kernels_pixwave.hip) and the FEE and charge universes (kernels_feeuni.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

// What the set-up pass (fee_setup_kernel) leaves per pixel: a header, and one row per slot in a pool indexed like the sorted pair
// list (slot k of the pixel whose pairs start at p0: row p0 + k), so the record is sized by the slots that exist, not by M.
struct __attribute__((aligned(32))) FeeHdr {
  int32_t u;            // the unique pixel
  int32_t n_slots;      // valid pairs, at most M
  int32_t overflow;     // the pixel has pairs beyond its slots
  int32_t t_lo, t_hi;   // the ticks the slots' windows cover (t_lo = NT, t_hi = 0: none)
  int32_t s_lo;         // first tick held in LDS by the one-wave form
  int32_t bfirst;       // first relative segment index of the pixel's batch
  int32_t ubatch;
  int64_t p0;           // first pair
  int64_t pad;
};
struct __attribute__((aligned(16))) FeeSlot {
  int32_t start;        // tick of the row's element 0 on the pixel's time axis (detsim.py:506)
  int32_t w0, w1;       // the ticks of the row tracks_current wrote
  int32_t track;        // segment index in the batch (track_pixel_map)
};

// The headers in their slot (SB_FEEHDR).  lists = 0: headers [U], header u at index u.  lists = 1: two lists [2][U] (list 1 behind
// list 0's U places), and behind them the two lists' counts u64 [2].  hdr_bytes: the headers alone (where the counts start);
// bytes: with the counts.
struct FeeHdrView {
  FeeHdr* hdr;
  unsigned long long* counts;   // [2], or NULL without lists
  size_t hdr_bytes, bytes;
};
static inline FeeHdrView fee_hdr_view(void* base, int lists, int64_t U) {
  const size_t hb = (size_t)U * sizeof(FeeHdr) * (lists ? 2 : 1);
  return FeeHdrView{(FeeHdr*)base, lists && base ? (unsigned long long*)((char*)base + hb) : nullptr, hb, hb + (lists ? 16 : 0)};
}
