// kernels_pixwave.hip -- pixel current waveforms: the summed induced current S[t] of every unique pixel of the last chain launch,
// zero-suppressed into spans (include/ldsim.h, "pixel current waveforms"; the definition in numpy: larndsim_amd/pixel_waveforms.py).
//
// A sibling of kernels_pixtruth.hip: it reads the same two things the launch left in HBM, the per-pair current rows (f32
// [n_pairs][T]) and the FEE set-up record (fee_record.h), and changes nothing of the chain.  A wave per pixel, four pixels per
// workgroup; lane k holds slot k's window (fee_reader.h: FeeWavePixel, M <= 64 = the wave).  The pixel's time axis is cut into 64-tick words (word c: the ticks
// [64 c, 64 c + 64)), lane l owning tick 64 c + l, and fee_wave_chunk_sum (fee_reader.h, pixel_truth_kernel's pass B too) forms S of a
// word as pixel_adc_body does: f64, the slots' rows added in slot order.
//   count  per word one 64-bit ballot of |S| > min_abs_current; the kept ticks of word c are the active ticks of the words
//          c - 1, c, c + 1 dilated by pad_ticks <= 64; spans are the rising edges, samples the popcount: per pixel two counts
//   scan   two exclusive 64-bit scans over the pixels (row order): a pixel's first span row and first sample
//   fill   S again (the rows come from L2 or HBM once more; nothing of size U x N_t is kept between the passes): the kept ticks
//          are written as f32 at their places, and the lane behind a span's last tick writes its row
// No atomics: every position is a function of the launch alone.
#include "launchers.h"
#include "fee_reader.h"

#define PW_WAVES 4       // pixels per workgroup

__device__ __forceinline__ unsigned long long pw_low_bits(int n) {      // the n lowest bits, 0 <= n <= 64
  return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}

// The walk over one pixel's words, shared by the two passes.  FILL = false: counts only.
template <bool FILL>
__device__ __forceinline__ void pw_walk(const float* __restrict__ waves, const FeeWavePixel& P, int T, int NT, int lane, double thr, int pad,
                                        unsigned long long& n_spans, unsigned long long& n_samples,
                                        // fill: the pixel's first span row and first sample, the sizes of the two arrays, the row's identity
                                        unsigned long long span0, unsigned long long samp0, unsigned long long spans_cap,
                                        unsigned long long samples_cap, int32_t pixel_id, int32_t batch,
                                        LdsimPixelWaveSpan* __restrict__ spans, float* __restrict__ samples) {
  n_spans = n_samples = 0;
  if (P.t_hi <= P.t_lo) return;                                 // (no slot, or no window inside the axis)
  const int NW = (NT + 63) >> 6;
  const int c_lo = P.t_lo >> 6, c_hi = (P.t_hi + 63) >> 6;      // words that can hold an active tick: [c_lo, c_hi), c_hi <= NW
  const int c_first = max(c_lo - 1, 0), c_last = min(c_hi, NW - 1);      // words that can hold a kept tick (pad <= 64)
  const unsigned long long lt = (1ull << lane) - 1ull;          // the lanes below this one
  unsigned long long a_prev = 0, a_cur = 0, a_next = 0;         // activity of the words c - 1, c, c + 1
  double s_cur = 0, s_next = 0;
  if (c_first >= c_lo) {
    s_cur = fee_wave_chunk_sum(waves, P, T, c_first << 6, lane);
    a_cur = __ballot(fabs(s_cur) > thr);
  }
  unsigned long long carry = 0;                                 // the last tick of the word before was kept
  int open_t = 0;                                               // fill: first tick and first sample of the span that is open
  unsigned long long open_s = 0;
  for (int c = c_first; c <= c_last; c++) {
    s_next = 0;
    a_next = 0;
    if (c + 1 >= c_lo && c + 1 < c_hi) {
      s_next = fee_wave_chunk_sum(waves, P, T, (c + 1) << 6, lane);
      a_next = __ballot(fabs(s_next) > thr);
    }
    // kept: an active tick within pad of this one, in this word or in a neighbour
    const int b_lo = lane - pad, b_hi = lane + pad;             // [-64, 127]
    bool k = (a_cur & pw_low_bits(min(b_hi, 63) + 1) & ~pw_low_bits(max(b_lo, 0))) != 0;
    if (b_lo < 0) k = k || (a_prev >> (64 + b_lo)) != 0;
    if (b_hi > 63) k = k || (a_next & pw_low_bits(b_hi - 63)) != 0;
    k = k && (c << 6) + lane < NT;
    const unsigned long long kept = __ballot(k);
    const unsigned long long before = (kept << 1) | carry;      // bit l: tick l - 1 was kept
    const unsigned long long rises = kept & ~before;            // a span begins
    if (!FILL) {
      n_spans += (unsigned long long)__popcll(rises);
    } else {
      const unsigned long long pos = samp0 + n_samples + (unsigned long long)__popcll(kept & lt);
      if (k && pos < samples_cap) samples[pos] = (float)s_cur;
      const unsigned long long ends = ~kept & before;           // bit l: the open span ended with tick l - 1
      if ((ends >> lane) & 1ull) {
        const unsigned long long r = rises & lt;                // where it began: the last rise below, or in an earlier word
        int t_begin = open_t;
        unsigned long long s_begin = open_s;
        if (r) {
          const int b = 63 - __clzll((long long)r);
          t_begin = (c << 6) + b;
          s_begin = samp0 + n_samples + (unsigned long long)__popcll(kept & pw_low_bits(b));
        }
        const unsigned long long row = span0 + n_spans + (unsigned long long)__popcll(ends & lt);
        if (row < spans_cap)
          spans[row] = LdsimPixelWaveSpan{(int32_t)P.u, pixel_id, batch, t_begin, (c << 6) + lane - t_begin, 0, (int64_t)s_begin};
      }
      if (kept >> 63) {                                         // open into the next word: begun at this word's last rise, if it has one
        if (rises) {
          const int b = 63 - __clzll((long long)rises);
          open_t = (c << 6) + b;
          open_s = samp0 + n_samples + (unsigned long long)__popcll(kept & pw_low_bits(b));
        }
      }
      n_spans += (unsigned long long)__popcll(ends);
    }
    n_samples += (unsigned long long)__popcll(kept);
    carry = kept >> 63;
    a_prev = a_cur;
    a_cur = a_next;
    s_cur = s_next;
  }
  if (FILL && carry) {                                          // the span that reaches the end of the axis (or of the last word)
    const int t_end = min((c_last + 1) << 6, NT);
    const unsigned long long row = span0 + n_spans;
    if (lane == 0 && row < spans_cap)
      spans[row] = LdsimPixelWaveSpan{(int32_t)P.u, pixel_id, batch, open_t, t_end - open_t, 0, (int64_t)open_s};
    n_spans++;
  }
}

// count[u] = the pixel's spans, count[U + 1 + u] = its samples (two arrays of U + 1 places, zeroed before; place U stays 0 so the
// exclusive scans end in the totals)
__global__ void __launch_bounds__(64 * PW_WAVES) pixel_wave_count_kernel(FeeRecArgs R, const int32_t* __restrict__ hit_count, double thr,
                                                                         int pad, int hits_only, unsigned long long* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * PW_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  FeeWavePixel P;
  if (!fee_wave_pixel(R, w, lane, P)) return;
  if (hits_only && hit_count[P.u] <= 0) return;
  unsigned long long n_spans, n_samples;
  pw_walk<false>(R.waves, P, R.T, R.NT, lane, thr, pad, n_spans, n_samples, 0, 0, 0, 0, 0, 0, nullptr, nullptr);
  if (lane == 0) {
    count[P.u] = n_spans;
    count[R.U + 1 + P.u] = n_samples;
  }
}

__global__ void __launch_bounds__(64 * PW_WAVES) pixel_wave_fill_kernel(
    FeeRecArgs R, const int32_t* __restrict__ upix, const int32_t* __restrict__ ubatch, double thr, int pad,
    const unsigned long long* __restrict__ count, const unsigned long long* __restrict__ first, unsigned long long spans_cap,
    unsigned long long samples_cap, LdsimPixelWaveSpan* __restrict__ spans, float* __restrict__ samples) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * PW_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  FeeWavePixel P;
  if (!fee_wave_pixel(R, w, lane, P)) return;
  if (count[P.u] == 0) return;                                  // (nothing kept, or not selected: a kept tick makes a span)
  unsigned long long n_spans, n_samples;
  pw_walk<true>(R.waves, P, R.T, R.NT, lane, thr, pad, n_spans, n_samples, first[P.u], first[R.U + 1 + P.u], spans_cap, samples_cap,
                upix[P.u], ubatch[P.u], spans, samples);
}

// the dense form of the rows [u_begin, u_end): (float)S[t] into out [u_end - u_begin][NT], zeroed before
__global__ void __launch_bounds__(64 * PW_WAVES) pixel_wave_dense_kernel(FeeRecArgs R, int64_t u_begin, int64_t u_end,
                                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * PW_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  FeeWavePixel P;
  if (!fee_wave_pixel(R, w, lane, P)) return;
  if (P.u < u_begin || P.u >= u_end) return;
  float* row = out + (P.u - u_begin) * (int64_t)R.NT;
  for (int base = (P.t_lo >> 6) << 6; base < P.t_hi; base += 64) {
    const double S = fee_wave_chunk_sum(R.waves, P, R.T, base, lane);
    if (base + lane < R.NT) row[base + lane] = (float)S;
  }
}

extern "C" int ldsim_chain_pixel_waveforms(ldsim_ctx* ctx, double min_abs_current, int32_t pad_ticks, int32_t hits_only, int64_t sizes[3]) {
  LDSIM_ENTER(ctx);
  if (!ctx || !sizes) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
  sizes[0] = sizes[1] = sizes[2] = 0;
  if (!(min_abs_current >= 0) || !(min_abs_current < HUGE_VAL)) {
    ldsim_set_error("pixel waveforms: min_abs_current %g must be finite and >= 0", min_abs_current);
    return LDSIM_EINVAL;
  }
  if (pad_ticks < 0 || pad_ticks > 64) {
    ldsim_set_error("pixel waveforms: pad_ticks %d must lie in [0, 64]", (int)pad_ticks);
    return LDSIM_EINVAL;
  }
  CK(launch_need_record(ctx, "ldsim_chain_pixel_waveforms"));
  HIPCHK(hipSetDevice(ctx->device));
  const ChainView v = chain_view(ctx);      // (the pass grows its own buffers and SB_SORTTMP only)
  const int64_t U = v.U;
  ctx->pw_gen = -1;                         // (until the pass is complete)
  ctx->pw_n[0] = ctx->pw_n[1] = 0;
  sizes[2] = U ? ctx->fee_rec.NT : ctx->h_consts.n_time_ticks;
  if (U == 0) {
    ctx->pw_gen = ctx->out_gen;
    return 0;
  }
  const ldsim_ctx::FeeRecord& R = ctx->fee_rec;
  const FeeRecArgs F = fee_rec_args(ctx, v);
  hipStream_t st = ctx->stream;
  const size_t n_cnt = 2 * ((size_t)U + 1);
  CK(pass_ensure(ctx->pw_sel, 2 * n_cnt * 8, "pixel waveforms", "the counts"));
  unsigned long long *count = ctx->pw_sel.as<unsigned long long>(), *first = count + n_cnt;
  HIPCHK(hipMemsetAsync(count, 0, n_cnt * 8, st));
  const dim3 grid((unsigned)((U + PW_WAVES - 1) / PW_WAVES)), block(64 * PW_WAVES);
  for (int k = 0; k < 4; k++) CK(ctx->pw_ev[k].ensure());
  ctx->pw_filled = false;
  HIPCHK(hipEventRecord(ctx->pw_ev[0], st));
  hipLaunchKernelGGL(pixel_wave_count_kernel, grid, block, 0, st, F, v.hit_count, min_abs_current, (int)pad_ticks,
                     (int)(hits_only != 0), count);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->pw_ev[1], st));
  // 64-bit from the start: the samples of a launch can pass 2^31.  Place U of each array is 0, so first[U] is the total.
  CK(sort_exclusive_scan_u64(ctx, count, first, U + 1));
  CK(sort_exclusive_scan_u64(ctx, count + U + 1, first + U + 1, U + 1));
  unsigned long long total[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&total[0], first + U, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&total[1], first + 2 * U + 1, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // every span holds a sample and every pixel at most N_t of them: anything else is not this launch's record
  if (total[0] > total[1] || total[1] > (unsigned long long)U * (unsigned long long)R.NT) {
    ldsim_set_error("pixel waveforms: the count pass found %llu spans and %llu samples on %lld pixels of %d ticks", total[0], total[1],
                    (long long)U, (int)R.NT);
    return LDSIM_ESTATE;
  }
  const size_t b_spans = (size_t)total[0] * sizeof(LdsimPixelWaveSpan);
  CK(pass_ensure(ctx->pw_out, b_spans + (size_t)total[1] * 4, "pixel waveforms", "the spans and samples"));
  if (total[0]) {
    HIPCHK(hipEventRecord(ctx->pw_ev[2], st));
    hipLaunchKernelGGL(pixel_wave_fill_kernel, grid, block, 0, st, F, v.upix, v.ubatch, min_abs_current, (int)pad_ticks, count, first,
                       total[0], total[1], (LdsimPixelWaveSpan*)ctx->pw_out.p, (float*)((char*)ctx->pw_out.p + b_spans));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->pw_ev[3], st));
    ctx->pw_filled = true;
  }
  ctx->pw_n[0] = (int64_t)total[0];
  ctx->pw_n[1] = (int64_t)total[1];
  ctx->pw_gen = ctx->out_gen;
  sizes[0] = ctx->pw_n[0];
  sizes[1] = ctx->pw_n[1];
  return 0;
}

static int pw_need_pass(ldsim_ctx* ctx) {
  if (ctx->pw_gen < 0 || ctx->pw_gen != ctx->out_gen) {
    ldsim_set_error("ldsim_chain_pixel_waveforms has not run for the last chain launch");
    return LDSIM_ESTATE;
  }
  return 0;
}

extern "C" int ldsim_chain_pixel_waveforms_download(ldsim_ctx* ctx, LdsimPixelWaveSpan* spans, float* samples) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(pw_need_pass(ctx));
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t b_spans = (size_t)ctx->pw_n[0] * sizeof(LdsimPixelWaveSpan), b_samples = (size_t)ctx->pw_n[1] * 4;
  if (spans && b_spans) HIPCHK(hipMemcpyAsync(spans, ctx->pw_out.p, b_spans, hipMemcpyDeviceToHost, st));
  if (samples && b_samples) HIPCHK(hipMemcpyAsync(samples, (const char*)ctx->pw_out.p + b_spans, b_samples, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int ldsim_chain_pixel_waveforms_ms(ldsim_ctx* ctx, double* count_ms, double* fill_ms) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(pw_need_pass(ctx));
  if (count_ms) *count_ms = 0;
  if (fill_ms) *fill_ms = 0;
  if (ctx->chain_U == 0) return 0;                              // (no kernel ran)
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->pw_ev[0], ctx->pw_ev[1]));
  if (count_ms) *count_ms = ms;
  if (ctx->pw_filled) {
    HIPCHK(hipEventElapsedTime(&ms, ctx->pw_ev[2], ctx->pw_ev[3]));
    if (fill_ms) *fill_ms = ms;
  }
  return 0;
}

extern "C" int ldsim_chain_pixel_waveforms_dense(ldsim_ctx* ctx, int64_t u_begin, int64_t u_end, float* S) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(launch_need_record(ctx, "ldsim_chain_pixel_waveforms_dense"));
  const int64_t U = ctx->chain_U;
  if (u_begin < 0 || u_end < u_begin || u_end > U) {
    ldsim_set_error("pixel waveforms: rows [%lld, %lld) are not a range of the launch's %lld unique pixels", (long long)u_begin,
                    (long long)u_end, (long long)U);
    return LDSIM_EINVAL;
  }
  if (u_end == u_begin) return 0;
  if (!S) { ldsim_set_error("pixel waveforms: null array for %lld rows", (long long)(u_end - u_begin)); return LDSIM_EINVAL; }
  HIPCHK(hipSetDevice(ctx->device));
  const ChainView v = chain_view(ctx);
  const ldsim_ctx::FeeRecord& R = ctx->fee_rec;
  hipStream_t st = ctx->stream;
  const size_t bytes = (size_t)(u_end - u_begin) * (size_t)R.NT * 4;
  CK(pass_ensure(ctx->pw_dense, bytes, "pixel waveforms", "the dense rows"));
  HIPCHK(hipMemsetAsync(ctx->pw_dense.p, 0, bytes, st));
  hipLaunchKernelGGL(pixel_wave_dense_kernel, dim3((unsigned)((U + PW_WAVES - 1) / PW_WAVES)), dim3(64 * PW_WAVES), 0, st,
                     fee_rec_args(ctx, v), u_begin, u_end, ctx->pw_dense.as<float>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(S, ctx->pw_dense.p, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
