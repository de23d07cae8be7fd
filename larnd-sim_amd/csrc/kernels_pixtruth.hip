// kernels_pixtruth.hip -- pixel charge truth: the induced charge per unique pixel and per (pixel, track) of the last chain
// launch, reduced from what the launch left in HBM (include/ldsim.h, "pixel charge truth").
//
// Nothing of the reference is mirrored: its output ends in hits.  The pass reads the per-pair current rows once (f32
// [n_pairs][T], the only large input) and the FEE set-up record (fee_record.h): per pixel a header, per slot its start tick,
// written window and track.  A wave per pixel, four pixels per workgroup; lane k holds slot k's window (fee_reader.h: FeeWavePixel,
// M <= 64 = the wave), so the slot loops read it with readlane and nothing goes through LDS.
//   pass A  per slot, the lanes stride over the slot's window (256 contiguous bytes per wave instruction) and a DPP wave sum
//           follows: q_track, the read of the rows from HBM
//   pass B  the pixel's ticks [t_lo, t_hi) in 64-tick chunks, every lane summing in slot order the slots that cover its tick:
//           S[t] by fee_wave_chunk_sum, as pixel_adc_body forms it, so q_induced and q_abs need no S array (the rows come from L2 now)
// then a selection on the device (flags, two exclusive scans, a gather) into the compact form.
#include "launchers.h"
#include "fee_reader.h"

#define PT_WAVES 4       // pixels per workgroup

__global__ void __launch_bounds__(64 * PT_WAVES) pixel_truth_kernel(
    FeeRecArgs R, double dt, double* __restrict__ q_induced, double* __restrict__ q_abs, double* __restrict__ q_track,
    int32_t* __restrict__ n_slots_out) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * PT_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (a record that is not this launch's is refused on the host; nothing outside the buffers is touched whatever it holds)
  FeeWavePixel P;
  if (!fee_wave_pixel(R, w, lane, P)) return;
  const float* __restrict__ waves = R.waves;
  const int T = R.T, M = R.M;
  // ---- pass A: q_track ------------------------------------------------------------------------------------------------
  // A lane owns the ticks congruent to it mod 64, like the FEE sum, and adds them in rising order: the order of the sum is the
  // pixel's own, whatever else the launch holds (the same bits at any chunking of the batches).
  double q_mine = 0;
  for (int k = 0; k < P.n_slots; k++) {
    const int st_k = wave_lane_i32(P.win.st, k), lo_k = wave_lane_i32(P.win.lo, k), hi_k = wave_lane_i32(P.win.hi, k);
    const int64_t row = (P.p0 + k) * (int64_t)T - st_k;        // element of tick 0 (the ticks [lo_k, hi_k) lie inside the row)
    double acc = 0;
    for (int t = lo_k + ((lane - lo_k) & 63); t < hi_k; t += 64) acc += (double)waves[row + t];
    acc = wave_add_f64(acc);
    if (lane == k) q_mine = acc * dt;
  }
  // ---- pass B: S[t] over the pixel's ticks in 64-tick chunks (fee_wave_chunk_sum: slots added in slot order) ------------------
  double acc_i = 0, acc_a = 0;
  for (int base = P.t_lo; base < P.t_hi; base += 64) {
    const double S = fee_wave_chunk_sum(waves, P, T, base, lane);
    acc_i += S;
    acc_a += fabs(S);
  }
  acc_i = wave_add_f64(acc_i);
  acc_a = wave_add_f64(acc_a);
  if (lane == 0) {
    q_induced[P.u] = acc_i * dt;
    q_abs[P.u] = acc_a * dt;
    n_slots_out[P.u] = P.n_slots;
  }
  if (lane < M) q_track[P.u * M + lane] = q_mine;              // (0 behind the last slot)
}

// the current samples pixel_truth_kernel's pass A sums (timing tools: the bytes it reads from the rows are 4 x that): a thread per
// header, resolved and clipped as there; one atomic per workgroup
__global__ void __launch_bounds__(256) pixel_truth_samples_kernel(FeeRecArgs R, unsigned long long* __restrict__ total) {
  __shared__ unsigned long long s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long mine = 0;
  FeeHdr H;
  int n_slots;
  if (w < R.U && fee_rec_header(R, w, H, n_slots))
    for (int k = 0; k < n_slots; k++) {
      const FeeWindow W = fee_slot_window(R.slots[H.p0 + k], R.T, R.NT);
      if (W.hi > W.lo) mine += (unsigned long long)(W.hi - W.lo);
    }
  if (mine) atomicAdd(&s_sum, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_sum) atomicAdd(total, s_sum);
}

// a pixel is kept when it holds a hit or saw at least min_abs of |charge|; its track entries: its slots
__global__ void __launch_bounds__(256) pixel_truth_flag_kernel(int64_t U, const int32_t* __restrict__ hit_count,
                                                               const double* __restrict__ q_abs, const int32_t* __restrict__ n_slots,
                                                               double min_abs, int32_t* __restrict__ keep, int32_t* __restrict__ cnt) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= U) return;
  const int k = hit_count[u] > 0 || q_abs[u] >= min_abs;
  keep[u] = k;
  cnt[u] = k ? n_slots[u] : 0;
}

__global__ void __launch_bounds__(256) pixel_truth_gather_kernel(
    int64_t U, int A, int M, const int32_t* __restrict__ keep, const int32_t* __restrict__ o_keep, const int32_t* __restrict__ o_cnt,
    const int32_t* __restrict__ upix, const int32_t* __restrict__ ubatch, const int32_t* __restrict__ hit_count,
    const double* __restrict__ adc_list, const int64_t* __restrict__ tpm, const double* __restrict__ q_induced,
    const double* __restrict__ q_abs, const double* __restrict__ q_track, const int32_t* __restrict__ n_slots,
    LdsimPixelTruthRow* __restrict__ rows, LdsimPixelTruthTrack* __restrict__ entries) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= U || !keep[u]) return;
  int nh = hit_count[u];
  nh = nh < 0 ? 0 : (nh > A ? A : nh);
  const int nt = n_slots[u];
  double qh = 0;
  for (int h = 0; h < nh; h++) qh += adc_list[u * A + h];      // (slot 0 up)
  LdsimPixelTruthRow r;
  r.row = (int32_t)u; r.pixel_id = upix[u]; r.batch = ubatch[u]; r.n_hits = nh; r.n_tracks = nt; r.pad = 0;
  r.q_hits = qh; r.q_induced = q_induced[u]; r.q_abs = q_abs[u];
  rows[o_keep[u]] = r;
  for (int k = 0; k < nt; k++) entries[(int64_t)o_cnt[u] + k] = LdsimPixelTruthTrack{tpm[u * M + k], q_track[u * M + k]};
}

// the dense arrays of ctx->pt_dense for U rows of M slots
struct PtDense {
  double *q_induced, *q_abs, *q_track;
  int32_t* n_slots;
  size_t bytes;
};
static size_t pt_dense_bytes(int64_t U, int M) { return (size_t)U * (2 + (size_t)M) * 8 + (size_t)U * 4; }
static PtDense pt_dense_of(void* p, int64_t U, int M) {
  PtDense d;
  d.q_induced = (double*)p;
  d.q_abs = d.q_induced + U;
  d.q_track = d.q_abs + U;
  d.n_slots = (int32_t*)(d.q_track + U * (int64_t)M);
  d.bytes = pt_dense_bytes(U, M);
  return d;
}

extern "C" int ldsim_chain_pixel_truth(ldsim_ctx* ctx, double min_abs_charge, int64_t sizes[2]) {
  LDSIM_ENTER(ctx);
  if (!ctx || !sizes) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
  sizes[0] = sizes[1] = 0;
  if (!(min_abs_charge >= 0)) {
    ldsim_set_error("pixel truth: min_abs_charge %g must be >= 0", min_abs_charge);
    return LDSIM_EINVAL;
  }
  CK(launch_need_record(ctx, "pixel truth"));
  HIPCHK(hipSetDevice(ctx->device));
  const ChainView v = chain_view(ctx);      // (the pass grows its own buffers and SB_SORTTMP only)
  const int64_t U = v.U;
  ctx->pt_gen = ctx->out_gen;
  ctx->pt_U = U;
  ctx->pt_n[0] = ctx->pt_n[1] = 0;
  ctx->pt_M = ctx->h_consts.max_tracks_per_pixel;
  if (U == 0) return 0;
  const ldsim_ctx::FeeRecord& R = ctx->fee_rec;
  ctx->pt_M = R.M;
  hipStream_t st = ctx->stream;
  CK(ctx->pt_dense.ensure(pt_dense_bytes(U, R.M)));
  CK(ctx->pt_sel.ensure((size_t)(4 * U + 4) * 4));
  const PtDense D = pt_dense_of(ctx->pt_dense.p, U, R.M);
  HIPCHK(hipMemsetAsync(ctx->pt_dense.p, 0, D.bytes, st));
  hipLaunchKernelGGL(pixel_truth_kernel, dim3((unsigned)((U + PT_WAVES - 1) / PT_WAVES)), dim3(64 * PT_WAVES), 0, st,
                     fee_rec_args(ctx, v), R.dt, D.q_induced, D.q_abs, D.q_track, D.n_slots);
  HIPCHK(hipGetLastError());
  // ---- selection: flags, exclusive scans of the flags and of the kept pixels' slot counts, then the gather ------------------
  int32_t* keep = ctx->pt_sel.as<int32_t>();
  int32_t *cnt = keep + U, *o_keep = cnt + U, *o_cnt = o_keep + U;
  const int32_t* d_hitcnt = v.hit_count;
  const unsigned g0 = (unsigned)((U + 255) / 256);
  hipLaunchKernelGGL(pixel_truth_flag_kernel, dim3(g0), dim3(256), 0, st, U, d_hitcnt, D.q_abs, D.n_slots, min_abs_charge, keep, cnt);
  HIPCHK(hipGetLastError());
  CK(sort_exclusive_scan_i32(ctx, keep, o_keep, U));
  CK(sort_exclusive_scan_i32(ctx, cnt, o_cnt, U));
  int32_t last[4];
  HIPCHK(hipMemcpyAsync(&last[0], keep + (U - 1), 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&last[1], o_keep + (U - 1), 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&last[2], cnt + (U - 1), 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&last[3], o_cnt + (U - 1), 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t n_pix = (int64_t)last[0] + last[1], n_trk = (int64_t)last[2] + last[3];
  if (n_pix < 0 || n_pix > U || n_trk < 0 || n_trk > R.n_pairs) {
    ldsim_set_error("pixel truth: the selection counted %lld pixels and %lld track entries of %lld pixels and %lld pairs",
                    (long long)n_pix, (long long)n_trk, (long long)U, (long long)R.n_pairs);
    return LDSIM_ESTATE;
  }
  const size_t b_rows = (size_t)n_pix * sizeof(LdsimPixelTruthRow);
  CK(ctx->pt_out.ensure(b_rows + (size_t)n_trk * sizeof(LdsimPixelTruthTrack)));
  if (n_pix) {
    hipLaunchKernelGGL(pixel_truth_gather_kernel, dim3(g0), dim3(256), 0, st, U, R.A, R.M, keep, o_keep, o_cnt,
                       v.upix, v.ubatch, d_hitcnt, v.adc, v.tpm, D.q_induced, D.q_abs, D.q_track,
                       D.n_slots, (LdsimPixelTruthRow*)ctx->pt_out.p, (LdsimPixelTruthTrack*)((char*)ctx->pt_out.p + b_rows));
    HIPCHK(hipGetLastError());
  }
  ctx->pt_n[0] = n_pix;
  ctx->pt_n[1] = n_trk;
  sizes[0] = n_pix;
  sizes[1] = n_trk;
  return 0;
}

extern "C" int ldsim_chain_pixel_truth_row_samples(ldsim_ctx* ctx, int64_t* n_samples) {
  LDSIM_ENTER(ctx);
  if (!ctx || !n_samples) { ldsim_set_error("null argument"); return LDSIM_EINVAL; }
  *n_samples = 0;
  CK(launch_need_record(ctx, "ldsim_chain_pixel_truth_row_samples"));
  const int64_t U = ctx->chain_U;
  if (U == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  CK(ctx->pt_sel.ensure((size_t)(4 * U + 4) * 4));
  unsigned long long* d_total = (unsigned long long*)(ctx->pt_sel.as<int32_t>() + 4 * U);      // (behind the scans; 16 U bytes in: 8-byte aligned)
  HIPCHK(hipMemsetAsync(d_total, 0, 8, ctx->stream));
  hipLaunchKernelGGL(pixel_truth_samples_kernel, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, ctx->stream,
                     fee_rec_args(ctx, chain_view(ctx)), d_total);
  HIPCHK(hipGetLastError());
  unsigned long long h = 0;
  HIPCHK(hipMemcpyAsync(&h, d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *n_samples = (int64_t)h;
  return 0;
}

static int pt_need_pass(ldsim_ctx* ctx) {
  if (ctx->pt_gen < 0 || ctx->pt_gen != ctx->out_gen) {
    ldsim_set_error("ldsim_chain_pixel_truth has not run for the last chain launch");
    return LDSIM_ESTATE;
  }
  return 0;
}

extern "C" int ldsim_chain_pixel_truth_download(ldsim_ctx* ctx, LdsimPixelTruthRow* pixel_rows, LdsimPixelTruthTrack* track_entries) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(pt_need_pass(ctx));
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t b_rows = (size_t)ctx->pt_n[0] * sizeof(LdsimPixelTruthRow), b_trk = (size_t)ctx->pt_n[1] * sizeof(LdsimPixelTruthTrack);
  if (pixel_rows && b_rows) HIPCHK(hipMemcpyAsync(pixel_rows, ctx->pt_out.p, b_rows, hipMemcpyDeviceToHost, st));
  if (track_entries && b_trk) HIPCHK(hipMemcpyAsync(track_entries, (const char*)ctx->pt_out.p + b_rows, b_trk, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int ldsim_chain_pixel_truth_dense_download(ldsim_ctx* ctx, int64_t U, double* q_induced, double* q_abs, double* q_track) {
  LDSIM_ENTER(ctx);
  if (!ctx) { ldsim_set_error("null ctx"); return LDSIM_EINVAL; }
  CK(pt_need_pass(ctx));
  if (U != ctx->pt_U) {
    ldsim_set_error("pixel truth: the last pass holds %lld rows, the caller's arrays %lld", (long long)ctx->pt_U, (long long)U);
    return LDSIM_EINVAL;
  }
  if (U == 0) return 0;
  if (ctx->pt_M != ctx->h_consts.max_tracks_per_pixel) {      // (the caller sizes q_track by the constants that hold now)
    ldsim_set_error("pixel truth: the last pass ran with MAX_TRACKS_PER_PIXEL %d, the constants now hold %d", ctx->pt_M,
                    ctx->h_consts.max_tracks_per_pixel);
    return LDSIM_ESTATE;
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const PtDense D = pt_dense_of(ctx->pt_dense.p, U, ctx->pt_M);
  if (q_induced) HIPCHK(hipMemcpyAsync(q_induced, D.q_induced, (size_t)U * 8, hipMemcpyDeviceToHost, st));
  if (q_abs) HIPCHK(hipMemcpyAsync(q_abs, D.q_abs, (size_t)U * 8, hipMemcpyDeviceToHost, st));
  if (q_track) HIPCHK(hipMemcpyAsync(q_track, D.q_track, (size_t)U * ctx->pt_M * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
