// chain.hip -- host orchestration of the device-resident charge chain (a5..a16) on the ctx stream.
// Mirrors the body of the reference's batch loop (cli/simulate_pixels.py:917-1105) for MANY batches at
// once: every (event, TPC-group, sub-batch) batch keeps its own unique-pixel set, max_length and
// segment numbering because the batch id is the leading key of the pair sort.
#include <stdio.h>
#include <math.h>

#include <vector>

#include "launchers.h"
#include <utility>

static void fill_cur_common(ldsim_ctx* ctx, CurArgs& a) {
  a.s = charge_store(ctx);   // (the anode view after a mapped quench_drift)
  a.c = ctx->d_consts.as<LdsimConsts>();
  a.resp = ctx->d_resp.as<double>();
  a.ni = ctx->ni; a.nj = ctx->nj; a.nk = ctx->nk;
  if (ctx->trim_response && ctx->resp_k_last >= ctx->resp_k_first) {
    a.k_first = ctx->resp_k_first;
    a.k_last = ctx->resp_k_last;
  } else {
    a.k_first = 0;
    a.k_last = ctx->nk - 1;
  }
  a.prune_log = ctx->prune_log;
  a.tail_log = ctx->tail_log;
  a.debug_phases = ctx->debug_phases;
  a.numba_f32 = ctx->numba_f32;
  a.split_max_items = ctx->split_max_items;
}

// a9-a12 for the pairs of `a` (sorted pair list of the chain, or the dense [S][P] grid of the stage call) by the configured
// kernels: tracks_current_mc, the split path (weights stage + correlation, overflowed pairs recomputed by the monolithic
// kernel) or the monolithic kernel for everything.  counters = ChainMisc::counters, zeroed by the caller.
// a.win set: *win_used tells whether the kernels that ran wrote the windows (else every row is complete and a.win is unset).
static int run_tracks_current(ldsim_ctx* ctx, CurArgs& a, int64_t n_seg, unsigned long long* counters, bool* split_timed,
                              bool* win_used = nullptr) {
  hipStream_t st = ctx->stream;
  const int64_t n_valid = a.n_pairs;
  *split_timed = false;
  size_t ib = 0, hb = 0, cb = 0;
  int32_t* win = a.win;
  a.win = nullptr;
  if (win_used) *win_used = false;
  ctx->gform_rec.valid = 0;            // (gform_launch sets it: every other path leaves no census)
  if (ctx->mc_current) return current_mc_launch(ctx, a, n_seg);   // the driver's call site (cli/simulate_pixels.py:1016)
  // The node-separable form pays per response tick of the staged support (nodes x cells x ticks on the matrix pipe), the
  // shifted-window kernels per 512-tick tile and (weight, tick) pair.  Until round 4 a table with full support (no exact zeros
  // over ~2000 ticks) was 20 % faster in the latter and "gform_max_support" = 768 ticks handed it over; with the 1e-7 node rule
  // (one batch of <= 16 nodes for most pairs) the matrix form is ahead there too -- module0 / 2x2 +18 %, ndlar +33 %
  // (profiles/r04_dense_handover.log) -- and the default no longer hands over.  weights_mode 1 / 0 force the shifted-window path,
  // a finite gform_max_support (ticks of TIME_SAMPLING) restores the hand-over.
  const int M_ratio = (int)llround(ctx->h_consts.time_sampling / ctx->h_consts.response_sampling);
  const int support_ticks = (a.k_last - a.k_first + 1) / (M_ratio > 0 ? M_ratio : 1);
  const bool use_gform = ctx->weights_mode == 2 && support_ticks <= ctx->gform_max_support;
  if (ctx->split_kernels && use_gform && n_valid > 0) {
    // node-separable form (gform.h): tables, then the correlation on the matrix pipe; no weight pool, no repeat launches
    int32_t* flags = nullptr;
    a.win = win;
    int rc = gform_launch(ctx, a, counters, &flags, &a.flag_list, &a.flag_count);
    a.win = nullptr;                       // (the monolithic kernel writes its rows in full)
    if (rc < 0) return rc;
    if (rc == 0) {
      *split_timed = true;
      if (win_used) *win_used = win != nullptr;
      a.only_flagged = flags - 7;          // current_kernel reads only_flagged[pair * flag_stride + 7]
      a.flag_stride = 1;
      return current_launch(ctx, a);
    }
    a.flag_list = nullptr;
    a.flag_count = nullptr;
  }
  if (!(ctx->split_kernels && n_valid > 0 && split_sizes(ctx, a, &ib, &hb, &cb) > 0)) return current_launch(ctx, a);
  CK(ctx->scratch[SB_ITEMS].ensure((size_t)n_valid * ib));
  CK(ctx->scratch[SB_HDR].ensure((size_t)n_valid * hb));
  CK(ctx->scratch[SB_CORR].ensure((size_t)n_valid * cb));
  // The weights go to one pool shared by all pairs of the launch (bump allocator, counters[ST_POOL_CURSOR] = doubles requested).
  // Which pairs lose when it runs dry depends on scheduling order, and a pair recomputed by the monolithic kernel
  // agrees only to rounding -- so a launch that exhausted the pool is never used: the pool is grown to the demand
  // (a lower bound then: an exhausted pair stops requesting) and weights_kernel runs again.  The size per pair is
  // remembered, so this happens on the first launches of a new detector configuration only.
  double per_pair = fmax((double)ctx->wbuf_doubles_per_pair, ctx->wbuf_learned);
  unsigned long long wcap = 0, demand = 0;
  bool fits = false;
  for (int attempt = 0; attempt < 6 && !fits; attempt++) {
    wcap = (unsigned long long)ceil(per_pair * (double)n_valid);
    CK(ctx->scratch[SB_WBUF].ensure((size_t)wcap * 8));
    if (attempt > 0) {
      HIPCHK(hipMemsetAsync(&counters[ST_POOL_CURSOR], 0, 8, st));
      HIPCHK(hipMemsetAsync(&counters[ST_N], 0, STAT_BYTES - 8 * ST_N, st));     // the kernels' stripes (nothing earlier adds to them)
    }
    int rc = split_launch_weights(ctx, a, ctx->scratch[SB_ITEMS].p, ctx->scratch[SB_HDR].p, ctx->scratch[SB_CORR].p,
                                  ctx->scratch[SB_WBUF].as<double>(), wcap, &counters[ST_POOL_CURSOR]);
    if (rc > 0) { ldsim_set_error("split path refused a configuration split_sizes accepted"); return LDSIM_ESTATE; }
    if (rc < 0) return rc;
    HIPCHK(hipMemcpyAsync(&demand, &counters[ST_POOL_CURSOR], 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    fits = demand <= wcap;
    if (!fits) per_pair = 1.5 * (double)(demand > wcap ? demand : wcap) / (double)n_valid;
  }
  ctx->wbuf_learned = fmax(ctx->wbuf_learned, 1.25 * (double)demand / (double)n_valid);
  HIPCHK(hipEventRecord(ctx->ev[5], st));
  int rc = split_launch_mac(ctx, a, ctx->scratch[SB_ITEMS].p, ctx->scratch[SB_HDR].p, ctx->scratch[SB_CORR].p,
                            ctx->scratch[SB_WBUF].as<double>(), wcap, &counters[ST_POOL_CURSOR]);
  if (rc > 0) { ldsim_set_error("split path refused a configuration split_sizes accepted"); return LDSIM_ESTATE; }
  if (rc < 0) return rc;
  HIPCHK(hipEventRecord(ctx->ev[6], st));
  *split_timed = true;
  // pairs beyond the per-pair item / correction / run capacities (and, after 6 attempts, a pool that still does not
  // fit): recomputed by the monolithic kernel
  a.only_flagged = ctx->scratch[SB_HDR].as<const int32_t>();
  a.flag_stride = (int32_t)(hb / 4);
  return current_launch(ctx, a);
}

static void stats_from_counters(LdsimChainStats& s, const unsigned long long* h_cnt) {
  s.n_ambiguous = (int32_t)h_cnt[ST_AMBIGUOUS];
  s.n_samples = (int64_t)h_cnt[ST_SAMPLES];
  s.n_dfma = (int64_t)h_cnt[ST_DFMA];
  s.n_fallback = (int64_t)h_cnt[ST_FALLBACK];
  s.n_wbuf = (int64_t)h_cnt[ST_POOL_CURSOR];
  s.n_dfma_useful = (int64_t)h_cnt[ST_DFMA_USEFUL];
}

// materialising tracks_current: dense [S][P] pixel array, signals [S][P][T].  Runs the kernels the options select, like the
// chain: the per-tick parity tests reach the default (split) kernels through this call; ldsim_tracks_current_stats tells
// which kernels carried the pairs.
int chain_tracks_current(ldsim_ctx* ctx, const int32_t* d_pixels, int P, float* d_signals, int T, int mc) {
  launch_invalidate(ctx, "a host-array tracks_current stage call reused the launch's buffers");
  CK(ctx->scratch[SB_MISC].ensure(MISC_BYTES));
  unsigned long long* counters = ctx->scratch[SB_MISC].as<ChainMisc>()->counters;
  HIPCHK(hipMemsetAsync(counters, 0, STAT_BYTES, ctx->stream));
  CurArgs a{};
  fill_cur_common(ctx, a);
  a.pair_val = nullptr; a.pair_key = nullptr;
  a.pixels = d_pixels;
  a.seg_begin = 0;
  a.P = P;
  a.n_pairs = ctx->seg.n * (int64_t)P;
  a.out = d_signals;
  a.T = T;
  a.tmax_batch = nullptr;
  a.batch0 = 0;
  a.counters = counters;
  a.only_flagged = nullptr;
  a.flag_stride = 0;
  ctx->stage_stats = LdsimChainStats{};
  ctx->stage_stats.n_segments = ctx->seg.n;
  ctx->stage_stats.n_pairs = a.n_pairs;
  ctx->stage_stats.max_neigh = P;
  ctx->stage_stats.max_length = T;
  if (mc) {
    ctx->gform_rec.valid = 0;
    return current_mc_launch(ctx, a, ctx->seg.n);
  }
  bool split_timed = false;
  const int keep_mc = ctx->mc_current;
  ctx->mc_current = 0;                 // the stage call names its kernel itself
  int rc = run_tracks_current(ctx, a, ctx->seg.n, counters, &split_timed);
  ctx->mc_current = keep_mc;
  if (rc) return rc;
  unsigned long long h_cnt[ST_N];
  CK(ctx->readback.ensure(sizeof(ChainReadback)));
  ChainReadback* rb = ctx->readback.as<ChainReadback>();
  HIPCHK(hipMemcpyAsync(rb->raw, counters, STAT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  stat_sum(rb->raw, h_cnt);
  stats_from_counters(ctx->stage_stats, h_cnt);
  return 0;
}

int chain_run(ldsim_ctx* ctx, int64_t seg_begin, int64_t seg_end, int want_fractions) {
  const LdsimConsts& h = ctx->h_consts;
  const int64_t n = seg_end - seg_begin;
  // results of the launch before this one may still be on their way to the host (ldsim_chain_download_async): this launch
  // writes the other set of output buffers; a copy that reads the set about to be written (two launches old) is waited for
  ctx->out_gen++;
  if (ctx->async_out) {
    if (ctx->copy_pending && ctx->pending_gen <= ctx->out_gen - 2) {
      HIPCHK(hipStreamSynchronize(ctx->copy_stream));
      ctx->copy_pending = 0;
    }
    static const int out_slots[7] = {SB_UPIX, SB_UBATCH, SB_ADC, SB_TICKS, SB_DIGIT, SB_TPM, SB_FRAC};
    for (int k = 0; k < 7; k++) std::swap(ctx->scratch[out_slots[k]], ctx->out_alt[k]);
  }
  ctx->stats = LdsimChainStats{};
  ctx->stats.n_segments = n;
  ctx->chain_U = 0;
  ctx->chain_hits = 0;
  ctx->want_fractions = want_fractions;
  ctx->ms_current = ctx->ms_adc = ctx->ms_total = 0;
  // per-pixel threshold / gain tables are dense over one pixel geometry: refuse another one before any work is launched
  const bool tables_fit = ctx->pix_table_n == (int64_t)h.n_pixels[0] * h.n_pixels[1] * h.n_tpc;
  if (!tables_fit && (ctx->d_pix_thr.p || ctx->d_pix_gain.p)) {
    ldsim_set_error("pixel threshold/gain tables were set for another pixel geometry: set them again after set_consts");
    return LDSIM_ESTATE;
  }
  if (n == 0) return 0;
  const int A = h.max_adc_values, M = h.max_tracks_per_pixel;
  hipStream_t st = ctx->stream;
  HIPCHK(hipEventRecord(ctx->ev[0], st));

  // batch id range of this call: the non-negative ids are non-decreasing (checked at upload against the host copy kept
  // in the ctx), so the first and the last one are the range; negative = not simulated
  int32_t b_first = 0, b_last = 0;
  {
    if ((int64_t)ctx->h_batch.size() < seg_end) {
      ldsim_set_error("resident batch ids missing: ldsim_segments_upload first");
      return LDSIM_ESTATE;
    }
    const int32_t* hb = ctx->h_batch.data() + seg_begin;
    int64_t i0 = 0, i1 = n - 1;
    while (i0 < n && hb[i0] < 0) i0++;
    if (i0 == n) return 0;
    while (hb[i1] < 0) i1--;
    b_first = hb[i0];
    b_last = hb[i1];
    if (b_last < b_first) {
      ldsim_set_error("batch ids of the resident segments are not non-decreasing");
      return LDSIM_EINVAL;
    }
  }
  if (ctx->rng_keyed && (int64_t)b_last >= ctx->rng_batch_keys_n) {
    ldsim_set_error("keyed random mode: no key for batch id %d (ldsim_chain_set_batch_keys holds %lld): set the batch keys "
                    "after every upload", b_last, (long long)ctx->rng_batch_keys_n);
    return LDSIM_ESTATE;
  }
  const int32_t batch0 = b_first;
  const int64_t n_batches = (int64_t)b_last - b_first + 1;
  ctx->stats.n_batches = n_batches;
  if (n_batches >= (1 << 27)) {
    ldsim_set_error("too many batches in one chain call");
    return LDSIM_EINVAL;
  }

  // ---- misc block (ChainMisc) and, behind it, the per-batch block: one memset clears both ------------------------------------
  CK(ctx->scratch[SB_MISC].ensure(MISC_BYTES + batch_block_bytes(n_batches)));
  ChainMisc* misc = ctx->scratch[SB_MISC].as<ChainMisc>();
  unsigned long long* counters = misc->counters;
  const BatchBlock bb = batch_block((char*)misc + MISC_BYTES, n_batches);
  int32_t *d_tmax_b = bb.tmax, *d_first_b = bb.first, *d_radius_b = bb.radius;
  unsigned long long* d_tran_b = bb.tran;
  HIPCHK(hipMemsetAsync(misc, 0, MISC_BYTES + batch_block_bytes(n_batches), st));
  // the words the launch reads back between its stages land in page-locked memory of the context (nothing is in flight here:
  // every launch ends with a synchronisation)
  CK(ctx->readback.ensure(chain_readback_bytes(n_batches)));
  ChainReadback* rb = ctx->readback.as<ChainReadback>();
  const ChainReadbackBatch rbb = chain_readback_batch(rb, n_batches);

  // ---- the segment front in one pass: a8 time_intervals per batch, the batches' first segments, a5 max_pixels
  // (cli/simulate_pixels.py:918-928) and the per-batch max tran_diff that sets max_radius ------------------------------------------
  CK(ctx->scratch[SB_STARTS].ensure((size_t)n * 8));
  double* d_starts = ctx->scratch[SB_STARTS].as<double>();
  CK(seg_launch_front(ctx, seg_begin, seg_end, batch0, d_starts, &misc->nmax, d_tmax_b, d_first_b, d_tran_b));
  // read-back 1: nmax and the batches' tran_diff size P, and with it every buffer of the pixel stages
  HIPCHK(hipMemcpyAsync(&rb->nmax, &misc->nmax, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(rbb.tran, d_tran_b, n_batches * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int32_t nmax = rb->nmax;
  int radius = 0;
  for (int64_t b = 0; b < n_batches; b++) {
    double mt;
    memcpy(&mt, &rbb.tran[b], 8);
    rbb.radius[b] = (int32_t)ceil(mt * 5 / h.pixel_pitch);      // max_radius of the batch
    radius = rbb.radius[b] > radius ? rbb.radius[b] : radius;
  }
  HIPCHK(hipMemcpyAsync(d_radius_b, rbb.radius, n_batches * 4, hipMemcpyHostToDevice, st));
  const int P = (2 * radius + 1) * nmax + (1 + 2 * radius) * radius * 2;
  ctx->stats.max_active = nmax;
  ctx->stats.max_neigh = P;
  if (nmax == 0 || P == 0) return 0;

  // ---- a6 get_pixels (the kernel writes every slot of its rows, the empty ones as -1) ------------------------------------------------
  const int64_t n_entries = n * P;
  if (n_entries >= 0x7fffffffLL) {
    ldsim_set_error("chain call too large: %lld (segment, pixel) slots; split the segment range", (long long)n_entries);
    return LDSIM_EINVAL;
  }
  CK(ctx->scratch[SB_ACTIVE].ensure((size_t)n * nmax * 4));
  CK(ctx->scratch[SB_NEIGH].ensure((size_t)n_entries * 4));
  CK(ctx->scratch[SB_NRAD].ensure((size_t)n_entries * 4));
  int32_t* d_neigh = ctx->scratch[SB_NEIGH].as<int32_t>();
  int32_t* d_nrad = ctx->scratch[SB_NRAD].as<int32_t>();
  CK(seg_launch_get_pixels(ctx, seg_begin, seg_end, radius, ctx->scratch[SB_ACTIVE].as<int32_t>(), nmax, d_neigh, d_nrad,
                           P, nullptr, d_radius_b, batch0));

  // ---- a7 unique pixels: stable radix sort of (batch, pixel, ring code) --------------------------------------------------------
  // The empty slots (three quarters of the entries of the module0 bench) never become keys: one stable selection forms the key of
  // every entry where it reads it and keeps the valid (key, entry index) pairs -- equal keys keep the order of their entries -- and
  // the count comes back with the per-batch tick counts, before the sort instead of after it.
  CK(ctx->scratch[SB_KEYS].ensure((size_t)n_entries * 8));
  CK(ctx->scratch[SB_KEYS2].ensure((size_t)n_entries * 8));
  CK(ctx->scratch[SB_VALS].ensure((size_t)n_entries * 4));
  CK(ctx->scratch[SB_VALS2].ensure((size_t)n_entries * 4));
  unsigned long long* d_keys = ctx->scratch[SB_KEYS].as<unsigned long long>();
  unsigned long long* d_keys2 = ctx->scratch[SB_KEYS2].as<unsigned long long>();
  int32_t* d_vals = ctx->scratch[SB_VALS].as<int32_t>();
  int32_t* d_vals2 = ctx->scratch[SB_VALS2].as<int32_t>();
  CK(sort_select_pairs(ctx, d_neigh, d_nrad, seg_begin, batch0, P, n_entries, d_keys, d_vals, &counters[ST_VALID_PAIRS]));
  // read-back 2: the valid pairs size the sort and everything per pair; the tick counts size the current rows
  HIPCHK(hipMemcpyAsync(&rb->n_valid, &counters[ST_VALID_PAIRS], 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(rbb.tmax, d_tmax_b, n_batches * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t n_valid = (int64_t)rb->n_valid;
  {
    // key = batch << 36 | pixel << 4 | ring code.  The sort looks at the bits that can differ only (sort_key_ranges): up to the top of
    // the largest pixel id these constants allow, and the launch's batch bits (module0, 20 batches: 24 + 5 bits, four 8-bit passes
    // where [0, 41) takes six)
    int kr[3];
    sort_key_ranges((unsigned long long)h.n_pixels[0] * h.n_pixels[1] * h.n_tpc - 1, n_batches, kr);
    CK(sort_pairs_bits(ctx, d_keys, d_keys2, d_vals, d_vals2, n_valid, 0, kr[0]));
    if (kr[2] > kr[1]) {
      CK(sort_pairs_bits(ctx, d_keys2, d_keys, d_vals2, d_vals, n_valid, kr[1], kr[2]));
      std::swap(d_keys, d_keys2);
      std::swap(d_vals, d_vals2);
    }
    // (d_keys2 / d_vals2: the sorted list, as below)
  }
  ctx->stats.n_pairs = n_valid;
  int32_t T = 0;
  for (int64_t b = 0; b < n_batches; b++) T = rbb.tmax[b] > T ? rbb.tmax[b] : T;
  ctx->stats.max_length = T;
  if (n_valid == 0 || T == 0) return 0;

  // a pair's unique-pixel index: the exclusive scan of the head flags.  The last index and the last flag give the number of unique
  // pixels U; nothing in the current stage needs it (CurArgs carries no per-pixel array), so their copies are only queued here and
  // read behind the synchronisation the current stage makes anyway (read-back 3, below)
  CK(ctx->scratch[SB_HEADS].ensure((size_t)n_valid * 4 + 16));
  CK(ctx->scratch[SB_UIDX].ensure((size_t)n_valid * 4 + 16));
  int32_t* d_heads = ctx->scratch[SB_HEADS].as<int32_t>();
  int32_t* d_uidx = ctx->scratch[SB_UIDX].as<int32_t>();
  CK(sort_heads(ctx, d_keys2, n_valid, d_heads));
  CK(sort_exclusive_scan_i32(ctx, d_heads, d_uidx, n_valid));
  HIPCHK(hipMemcpyAsync(&rb->last_idx, d_uidx + (n_valid - 1), 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&rb->last_head, d_heads + (n_valid - 1), 4, hipMemcpyDeviceToHost, st));

  // ---- a9-a12 induced current per sorted pair -------------------------------------------------------------------------------------
  CK(ctx->scratch[SB_WAVES].ensure((size_t)n_valid * T * 4));
  float* d_waves = ctx->scratch[SB_WAVES].as<float>();
  CurArgs a{};
  fill_cur_common(ctx, a);
  a.pair_val = d_vals2;
  a.pair_key = d_keys2;
  a.pixels = nullptr;
  a.seg_begin = seg_begin;
  a.P = P;
  a.n_pairs = n_valid;
  a.out = d_waves;
  a.T = T;
  a.tmax_batch = d_tmax_b;
  a.batch0 = batch0;
  a.batch_first = d_first_b;
  a.counters = counters;
  a.only_flagged = nullptr;
  a.flag_stride = 0;
  CK(ctx->scratch[SB_WIN].ensure((size_t)n_valid * 8 + 8));
  a.win = ctx->scratch[SB_WIN].as<int32_t>();
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  bool split_timed = false, win_used = false;
  CK(run_tracks_current(ctx, a, n, counters, &split_timed, &win_used));
  HIPCHK(hipEventRecord(ctx->ev[2], st));

  // ---- the unique pixels (read-back 3: U, queued before the current stage) ---------------------------------------------------------------
  // gform_launch has synchronised behind that copy for its pool size; every other current path gets a synchronisation here
  if (!ctx->gform_rec.valid) HIPCHK(hipStreamSynchronize(st));
  const int64_t U = (int64_t)rb->last_idx + rb->last_head;
  ctx->stats.n_unique = U;
  ctx->chain_U = U;
  CK(ctx->scratch[SB_UPIX].ensure((size_t)U * 4));
  CK(ctx->scratch[SB_UBATCH].ensure((size_t)U * 4));
  CK(ctx->scratch[SB_PIXOFF].ensure((size_t)(U + 1) * 8));
  int32_t* d_upix = ctx->scratch[SB_UPIX].as<int32_t>();
  int32_t* d_ubatch = ctx->scratch[SB_UBATCH].as<int32_t>();
  int64_t* d_uoff = ctx->scratch[SB_PIXOFF].as<int64_t>();
  CK(sort_fill_unique(ctx, d_keys2, d_heads, d_uidx, n_valid, batch0, d_upix, d_ubatch, d_uoff, U));

  // ---- a13-a16 per-pixel sum, trigger scan, digitise ---------------------------------------------------------------------------------
  CK(ctx->scratch[SB_ADC].ensure((size_t)U * A * 8));
  CK(ctx->scratch[SB_TICKS].ensure((size_t)U * A * 8));
  CK(ctx->scratch[SB_DIGIT].ensure((size_t)U * A * 8));
  CK(ctx->scratch[SB_TPM].ensure((size_t)U * M * 8));
  CK(ctx->scratch[SB_HITCNT].ensure(hit_counts_bytes(U)));
  if (want_fractions) CK(ctx->scratch[SB_FRAC].ensure((size_t)U * A * M * 8));
  const HitCounts hc = hit_counts(ctx->scratch[SB_HITCNT].p, U);
  int32_t *d_hitcnt = hc.count, *d_hitoff = hc.off;
  FeeArgs F{};
  F.c = ctx->d_consts.as<LdsimConsts>();
  F.k = FEEK_FROM(h);
  F.U = U;
  F.upix = d_upix; F.ubatch = d_ubatch; F.uoff = d_uoff;
  F.pair_val = d_vals2; F.pair_key = d_keys2;
  F.n_pairs = n_valid;
  F.P = P;
  F.track_starts = d_starts;
  F.waves = d_waves;
  F.win = win_used ? ctx->scratch[SB_WIN].as<const int32_t>() : nullptr;
  F.T = T;
  F.batch_first = d_first_b;
  F.batch0 = batch0;
  F.threshold = h.discrimination_threshold * 1.0;   // DISCRIMINATION_THRESHOLD * units.e
  F.thr_table = tables_fit ? ctx->d_pix_thr.as<double>() : nullptr;
  F.gain_table = tables_fit ? ctx->d_pix_gain.as<double>() : nullptr;
  F.time_padding = 0.0;                             // cli/simulate_pixels.py:1092
  F.adc_list = ctx->scratch[SB_ADC].as<double>();
  F.adc_ticks = ctx->scratch[SB_TICKS].as<double>();
  F.adc_digit = ctx->scratch[SB_DIGIT].as<double>();
  F.tpm = ctx->scratch[SB_TPM].as<int64_t>();
  F.fractions = want_fractions ? ctx->scratch[SB_FRAC].as<double>() : nullptr;
  F.counters = counters;
  F.hit_count = d_hitcnt;
  F.debug = ctx->debug_phases;
  // FEE noise (fee.py:557,583-584,616-617,621,649): row u of this launch draws from state u of the numba-style table, or
  // (keyed mode) from the stream of its (batch, pixel) identity, inline in the scan: no draws table, no advance pass
  const bool noisy = h.reset_noise_charge != 0 || h.uncorrelated_noise_charge != 0 || h.discriminator_noise != 0;
  const bool keyed_inline = noisy && ctx->rng_keyed && !ctx->debug_rng_materialize;
  if (keyed_inline) {
    F.batch_keys = (const uint64_t*)ctx->d_batch_keys.p;
    F.rng_seed = ctx->rng_seed;
  } else if (noisy && ctx->rng_keyed) {
    // debug_rng_materialize: the keyed normals written into the table layout and read by the table scan (tests)
    const int nd = rng_fee_draws_per_pixel(h, h.n_time_ticks);
    CK(ctx->scratch[SB_NOISE].ensure((size_t)U * nd * 4));
    CK(ctx->scratch[SB_NDRAWS].ensure((size_t)U * 4 + 4));
    CK(rng_launch_fee_keyed_fill(ctx, d_ubatch, d_upix, U, nd, ctx->scratch[SB_NOISE].as<float>()));
    F.noise_z = ctx->scratch[SB_NOISE].as<const float>();
    F.noise_nd = nd;
    F.n_draws = ctx->scratch[SB_NDRAWS].as<int32_t>();
  } else if (noisy) {
    CK(rng_ensure_states(ctx, U));
    const int nd = rng_fee_draws_per_pixel(h, h.n_time_ticks);
    CK(ctx->scratch[SB_NOISE].ensure((size_t)U * nd * 4));
    CK(ctx->scratch[SB_NDRAWS].ensure((size_t)U * 4 + 4));
    CK(rng_launch_fee_noise(ctx, U, nd, ctx->scratch[SB_NOISE].as<float>()));
    F.noise_z = ctx->scratch[SB_NOISE].as<const float>();
    F.noise_nd = nd;
    F.n_draws = ctx->scratch[SB_NDRAWS].as<int32_t>();
  }
  CK(fee_launch_chain(ctx, F));
  if (noisy && !ctx->rng_keyed) CK(rng_launch_advance(ctx, U, F.n_draws));
  HIPCHK(hipEventRecord(ctx->ev[3], st));

  // ---- compact hit rows (payload of the multi-GPU all-gather) -----------------------------------------------------------------------------
  // (the rows are sized by their bound, U x MAX_ADC_VALUES -- 140 MB per 100 k segments -- so that the hit count comes back with
  // the launch's last synchronisation instead of one of its own)
  CK(sort_exclusive_scan_i32(ctx, d_hitcnt, d_hitoff, U));
  CK(ctx->scratch[SB_HITS].ensure((size_t)U * A * 24 + 24));
  CK(sort_compact_hits(ctx, d_upix, d_ubatch, d_hitcnt, d_hitoff, F.adc_digit, F.adc_ticks, A, U,
                       ctx->scratch[SB_HITS].as<int32_t>()));
  // read-back 4: the launch counters, with the launch's last synchronisation
  unsigned long long h_cnt[ST_N];
  HIPCHK(hipMemcpyAsync(rb->raw, counters, STAT_BYTES, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(ctx->ev[4], st));
  HIPCHK(hipStreamSynchronize(st));
  stat_sum(rb->raw, h_cnt);
  if (ctx->debug_gform & 128)       // timing tools: cycle stamps of gcorr_kernel's waves (kernels_gcorr.hip)
    fprintf(stderr, "gcorr stamps (shader cycles, summed over waves): info %llu stage %llu G %llu P %llu edges %llu tail %llu life %llu\n",
            h_cnt[ST_GCORR_INFO], h_cnt[ST_GCORR_STAGE], h_cnt[ST_GCORR_G], h_cnt[ST_GCORR_P], h_cnt[ST_GCORR_EDGES],
            h_cnt[ST_GCORR_TAIL], h_cnt[ST_GCORR_LIFE]);
  if (ctx->debug_gform & 2048)      // the same stripes, written by gtables_wave_kernel's waves instead (kernels_gtables.hip)
    fprintf(stderr, "gtables stamps (shader cycles, summed over waves): loads %llu maps %llu batch_prologue %llu tables_xy %llu tables_z %llu cells %llu life %llu\n",
            h_cnt[ST_GTAB_LOADS], h_cnt[ST_GTAB_MAPS], h_cnt[ST_GTAB_BATCH_PROLOGUE], h_cnt[ST_GTAB_TABLES_XY],
            h_cnt[ST_GTAB_TABLES_Z], h_cnt[ST_GTAB_CELLS], h_cnt[ST_GTAB_LIFE]);
  ctx->stats.n_overflow = (int64_t)h_cnt[ST_OVERFLOW_PIXELS];
  ctx->chain_hits = (int64_t)h_cnt[ST_HITS];
  stats_from_counters(ctx->stats, h_cnt);
  ctx->n_fallback = (int64_t)h_cnt[ST_FALLBACK];
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2])); ctx->ms_current = ms;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3])); ctx->ms_adc = ms;
  ctx->ms_weights = ctx->ms_mac = 0;
  ctx->ms_fallback = ctx->ms_current;
  if (split_timed) {
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[5])); ctx->ms_weights = ms;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[6])); ctx->ms_mac = ms;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[2])); ctx->ms_fallback = ms;
  }
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[4])); ctx->ms_total = ms;
  return 0;
}
