// comm.hip -- the one exchange step of the batch-sharded path, directly on RCCL over xGMI: one process per GPU,
// every rank simulates its own (event, TPC-group) batches with no data-path collective, then the compact hit rows
// {batch, pixel, adc, slot, tick} (24 B) are reassembled on every rank: an all-gather of the row counts followed by an
// all-gather-v of the rows (one ncclBroadcast per rank inside a group call: no padding to the largest shard).
// The communicator is bootstrapped from an ncclUniqueId the host side hands to every rank (larndsim_amd/comm.py).
#include <rccl/rccl.h>

#include "ldsim_args.h"

#define NCCLCHK(expr)                                                                                  \
  do {                                                                                                 \
    ncclResult_t r_ = (expr);                                                                          \
    if (r_ != ncclSuccess) {                                                                           \
      ldsim_set_error("%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__);     \
      return LDSIM_EHIP;                                                                               \
    }                                                                                                  \
  } while (0)

static_assert(sizeof(ncclUniqueId) == LDSIM_COMM_ID_BYTES, "LDSIM_COMM_ID_BYTES must be sizeof(ncclUniqueId)");

extern "C" int ldsim_comm_unique_id(void* id) {
  NEED(id, "null id");
  ncclUniqueId u;
  NCCLCHK(ncclGetUniqueId(&u));
  memcpy(id, &u, sizeof(u));
  return 0;
}

extern "C" int ldsim_comm_init(ldsim_ctx* ctx, const void* id, int32_t rank, int32_t world) {
  LDSIM_ENTER(ctx);
  NEED(ctx && id && world >= 1 && rank >= 0 && rank < world, "bad communicator arguments");
  NEED(!ctx->comm, "communicator already initialised");
  HIPCHK(hipSetDevice(ctx->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  ncclComm_t comm = nullptr;
  NCCLCHK(ncclCommInitRank(&comm, world, u, rank));
  ctx->comm = (void*)comm;
  ctx->comm_rank = rank;
  ctx->comm_world = world;
  return 0;
}

// ranks in the communicator as RCCL reports them (ncclCommCount / ncclCommUserRank): lets a caller check that every rank of the
// launch really joined, instead of trusting the environment it was started with
extern "C" int ldsim_comm_count(ldsim_ctx* ctx, int32_t* n_ranks, int32_t* rank) {
  LDSIM_ENTER(ctx);
  NEED(ctx && ctx->comm && n_ranks, "no communicator / null argument");
  int n = 0, r = 0;
  NCCLCHK(ncclCommCount((ncclComm_t)ctx->comm, &n));
  NCCLCHK(ncclCommUserRank((ncclComm_t)ctx->comm, &r));
  *n_ranks = n;
  if (rank) *rank = r;
  return 0;
}

extern "C" int ldsim_comm_destroy(ldsim_ctx* ctx) {
  LDSIM_ENTER(ctx);
  if (!ctx || !ctx->comm) return 0;
  (void)hipStreamSynchronize(ctx->stream);
  NCCLCHK(ncclCommDestroy((ncclComm_t)ctx->comm));
  ctx->comm = nullptr;
  ctx->comm_world = 0;
  ctx->cpt_all_root = ctx->cpt_all_src = ctx->gv_all_root = -1;
  return 0;
}

// value (host, in/out) reduced over the ranks: op 0 = sum, 1 = max.  Doubles as the barrier (every rank leaves after all entered).
extern "C" int ldsim_comm_allreduce_f64(ldsim_ctx* ctx, double* value, int32_t op) {
  LDSIM_ENTER(ctx);
  NEED(ctx && value && ctx->comm, "no communicator");
  HIPCHK(hipSetDevice(ctx->device));
  int rc = ctx->comm_tmp.ensure(64 + 8 * (size_t)ctx->comm_world);
  if (rc) return rc;
  double* d = (double*)ctx->comm_tmp.p;
  HIPCHK(hipMemcpyAsync(d, value, 8, hipMemcpyHostToDevice, ctx->stream));
  NCCLCHK(ncclAllReduce(d, d, 1, ncclDouble, op == 1 ? ncclMax : ncclSum, (ncclComm_t)ctx->comm, ctx->stream));
  HIPCHK(hipMemcpyAsync(value, d, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// Keep the compact hit rows of the chain calls of one pass: reset != 0 starts a new pass, then the last chain call's rows
// are appended (device-to-device, on the ctx stream, before the next chain call reuses its buffer).
extern "C" int ldsim_hits_accumulate(ldsim_ctx* ctx, int32_t reset) {
  LDSIM_ENTER(ctx);
  NEED(ctx, "null ctx");
  HIPCHK(hipSetDevice(ctx->device));
  if (reset) ctx->hits_acc_rows = 0;
  const int64_t n = ctx->chain_hits;
  if (n == 0) return 0;
  const size_t need = (size_t)(ctx->hits_acc_rows + n) * 24;
  CK(ctx->hits_acc.grow_keep(ctx->stream, (size_t)ctx->hits_acc_rows * 24, need));
  HIPCHK(hipMemcpyAsync((char*)ctx->hits_acc.p + (size_t)ctx->hits_acc_rows * 24, chain_view(ctx).hits, (size_t)n * 24,
                        hipMemcpyDeviceToDevice, ctx->stream));
  ctx->hits_acc_rows += n;
  return 0;
}

// All-gather-v of the accumulated rows.  counts[world] (host, may be NULL) receives every rank's row count; *gathered is a
// device pointer owned by the ctx (valid until the next call) holding the rows of rank 0, 1, .. back to back.
extern "C" int ldsim_comm_allgather_hits(ldsim_ctx* ctx, void** gathered, int64_t* total_rows, int64_t* counts) {
  LDSIM_ENTER(ctx);
  NEED(ctx && gathered && total_rows && ctx->comm, "no communicator / null argument");
  HIPCHK(hipSetDevice(ctx->device));
  const int W = ctx->comm_world;
  ncclComm_t comm = (ncclComm_t)ctx->comm;
  int rc = ctx->comm_tmp.ensure(64 + 8 * (size_t)W);
  if (rc) return rc;
  int64_t* d_mine = (int64_t*)ctx->comm_tmp.p;
  int64_t* d_all = (int64_t*)((char*)ctx->comm_tmp.p + 64);
  const int64_t mine = ctx->hits_acc_rows;
  HIPCHK(hipMemcpyAsync(d_mine, &mine, 8, hipMemcpyHostToDevice, ctx->stream));
  NCCLCHK(ncclAllGather(d_mine, d_all, 1, ncclInt64, comm, ctx->stream));
  std::vector<int64_t> h((size_t)W);
  HIPCHK(hipMemcpyAsync(h.data(), d_all, 8 * (size_t)W, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int64_t total = 0;
  for (int r = 0; r < W; r++) {
    NEED(h[r] >= 0, "negative row count received");
    total += h[r];
  }
  if ((rc = ctx->hits_all.ensure((size_t)(total > 0 ? total : 1) * 24))) return rc;
  NCCLCHK(ncclGroupStart());
  int64_t off = 0;
  for (int r = 0; r < W; r++) {
    if (h[r] > 0) {
      char* dst = (char*)ctx->hits_all.p + (size_t)off * 24;
      const void* src = (r == ctx->comm_rank) ? ctx->hits_acc.p : (const void*)dst;
      NCCLCHK(ncclBroadcast(src, dst, (size_t)h[r] * 24, ncclChar, r, comm, ctx->stream));
    }
    off += h[r];
  }
  NCCLCHK(ncclGroupEnd());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (counts) memcpy(counts, h.data(), 8 * (size_t)W);
  *gathered = ctx->hits_all.p;
  *total_rows = total;
  return 0;
}

// rows [0, n) of the gathered buffer to host (tests / the driver's output writer)
extern "C" int ldsim_comm_gathered_download(ldsim_ctx* ctx, void* rows, int64_t n) {
  LDSIM_ENTER(ctx);
  NEED(ctx && (rows || n == 0), "null argument");
  if (n == 0) return 0;
  NEED((size_t)n * 24 <= ctx->hits_all.bytes, "more rows requested than gathered");
  HIPCHK(hipMemcpy(rows, ctx->hits_all.p, (size_t)n * 24, hipMemcpyDeviceToHost));
  return 0;
}

// ---- the drop-in driver's exchange (cli/simulate_pixels.py --n_gpus): every rank's compact results to one writer ------------
// A rank keeps the five parts of ldsim_chain_compact_build of each of its launches in HBM, one growing buffer per part; at the
// end of a module root receives them, one source rank at a time.  Every part of a rank is one contiguous run, so a rank sends it in place with one ncclSend
// per part (no pack kernel).  Element bytes and, per part, which of cpt_n[] counts it:
//   0 hit-pixel rows [5] i32 (cpt_n[0]) | 1 track segments i64 (cpt_n[2]) | 2 hit rows 24 B (cpt_n[1]) | 3 charges f64 (cpt_n[1])
//   4 fractions f64 (cpt_n[3])
static const size_t CPT_ELEM[5] = {20, 8, 24, 8, 8};

extern "C" int ldsim_compact_accumulate(ldsim_ctx* ctx, int32_t reset) {
  LDSIM_ENTER(ctx);
  NEED(ctx, "null ctx");
  HIPCHK(hipSetDevice(ctx->device));
  if (reset) {                               // (empties the stream and appends nothing)
    for (int k = 0; k < 5; k++) ctx->cpt_acc_n[k] = 0;
    return 0;
  }
  if (ctx->cpt_gen != ctx->out_gen) {
    ldsim_set_error("ldsim_chain_compact_build has not run for the last chain launch");
    return LDSIM_ESTATE;
  }
  if (ctx->cpt_acc_gen == ctx->cpt_gen) {
    ldsim_set_error("the last chain launch's compact results are already in the stream");
    return LDSIM_ESTATE;
  }
  ctx->cpt_acc_gen = ctx->cpt_gen;
  const int64_t n_hp = ctx->cpt_n[0], n_hits = ctx->cpt_n[1], n_trk = ctx->cpt_n[2], n_frac = ctx->cpt_n[3];
  const size_t b_hp = ((size_t)n_hp * 20 + 7) & ~(size_t)7, b_trk = (size_t)n_trk * 8, b_chg = (size_t)n_hits * 8;
  const char* base = ctx->scratch[SB_CPO].as<const char>();
  const void* src[5] = {base, base + b_hp, chain_view(ctx).hits, base + b_hp + b_trk, base + b_hp + b_trk + b_chg};
  const int64_t cnt[5] = {n_hp, n_trk, n_hits, n_hits, n_frac};
  for (int k = 0; k < 5; k++) {
    if (cnt[k] == 0) continue;
    const size_t have = (size_t)ctx->cpt_acc_n[k] * CPT_ELEM[k], add = (size_t)cnt[k] * CPT_ELEM[k];
    CK(ctx->cpt_acc[k].grow_keep(ctx->stream, have, have + add));
    HIPCHK(hipMemcpyAsync((char*)ctx->cpt_acc[k].p + have, src[k], add, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->cpt_acc_n[k] += cnt[k];
  }
  return 0;
}

// One source rank per call: root never holds more than one rank's stream (its buffers are sized for that rank alone), and
// downloads and exports it before it receives the next.
extern "C" int ldsim_comm_gather_compact(ldsim_ctx* ctx, int32_t root, int32_t src_rank, int64_t* sizes) {
  LDSIM_ENTER(ctx);
  NEED(ctx && ctx->comm, "no communicator");
  const int W = ctx->comm_world, me = ctx->comm_rank;
  NEED(root >= 0 && root < W, "root out of range");
  NEED(src_rank >= 0 && src_rank < W, "source rank out of range");
  HIPCHK(hipSetDevice(ctx->device));
  ncclComm_t comm = (ncclComm_t)ctx->comm;
  hipStream_t st = ctx->stream;
  ctx->cpt_all_root = ctx->cpt_all_src = -1;
  int rc = ctx->comm_tmp.ensure(64 + 40 * (size_t)W);
  if (rc) return rc;
  int64_t* d_mine = (int64_t*)ctx->comm_tmp.p;
  int64_t* d_all = (int64_t*)((char*)ctx->comm_tmp.p + 64);
  HIPCHK(hipMemcpyAsync(d_mine, ctx->cpt_acc_n, 40, hipMemcpyHostToDevice, st));
  NCCLCHK(ncclAllGather(d_mine, d_all, 5, ncclInt64, comm, st));
  std::vector<int64_t> h((size_t)W * 5);
  HIPCHK(hipMemcpyAsync(h.data(), d_all, 40 * (size_t)W, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t i = 0; i < h.size(); i++) NEED(h[i] >= 0, "negative size received");
  for (int k = 0; k < 5; k++)
    if (h[(size_t)me * 5 + k] != ctx->cpt_acc_n[k]) {
      ldsim_set_error("gather_compact: the all-gathered size of part %d of rank %d (%lld) differs from the local one (%lld)", k,
                      me, (long long)h[(size_t)me * 5 + k], (long long)ctx->cpt_acc_n[k]);
      return LDSIM_EINVAL;
    }
  const int64_t* n = &h[(size_t)src_rank * 5];
  if (me == root)
    for (int k = 0; k < 5; k++)
      if ((rc = ctx->cpt_all[k].ensure((size_t)(n[k] > 0 ? n[k] : 1) * CPT_ELEM[k]))) return rc;
  if (src_rank == root) {
    if (me == root)                                    // root's own stream: a device-to-device copy
      for (int k = 0; k < 5; k++)
        if (n[k]) HIPCHK(hipMemcpyAsync(ctx->cpt_all[k].p, ctx->cpt_acc[k].p, (size_t)n[k] * CPT_ELEM[k], hipMemcpyDeviceToDevice, st));
  } else if (me == root || me == src_rank) {
    NCCLCHK(ncclGroupStart());
    for (int k = 0; k < 5; k++) {
      if (n[k] == 0) continue;
      const size_t bytes = (size_t)n[k] * CPT_ELEM[k];
      if (me == root) NCCLCHK(ncclRecv(ctx->cpt_all[k].p, bytes, ncclChar, src_rank, comm, st));
      else NCCLCHK(ncclSend(ctx->cpt_acc[k].p, bytes, ncclChar, root, comm, st));
    }
    NCCLCHK(ncclGroupEnd());
  }
  HIPCHK(hipStreamSynchronize(st));
  if (me == root) {
    for (int k = 0; k < 5; k++) ctx->cpt_all_n[k] = n[k];
    ctx->cpt_all_root = root;
    ctx->cpt_all_src = src_rank;
  }
  if (sizes) memcpy(sizes, h.data(), 40 * (size_t)W);
  return 0;
}

extern "C" int ldsim_comm_gathered_compact_download(ldsim_ctx* ctx, int32_t src_rank, int32_t* hit_pixels, int64_t* track_segments,
                                                    void* hit_rows, double* hit_charge, double* fractions) {
  LDSIM_ENTER(ctx);
  NEED(ctx && ctx->comm, "no communicator");
  NEED(src_rank >= 0 && src_rank < ctx->comm_world, "source rank out of range");
  if (ctx->cpt_all_root != ctx->comm_rank || ctx->cpt_all_src != src_rank) {
    ldsim_set_error("this rank holds no gathered compact results of rank %d (not the root of the last ldsim_comm_gather_compact "
                    "from that rank)", src_rank);
    return LDSIM_ESTATE;
  }
  HIPCHK(hipSetDevice(ctx->device));
  void* dst[5] = {hit_pixels, track_segments, hit_rows, hit_charge, fractions};
  for (int k = 0; k < 5; k++)
    if (dst[k] && ctx->cpt_all_n[k])
      HIPCHK(hipMemcpyAsync(dst[k], ctx->cpt_all[k].p, (size_t)ctx->cpt_all_n[k] * CPT_ELEM[k], hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int ldsim_comm_gatherv_bytes(ldsim_ctx* ctx, int32_t root, const void* host, int64_t n, int64_t* counts) {
  LDSIM_ENTER(ctx);
  NEED(ctx && ctx->comm, "no communicator");
  const int W = ctx->comm_world, me = ctx->comm_rank;
  NEED(root >= 0 && root < W, "root out of range");
  NEED(n >= 0 && (host || n == 0), "null host buffer / negative length");
  HIPCHK(hipSetDevice(ctx->device));
  ncclComm_t comm = (ncclComm_t)ctx->comm;
  hipStream_t st = ctx->stream;
  ctx->gv_all_root = -1;
  int rc = ctx->comm_tmp.ensure(64 + 8 * (size_t)W);
  if (rc) return rc;
  int64_t* d_mine = (int64_t*)ctx->comm_tmp.p;
  int64_t* d_all = (int64_t*)((char*)ctx->comm_tmp.p + 64);
  HIPCHK(hipMemcpyAsync(d_mine, &n, 8, hipMemcpyHostToDevice, st));
  NCCLCHK(ncclAllGather(d_mine, d_all, 1, ncclInt64, comm, st));
  std::vector<int64_t> h((size_t)W);
  HIPCHK(hipMemcpyAsync(h.data(), d_all, 8 * (size_t)W, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int64_t total = 0, mine_off = 0;
  for (int r = 0; r < W; r++) {
    NEED(h[r] >= 0, "negative length received");
    if (r < me) mine_off += h[r];
    total += h[r];
  }
  if (h[me] != n) {
    ldsim_set_error("gatherv_bytes: the all-gathered length of rank %d (%lld) differs from the local one (%lld)", me,
                    (long long)h[me], (long long)n);
    return LDSIM_EINVAL;
  }
  if (me == root) {
    if ((rc = ctx->gv_all.ensure((size_t)(total > 0 ? total : 1)))) return rc;
    if (n) HIPCHK(hipMemcpyAsync((char*)ctx->gv_all.p + mine_off, host, (size_t)n, hipMemcpyHostToDevice, st));
  } else if (n) {
    if ((rc = ctx->gv_send.ensure((size_t)n))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->gv_send.p, host, (size_t)n, hipMemcpyHostToDevice, st));
  }
  NCCLCHK(ncclGroupStart());
  int64_t off = 0;
  for (int r = 0; r < W; r++) {
    if (h[r] > 0 && r != root) {
      if (me == root) NCCLCHK(ncclRecv((char*)ctx->gv_all.p + off, (size_t)h[r], ncclChar, r, comm, st));
      else if (me == r) NCCLCHK(ncclSend(ctx->gv_send.p, (size_t)h[r], ncclChar, root, comm, st));
    }
    off += h[r];
  }
  NCCLCHK(ncclGroupEnd());
  HIPCHK(hipStreamSynchronize(st));
  ctx->gv_all_n = h;
  ctx->gv_all_root = root;
  if (counts) memcpy(counts, h.data(), 8 * (size_t)W);
  return 0;
}

extern "C" int ldsim_comm_gathered_bytes_download(ldsim_ctx* ctx, int32_t src_rank, void* out) {
  LDSIM_ENTER(ctx);
  NEED(ctx && ctx->comm, "no communicator");
  NEED(src_rank >= 0 && src_rank < ctx->comm_world, "source rank out of range");
  if (ctx->gv_all_root != ctx->comm_rank) {
    ldsim_set_error("this rank holds no gathered bytes (not the root of the last ldsim_comm_gatherv_bytes)");
    return LDSIM_ESTATE;
  }
  const int64_t n = ctx->gv_all_n[src_rank];
  NEED(out || n == 0, "null output buffer");
  if (n == 0) return 0;
  int64_t off = 0;
  for (int r = 0; r < src_rank; r++) off += ctx->gv_all_n[r];
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpy(out, (const char*)ctx->gv_all.p + off, (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}
