// sort.hip -- device-wide sort / scan steps of the chain (rocPRIM), and the small glue kernels around them.
// a7 (cli/simulate_pixels.py:952-957,1019-1026): unique pixel set + index map, here as a stable radix sort
// of (batch, pixel, ring-code) keys whose value is the pair's position in segment order.
#include <string.h>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "launchers.h"
#include "gform.h"

// key = batch(24) | pixel(32) | ringcode(4, 15 = invalid); an empty slot (no pixel, or a segment that is not simulated) has no key
// (n_entries < 2^31, checked by the chain: 32-bit index arithmetic).  The keys are formed where the selection reads its input
// (sort_select_pairs below): the entries are never written as a list of their own.
namespace {
typedef rocprim::tuple<unsigned long long, int32_t> KeyedEntry;      // (key, entry index r * P + slot)
struct EntryKey {
  const int32_t *neigh, *nrad, *batch;      // batch: of the launch's first segment on
  int32_t batch0;
  unsigned P;
  __device__ KeyedEntry operator()(unsigned i) const {
    const int32_t pix = neigh[i];
    const int32_t b = batch[i / P];
    unsigned long long key = ~0ull;
    if (pix >= 0 && b >= 0) {
      const int32_t d = nrad[i];
      const unsigned long long dn = (d < 0 || d > 14) ? 15ull : (unsigned long long)d;
      key = ((unsigned long long)(uint32_t)(b - batch0) << 36) | ((unsigned long long)(uint32_t)pix << 4) | dn;
    }
    return KeyedEntry(key, (int32_t)i);
  }
};
struct EntryValid {
  __device__ bool operator()(const KeyedEntry& e) const { return rocprim::get<0>(e) != ~0ull; }
};
}  // namespace

__global__ void heads_kernel(const unsigned long long* __restrict__ keys, int64_t n_valid, int32_t* __restrict__ heads) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_valid) return;
  heads[i] = (i == 0 || (keys[i] >> 4) != (keys[i - 1] >> 4)) ? 1 : 0;
}

__global__ void fill_unique_kernel(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ heads,
                                   const int32_t* __restrict__ uidx, int64_t n_valid, int32_t batch0,
                                   int32_t* __restrict__ upix, int32_t* __restrict__ ubatch, int64_t* __restrict__ uoff,
                                   int64_t U) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) uoff[U] = n_valid;
  if (i >= n_valid || !heads[i]) return;
  int32_t u = uidx[i];
  upix[u] = (int32_t)((keys[i] >> 4) & 0xFFFFFFFFull);
  ubatch[u] = (int32_t)(keys[i] >> 36) + batch0;
  uoff[u] = i;
}

// first relative segment index of every batch in [seg_begin, seg_end)
__global__ void batch_first_kernel(const int32_t* __restrict__ batch, int64_t seg_begin, int64_t n, int32_t batch0,
                                   int32_t* __restrict__ first) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int32_t b = batch[seg_begin + r];
  if (b < 0) return;
  if (r == 0 || batch[seg_begin + r - 1] != b) first[b - batch0] = (int32_t)r;
}

// compact hit rows for the multi-GPU all-gather: {batch i32, pixel i32, adc i32, tick f64-bits hi/lo}
__global__ void compact_hits_kernel(const int32_t* __restrict__ upix, const int32_t* __restrict__ ubatch,
                                    const int32_t* __restrict__ hit_count, const int32_t* __restrict__ hit_off,
                                    const double* __restrict__ digit, const double* __restrict__ ticks, int A, int64_t U,
                                    int32_t* __restrict__ rows) {
  int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  int n = hit_count[u];
  int64_t o = hit_off[u];
  for (int h = 0; h < n; h++) {
    int32_t* r = rows + (o + h) * 6;
    r[0] = ubatch[u];
    r[1] = upix[u];
    r[2] = (int32_t)digit[u * A + h];
    r[3] = h;
    double t = ticks[u * A + h];
    *(double*)(r + 4) = t;
  }
}

static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

int sort_pairs(ldsim_ctx* ctx, unsigned long long* keys_in, unsigned long long* keys_out, int32_t* vals_in,
               int32_t* vals_out, int64_t n) {
  if (n == 0) return 0;
  size_t tmp = 0;
  HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, 64, ctx->stream));
  int rc = ctx->scratch[SB_SORTTMP].ensure(tmp);
  if (rc) return rc;
  HIPCHK(rocprim::radix_sort_pairs(ctx->scratch[SB_SORTTMP].p, tmp, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0,
                                   64, ctx->stream));
  return 0;
}

// The valid (segment, neighbour slot) entries of get_pixels' arrays in their order of appearance: their keys -> keys_out, their indices ->
// vals_out, their number -> *d_count (a device word, overwritten).  One stable rocPRIM select over (key, index) pairs made by a transform
// iterator: the pair-list sort then runs over the valid entries only (a quarter of the entries of the module0 bench) and equal keys keep
// the entry order they had among all entries.
int sort_select_pairs(ldsim_ctx* ctx, const int32_t* neigh, const int32_t* nrad, int64_t seg_begin, int32_t batch0, int P,
                      int64_t n_entries, unsigned long long* keys_out, int32_t* vals_out, unsigned long long* d_count) {
  if (n_entries == 0) return 0;
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned>(0),
                                             EntryKey{neigh, nrad, ctx->seg.batch + seg_begin, batch0, (unsigned)P});
  auto out = rocprim::make_zip_iterator(rocprim::make_tuple(keys_out, vals_out));
  size_t tmp = 0;
  HIPCHK(rocprim::select(nullptr, tmp, in, out, d_count, (size_t)n_entries, EntryValid(), ctx->stream));
  int rc = ctx->scratch[SB_SORTTMP].ensure(tmp);
  if (rc) return rc;
  HIPCHK(rocprim::select(ctx->scratch[SB_SORTTMP].p, tmp, in, out, d_count, (size_t)n_entries, EntryValid(), ctx->stream));
  return 0;
}

// The bit ranges the pair-list sort has to look at.  key = batch << 36 | pixel << 4 | ring code, and the pixel field cannot use its 32
// bits: the largest id is n_pixels[0] * n_pixels[1] * n_tpc - 1 (pixel_max).  The bits between the top of that id and bit 36 are zero
// in every key, so two stable passes of the LSD sort -- [0, r[0]) and then [r[1], r[2]) -- leave the order, equal keys included, that
// one pass over [0, 36 + bb) leaves.  The two ranges are chosen only where they save a pass of SORT_RADIX_BITS bits; else
// r = {36 + bb, 0, 0}, the single range.  (One batch: bb = 0 and no second range at all.)
#define SORT_RADIX_BITS 8      // (rocPRIM's digit for 64-bit keys with 32-bit values: a pass per 8 bits, read off the trace)
void sort_key_ranges(unsigned long long pixel_max, int64_t n_batches, int r[3]) {
  int bb = 0, pb = 0;
  while ((1ll << bb) < n_batches) bb++;
  while (pb < 32 && (pixel_max >> pb) != 0) pb++;
  const int single = 36 + bb, lo = 4 + pb;
  auto passes = [](int bits) { return (bits + SORT_RADIX_BITS - 1) / SORT_RADIX_BITS; };
  r[0] = single;
  r[1] = r[2] = 0;
  if (passes(lo) + passes(bb) < passes(single)) {
    r[0] = lo;
    if (bb > 0) {
      r[1] = 36;
      r[2] = 36 + bb;
    }
  }
}

// sort_pairs over the key bits [begin_bit, end_bit) only (a pass per 8 bits)
int sort_pairs_bits(ldsim_ctx* ctx, unsigned long long* keys_in, unsigned long long* keys_out, int32_t* vals_in, int32_t* vals_out,
                    int64_t n, int begin_bit, int end_bit) {
  if (n == 0) return 0;
  if (end_bit > 64) end_bit = 64;
  size_t tmp = 0;
  HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp, keys_in, keys_out, vals_in, vals_out, (size_t)n, begin_bit, end_bit, ctx->stream));
  int rc = ctx->scratch[SB_SORTTMP].ensure(tmp);
  if (rc) return rc;
  HIPCHK(rocprim::radix_sort_pairs(ctx->scratch[SB_SORTTMP].p, tmp, keys_in, keys_out, vals_in, vals_out, (size_t)n, begin_bit,
                                   end_bit, ctx->stream));
  return 0;
}

// stable sort of 32-bit keys (their low `bits` bits) with 64-bit payloads: the photon-sum records (kernels_light.hip)
int sort_pairs_u32_u64(ldsim_ctx* ctx, unsigned* keys_in, unsigned* keys_out, unsigned long long* vals_in, unsigned long long* vals_out,
                       int64_t n, int bits) {
  if (n == 0) return 0;
  if (bits > 32) bits = 32;
  size_t tmp = 0;
  HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, bits, ctx->stream));
  int rc = ctx->scratch[SB_SORTTMP].ensure(tmp);
  if (rc) return rc;
  HIPCHK(rocprim::radix_sort_pairs(ctx->scratch[SB_SORTTMP].p, tmp, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, bits,
                                   ctx->stream));
  return 0;
}

int sort_exclusive_scan_i32(ldsim_ctx* ctx, const int32_t* in, int32_t* out, int64_t n) {
  if (n == 0) return 0;
  size_t tmp = 0;
  HIPCHK(rocprim::exclusive_scan(nullptr, tmp, in, out, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), ctx->stream));
  int rc = ctx->scratch[SB_SORTTMP].ensure(tmp);
  if (rc) return rc;
  HIPCHK(rocprim::exclusive_scan(ctx->scratch[SB_SORTTMP].p, tmp, in, out, (int32_t)0, (size_t)n,
                                 rocprim::plus<int32_t>(), ctx->stream));
  return 0;
}

// record offsets of the node-separable form: the exclusive scan of GInfo::size, read from the pairs' GInfo by the scan itself
// (gbig_list_kernel, which reads every GInfo anyway, puts the offsets into them)
namespace {
struct RecordSize {
  __device__ unsigned long long operator()(const GInfo& g) const { return g.size; }
};
}  // namespace
int sort_scan_record_sizes(ldsim_ctx* ctx, const GInfo* gi, unsigned long long* off, int64_t n) {
  if (n == 0) return 0;
  auto sizes = rocprim::make_transform_iterator(gi, RecordSize());
  size_t tmp = 0;
  HIPCHK(rocprim::exclusive_scan(nullptr, tmp, sizes, off, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), ctx->stream));
  int rc = ctx->scratch[SB_SORTTMP].ensure(tmp);
  if (rc) return rc;
  HIPCHK(rocprim::exclusive_scan(ctx->scratch[SB_SORTTMP].p, tmp, sizes, off, 0ull, (size_t)n,
                                 rocprim::plus<unsigned long long>(), ctx->stream));
  return 0;
}

int sort_exclusive_scan_u64(ldsim_ctx* ctx, const unsigned long long* in, unsigned long long* out, int64_t n) {
  if (n == 0) return 0;
  size_t tmp = 0;
  HIPCHK(rocprim::exclusive_scan(nullptr, tmp, in, out, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), ctx->stream));
  int rc = ctx->scratch[SB_SORTTMP].ensure(tmp);
  if (rc) return rc;
  HIPCHK(rocprim::exclusive_scan(ctx->scratch[SB_SORTTMP].p, tmp, in, out, 0ull, (size_t)n,
                                 rocprim::plus<unsigned long long>(), ctx->stream));
  return 0;
}

int sort_heads(ldsim_ctx* ctx, const unsigned long long* keys, int64_t n_valid, int32_t* heads) {
  if (n_valid == 0) return 0;
  hipLaunchKernelGGL(heads_kernel, dim3(nblk(n_valid, 256)), dim3(256), 0, ctx->stream, keys, n_valid, heads);
  HIPCHK(hipGetLastError());
  return 0;
}

int sort_fill_unique(ldsim_ctx* ctx, const unsigned long long* keys, const int32_t* heads, const int32_t* uidx,
                     int64_t n_valid, int32_t batch0, int32_t* upix, int32_t* ubatch, int64_t* uoff, int64_t U) {
  hipLaunchKernelGGL(fill_unique_kernel, dim3(nblk(n_valid > 0 ? n_valid : 1, 256)), dim3(256), 0, ctx->stream, keys,
                     heads, uidx, n_valid, batch0, upix, ubatch, uoff, U);
  HIPCHK(hipGetLastError());
  return 0;
}

int sort_batch_first(ldsim_ctx* ctx, int64_t seg_begin, int64_t n, int32_t batch0, int32_t* first) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(batch_first_kernel, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, ctx->seg.batch, seg_begin, n,
                     batch0, first);
  HIPCHK(hipGetLastError());
  return 0;
}

int sort_compact_hits(ldsim_ctx* ctx, const int32_t* upix, const int32_t* ubatch, const int32_t* hit_count,
                      const int32_t* hit_off, const double* digit, const double* ticks, int A, int64_t U, int32_t* rows) {
  if (U == 0) return 0;
  hipLaunchKernelGGL(compact_hits_kernel, dim3(nblk(U, 256)), dim3(256), 0, ctx->stream, upix, ubatch, hit_count,
                     hit_off, digit, ticks, A, U, rows);
  HIPCHK(hipGetLastError());
  return 0;
}
