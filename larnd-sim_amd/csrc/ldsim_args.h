// ldsim_args.h -- kernel argument blocks shared by the kernel translation units and the chain glue, and the layouts of what a
// chain launch keeps in the scratch slots: the misc block, the launch counters, the blocks inside a slot, chain_view.
#pragma once
#include <stddef.h>

#include "fee_record.h"
#include "ldsim_dev.h"

// ---- launch counters ----------------------------------------------------------------------------------------------------
// Statistics of a launch: ST_N u64 at `counters` (the flat block), then STAT_STRIPES copies of the block that the kernels add
// to with stat_add -- one workgroup, one stripe (blockIdx mod STAT_STRIPES).  A single address took 1.6 M device-scope atomics
// per launch from gcorr_kernel alone and cost it 2.7 ms of 11 (profiles/r03_phases_gform.log); the host sums the stripes after
// the download (stat_sum).  Flat block only, because the device reads them or the host copies them directly:
// ST_VALID_PAIRS (sort.hip) and ST_POOL_CURSOR.  Every other index lives in the stripes.
enum StatIndex {
  ST_AMBIGUOUS = 0,         // ambiguous-rounding slices
  ST_SAMPLES = 1,           // samples evaluated
  ST_OVERFLOW_PIXELS = 2,   // pixels with pairs beyond their slots (FEE)
  ST_HITS = 3,              // hits (FEE)
  ST_VALID_PAIRS = 4,       // valid (segment, pixel) pairs
  ST_DFMA = 5,              // DFMA lanes
  ST_FALLBACK = 6,          // pairs sent to the monolithic kernel
  ST_POOL_CURSOR = 7,       // doubles requested from the weight pool / written as table records
  ST_DFMA_USEFUL = 8,       // DFMA lanes that carried a term
  ST_STAMP0 = 9,            // 9 .. 15: cycle stamps of the timing tools, summed over waves.  A debug run stamps from one kernel:
  // gcorr_kernel (debug_gform & 128)   gtables_wave_kernel (debug_gform & 2048)
  ST_GCORR_INFO = ST_STAMP0,            ST_GTAB_LOADS = ST_STAMP0,
  ST_GCORR_STAGE = ST_STAMP0 + 1,       ST_GTAB_MAPS = ST_STAMP0 + 1,
  ST_GCORR_G = ST_STAMP0 + 2,           ST_GTAB_BATCH_PROLOGUE = ST_STAMP0 + 2,
  ST_GCORR_P = ST_STAMP0 + 3,           ST_GTAB_TABLES_XY = ST_STAMP0 + 3,
  ST_GCORR_EDGES = ST_STAMP0 + 4,       ST_GTAB_TABLES_Z = ST_STAMP0 + 4,
  ST_GCORR_TAIL = ST_STAMP0 + 5,        ST_GTAB_CELLS = ST_STAMP0 + 5,
  ST_GCORR_LIFE = ST_STAMP0 + 6,        ST_GTAB_LIFE = ST_STAMP0 + 6,
  ST_N = 16
};
#define STAT_STRIPES 64
#define STAT_WORDS (ST_N * (1 + STAT_STRIPES))
#define STAT_BYTES (8 * STAT_WORDS)
#ifdef __HIPCC__
__device__ __forceinline__ void stat_add(unsigned long long* counters, int i, unsigned long long v) {
  atomicAdd(&counters[ST_N * (1 + (blockIdx.x & (STAT_STRIPES - 1))) + i], v);
}
#endif
static inline void stat_sum(const unsigned long long* raw, unsigned long long* sum) {
  for (int i = 0; i < ST_N; i++) {
    sum[i] = raw[i];
    for (int s = 0; s < STAT_STRIPES; s++) sum[i] += raw[ST_N * (1 + s) + i];
  }
}

// ---- the misc block (SB_MISC): the words the host clears before and reads after a stage ------------------------------------
struct ChainMisc {
  int32_t err, pad0;                // quench / drift kernels: error flag
  int32_t nmax, pad1;               // max_pixels: most active pixels of a segment
  unsigned long long tran_bits;     // max_pixels: bits of the largest tran_diff
  int32_t time_max, pad2[9];        // time_intervals stage call: largest tick count
  unsigned int n_compact;           // unused (the stage calls clear the words before it)
  int32_t pad3[47];
  unsigned long long counters[STAT_WORDS];
  char tail[256];
};
#define MISC_BYTES (256 + STAT_BYTES + 256)
static_assert(offsetof(ChainMisc, err) == 0, "misc block layout");
static_assert(offsetof(ChainMisc, nmax) == 8, "misc block layout");
static_assert(offsetof(ChainMisc, tran_bits) == 16, "misc block layout");
static_assert(offsetof(ChainMisc, time_max) == 24, "misc block layout");
static_assert(offsetof(ChainMisc, n_compact) == 64, "misc block layout");
static_assert(offsetof(ChainMisc, counters) == 256, "misc block layout");
static_assert(sizeof(ChainMisc) == MISC_BYTES, "misc block layout");

// ---- blocks inside a slot ---------------------------------------------------------------------------------------------
// SB_MISC behind the ChainMisc (one memset clears both), per batch of a launch:
// tmax i32 [nb] | first i32 [nb] | (16-byte aligned) tran u64 [nb] | radius i32 [nb]
struct BatchBlock {
  int32_t *tmax, *first;
  unsigned long long* tran;
  int32_t* radius;
};
static inline size_t batch_block_bytes(int64_t nb) { return (size_t)nb * 24 + 64; }
static inline BatchBlock batch_block(void* p, int64_t nb) {
  BatchBlock b;
  b.tmax = (int32_t*)p;
  b.first = b.tmax + nb;
  b.tran = (unsigned long long*)((char*)p + ((nb * 8 + 15) / 16) * 16);
  b.radius = (int32_t*)(b.tran + nb);
  return b;
}
// ---- the words a chain launch reads back between its stages (ctx->readback, page-locked) ---------------------------------------
// One copy per word and synchronisation, straight into this block.  Behind it, per batch: tran u64 [nb] | tmax i32 [nb] |
// radius i32 [nb] (the last one goes the other way: the radii the host derives from tran).
struct ChainReadback {
  int32_t nmax, pad;                       // max_pixels
  int32_t last_idx, last_head;             // last entries of the head scan and of the heads: their sum is the unique pixels
  unsigned long long n_valid;              // counters[ST_VALID_PAIRS]
  unsigned long long gform_tot[8];         // gform_launch: pool size and list counts
  unsigned long long raw[STAT_WORDS];      // the launch counters
};
struct ChainReadbackBatch {
  unsigned long long* tran;
  int32_t *tmax, *radius;
};
static inline size_t chain_readback_bytes(int64_t nb) { return sizeof(ChainReadback) + (size_t)nb * 16; }
static inline ChainReadbackBatch chain_readback_batch(void* p, int64_t nb) {
  ChainReadbackBatch b;
  b.tran = (unsigned long long*)((char*)p + sizeof(ChainReadback));
  b.tmax = (int32_t*)(b.tran + nb);
  b.radius = b.tmax + nb;
  return b;
}
// SB_HITCNT: hit_count i32 [U] | hit_off i32 [U] (the exclusive scan of the counts)
struct HitCounts {
  int32_t *count, *off;
};
static inline size_t hit_counts_bytes(int64_t U) { return (size_t)U * 8 + 16; }
static inline HitCounts hit_counts(void* p, int64_t U) { return HitCounts{(int32_t*)p, (int32_t*)p + U}; }

// ---- what the last chain_run left in HBM ---------------------------------------------------------------------------------
// Typed pointers and sizes, computed from the slots at the moment of the call and returned by value.  Not to be kept across a
// call that may launch or grow a buffer: the async download swaps the output slots on every launch, and ensure() may free.
struct ChainView {
  int64_t U, n_hits;                 // unique pixels; hit rows
  int32_t A, M;                      // row lengths of the per-pixel arrays (the constants that hold now)
  int64_t n_pairs;                   // of the FEE set-up record (ctx->fee_rec has the rest of what that launch ran with)
  int32_t T;
  const int32_t *upix, *ubatch;      // [U]
  const double *adc, *ticks, *digit; // [U][A]
  const int64_t* tpm;                // [U][M]
  double* frac;                      // [U][A][M] (completed in place by fractions_complete)
  const int32_t *hit_count, *hit_off;   // [U]
  void* hits;                        // [n_hits] 24-byte rows
  const float* waves;                // [n_pairs][T]
  FeeHdrView fee;                    // FEE set-up record: headers (and list counts)
  const FeeSlot* fee_slots;          //   and slot rows [n_pairs]
};
static inline ChainView chain_view(const ldsim_ctx* ctx) {
  const DevBuf* sb = ctx->scratch;
  const HitCounts hc = hit_counts(sb[SB_HITCNT].p, ctx->chain_U);
  ChainView v;
  v.U = ctx->chain_U;
  v.n_hits = ctx->chain_hits;
  v.A = ctx->h_consts.max_adc_values;
  v.M = ctx->h_consts.max_tracks_per_pixel;
  v.n_pairs = ctx->fee_rec.n_pairs;
  v.T = ctx->fee_rec.T;
  v.upix = sb[SB_UPIX].as<int32_t>();
  v.ubatch = sb[SB_UBATCH].as<int32_t>();
  v.adc = sb[SB_ADC].as<double>();
  v.ticks = sb[SB_TICKS].as<double>();
  v.digit = sb[SB_DIGIT].as<double>();
  v.tpm = sb[SB_TPM].as<int64_t>();
  v.frac = sb[SB_FRAC].as<double>();
  v.hit_count = hc.count;
  v.hit_off = hc.off;
  v.hits = sb[SB_HITS].p;
  v.waves = sb[SB_WAVES].as<float>();
  v.fee = fee_hdr_view(sb[SB_FEEHDR].p, ctx->fee_rec.lists, ctx->chain_U);
  v.fee_slots = sb[SB_FEESLOT].as<FeeSlot>();
  return v;
}

struct CurArgs {
  SegStore s;
  const LdsimConsts* c;
  const double* resp;
  int32_t ni, nj, nk;
  int32_t k_first, k_last;       // response support (exact zeros outside), or [0, nk-1]
  const int32_t* pair_val;       // sorted pair list: value = r*P + ipix   (chain mode) or NULL (dense mode)
  const unsigned long long* pair_key;  // key carrying the pixel id            (chain mode)
  const int32_t* pixels;         // dense mode: pixels[S][P]
  int64_t seg_begin;             // first resident segment of this call (r is relative to it)
  int32_t P;
  int64_t n_pairs;
  float* out;                    // [n_pairs][T]
  int32_t T;                     // row stride == max ticks
  const int32_t* tmax_batch;     // per-batch max_length (chain) or NULL -> T
  int32_t batch0;
  const int32_t* batch_first;    // per-batch first relative segment index (chain) or NULL
  double prune_log;
  double tail_log;        // split path: samples below exp(-tail_log) of the peak density are evaluated in f32 (0 = off)
  int32_t debug_phases;
  int32_t numba_f32;      // 1: the sub-expressions Numba types f32 for f4 record fields are evaluated in float (oracle: o_set_numba_f32)
  int32_t split_max_items;   // validation knob: pairs with more items than this take the monolithic kernel (0 = capacity)
  unsigned long long* counters;  // the launch counters (StatIndex)
  int32_t* win;                  // [n_pairs][2] or NULL.  Set: a kernel that knows a pair's response-visible tick window writes it here
                                 // and leaves the ticks outside it unwritten (the chain's pixel sum reads the window only); NULL: every
                                 // row is written in full (zeros outside the window)
  const int32_t* only_flagged;   // if set: run only pairs whose only_flagged[pair*flag_stride + 7] != 0
  int32_t flag_stride;
  const int32_t* flag_list;      // if set: the flagged pairs as a list of *flag_count entries; a fixed grid walks it (no workgroup per pair
  const unsigned long long* flag_count;   //   that only finds its flag unset)
};

// The constants the FEE kernels use, by value (kernel arguments live in scalar registers): read through the pointer to the
// constants block in HBM every field costs a trip to L2, taken one after the other where the code first needs them -- a dozen
// dependent round trips per pixel in a kernel that is nothing but such chains.
struct FeeK {
  int32_t n_time_ticks, max_adc_values, max_tracks_per_pixel, pad;
  double time_sampling, buffer_risetime, clock_cycle, adc_hold_delay, reset_cycles, adc_busy_delay;
  double reset_noise_charge, uncorrelated_noise_charge, discriminator_noise;
  double v_pedestal, v_cm, v_ref, adc_counts, gain, time_interval1;
};
#define FEEK_FROM(h) FeeK{(h).n_time_ticks, (h).max_adc_values, (h).max_tracks_per_pixel, 0, (h).time_sampling, (h).buffer_risetime, \
                          (h).clock_cycle, (double)(h).adc_hold_delay, (double)(h).reset_cycles, (double)(h).adc_busy_delay,         \
                          (h).reset_noise_charge, (h).uncorrelated_noise_charge, (h).discriminator_noise, (h).v_pedestal, (h).v_cm, \
                          (h).v_ref, (double)(h).adc_counts, (h).gain, (h).time_interval[1]}

struct FeeArgs {
  const LdsimConsts* c;
  FeeK k;
  // unique pixels
  int64_t U;
  const int32_t* upix;
  const int32_t* ubatch;
  const int64_t* uoff;        // [U+1] offsets into the sorted pair list
  // sorted pairs
  const int32_t* pair_val;    // r*P + ipix
  const unsigned long long* pair_key;
  int64_t n_pairs;            // length of the sorted pair list (sizes the set-up pass's slot pool)
  int32_t P;
  const double* track_starts; // [n_seg] relative index r
  const float* waves;         // [n_pairs][T]
  const int32_t* win;         // [n_pairs][2]: the ticks of a row that were written, or NULL = all
  int32_t T;
  const int32_t* batch_first; // [n_batches] first relative segment index of each batch
  int32_t batch0;
  double threshold;
  const double* thr_table;    // [n_pixel_ids] per-pixel thresholds (cli/simulate_pixels.py:1079-1084) or NULL -> threshold
  const double* gain_table;   // [n_pixel_ids] per-pixel gains (:1097-1100) or NULL -> GAIN * mV / e
  double time_padding;
  // outputs
  double* adc_list;           // [U][A]
  double* adc_ticks;          // [U][A]
  double* adc_digit;          // [U][A]
  int64_t* tpm;               // [U][M]
  double* fractions;          // [U][A][M] or NULL
  unsigned long long* counters;  // the launch counters (StatIndex)
  int32_t* hit_count;         // [U]
  // FEE noise (fee.py:557,583-584,616-617,621,649): normals drawn ahead by fee_noise_kernel, or NULL = all noise charges 0
  const float* noise_z;       // [U][noise_nd]
  int32_t noise_nd;
  int32_t* n_draws;           // [U] normals the scan consumed
  // keyed mode (rng.h): row u draws stream key_mix(batch_keys[ubatch[u]], upix[u]) inline, no table (noise_z NULL)
  const uint64_t* batch_keys; // [batch ids of the upload] or NULL = table mode
  uint64_t rng_seed;
  int32_t debug;              // timing tools (debug_phases bits 0x10000 / 0x20000 / 0x40000: no waveform sum / scan / fractions;
                              // read only by a library built with make DEBUG_FEE=1)
  const double* tab;          // launch constants wtap[64] | G[64] (fee_launch_chain sets it: ctx->d_fee_tab)
};
