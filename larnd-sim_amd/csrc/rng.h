// rng.h -- numba.cuda.random's xoroshiro128p generator and float32 Box-Muller normal, as Numba documents them
// (third-party: module `numba`, not under the reference tree; restated, see oracle/ldsim_oracle.c for the statement of
// what is and is not pinned).  Call sites in the reference: fee.py:557,583-584,616-617,621,649; detsim.py:331,336-337.
#pragma once
#include <stdint.h>

struct RngState {
  uint64_t s0, s1;
};

__host__ __device__ inline uint64_t rng_rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
__host__ __device__ inline uint64_t rng_next(RngState& st) {
  uint64_t s0 = st.s0, s1 = st.s1;
  const uint64_t result = s0 + s1;
  s1 ^= s0;
  st.s0 = rng_rotl(s0, 55) ^ s1 ^ (s1 << 14);
  st.s1 = rng_rotl(s1, 36);
  return result;
}
// uint64_to_unit_float32: float32((x >> 11) * 2^-53)  (may round up to 1.0f, like Numba's)
__host__ __device__ inline float rng_uniform_f32(RngState& st) {
  return (float)((double)(rng_next(st) >> 11) * (1.0 / 9007199254740992.0));
}
// xoroshiro128p_normal_float32: z0 of Box-Muller in float32; the second value is discarded
__device__ inline float rng_normal_f32(RngState& st) {
  const float u1 = rng_uniform_f32(st), u2 = rng_uniform_f32(st);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// ---- keyed streams (opt-in: ldsim_rng_keyed_seed) ------------------------------------------------------------------------
// Every number is a pure function of (run seed, stage tag, stream key, draw index): Philox4x32-10 (Salmon et al., SC'11,
// "Parallel random numbers: as easy as 1, 2, 3"), key = the 64-bit run seed (lo, hi), counter = (m, stream key lo, stream key
// hi, stage tag).  Output word x -> uniform ((x >> 8) + 1) * 2^-24 in (0, 1].  Normals: float32 Box-Muller on pairs of
// uniforms, both values kept -- one Philox call gives draws 4m .. 4m+3:
//   r01 = sqrtf(-2 logf(u(x0))), a01 = 2pi_f * u(x1):  draw 4m = r01 * cosf(a01), draw 4m+1 = r01 * sinf(a01)
//   r23 = sqrtf(-2 logf(u(x2))), a23 = 2pi_f * u(x3):  draw 4m+2 = r23 * cosf(a23), draw 4m+3 = r23 * sinf(a23)
// Uniform draw i is u(x_{i mod 4}) of block m = i / 4.  Stream keys are SplitMix64 folds (key_mix) of the identity of what is
// simulated, never of its position in a launch: tests/test_cpu_keyed_rng.py restates all of this in numpy.
enum : uint32_t { RNG_TAG_FEE = 1, RNG_TAG_LIGHT_FLUCT = 2, RNG_TAG_LIGHT_NOISE = 3, RNG_TAG_MC = 4, RNG_TAG_CHARGE = 5, RNG_TAG_LUT = 6, RNG_TAG_GEN = 7 };

__host__ __device__ inline void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  const uint64_t p = (uint64_t)a * b;
  hi = (uint32_t)(p >> 32);
  lo = (uint32_t)p;
}
__host__ __device__ inline void philox4x32_10(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
#pragma unroll
  for (int r = 0; r < 10; r++) {
    uint32_t hi0, lo0, hi1, lo1;
    philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
    philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// SplitMix64's output function, and the fold h' = fin(h ^ fin(x + golden)) of one identity field into a key
__host__ __device__ inline uint64_t key_fin(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t key_mix(uint64_t h, uint64_t x) { return key_fin(h ^ key_fin(x + 0x9E3779B97F4A7C15ULL)); }
#define RNG_KEY_ROOT 0x6A09E667F3BCC909ULL      // h of an empty identity (fractional bits of sqrt(2))

__host__ __device__ inline void keyed_block(uint64_t seed, uint32_t tag, uint64_t key, uint32_t m, uint32_t out[4]) {
  const uint32_t ctr[4] = {m, (uint32_t)key, (uint32_t)(key >> 32), tag};
  philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}
__host__ __device__ inline float keyed_u01(uint32_t x) { return (float)((x >> 8) + 1u) * (1.0f / 16777216.0f); }
// the Box-Muller pair (draws 2j, 2j+1) of two words
__host__ __device__ inline void keyed_bm(uint32_t xa, uint32_t xb, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(keyed_u01(xa)));
  const float a = 6.28318530717958647692f * keyed_u01(xb);
  z0 = r * cosf(a);
  z1 = r * sinf(a);
}
__host__ __device__ inline float keyed_uniform(uint64_t seed, uint32_t tag, uint64_t key, uint32_t i) {
  uint32_t x[4];
  keyed_block(seed, tag, key, i >> 2, x);
  const uint32_t j = i & 3;
  return keyed_u01(j == 0 ? x[0] : j == 1 ? x[1] : j == 2 ? x[2] : x[3]);
}
__host__ __device__ inline float keyed_normal(uint64_t seed, uint32_t tag, uint64_t key, uint32_t i) {
  uint32_t x[4];
  keyed_block(seed, tag, key, i >> 2, x);
  const bool hi = (i & 2) != 0;
  float z0, z1;
  keyed_bm(hi ? x[2] : x[0], hi ? x[3] : x[1], z0, z1);
  return (i & 1) ? z1 : z0;
}
// draws i and i+1 (one Philox call and one Box-Muller pair when i is even)
__host__ __device__ inline void keyed_normal2(uint64_t seed, uint32_t tag, uint64_t key, uint32_t i, float& a, float& b) {
  if ((i & 1) == 0) {
    uint32_t x[4];
    keyed_block(seed, tag, key, i >> 2, x);
    const bool hi = (i & 2) != 0;
    keyed_bm(hi ? x[2] : x[0], hi ? x[3] : x[1], a, b);
  } else {
    a = keyed_normal(seed, tag, key, i);
    b = keyed_normal(seed, tag, key, i + 1);
  }
}
// a serial stream (draws 0, 1, 2, ...): one Philox call per four normals
struct KeyedStream {
  uint64_t seed, key;
  uint32_t tag, n;
  float z[4];
  __host__ __device__ KeyedStream(uint64_t s, uint32_t t, uint64_t k) : seed(s), key(k), tag(t), n(0), z{0, 0, 0, 0} {}
  __host__ __device__ float normal() {
    const uint32_t j = n & 3;
    if (j == 0) {
      uint32_t x[4];
      keyed_block(seed, tag, key, n >> 2, x);
      keyed_bm(x[0], x[1], z[0], z[1]);
      keyed_bm(x[2], x[3], z[2], z[3]);
    }
    n++;
    return j == 0 ? z[0] : j == 1 ? z[1] : j == 2 ? z[2] : z[3];
  }
};
