// fee_scan.h -- the LArPix trigger scan on one wave (fee.py:517-655) and what it is made of: the DPP wave scans, the buffer
// convolution, the digitisation and the two noise sources.  Shared by the kernels of kernels_fee.hip and by
// pixel_adc_universes_kernel (kernels_feeuni.hip), which runs one scan per wave over one summed waveform.
#pragma once
#include "ldsim_dev.h"
#include "rng.h"

// Wave-64 scans with DPP (row shifts inside the 16-lane rows, then row_bcast:15 / :31 across rows: the GFX9 controls gfx950
// keeps) instead of shuffles through the LDS crossbar, whose latency the trigger scan paid six times per 64-tick chunk.
// Lanes without a source read 0 (bound_ctrl), rows masked out keep the `old` operand 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_or_zero(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
  v += dpp_or_zero<0x111, 0xF>(v);       // row_shr:1
  v += dpp_or_zero<0x112, 0xF>(v);       // row_shr:2
  v += dpp_or_zero<0x114, 0xF>(v);       // row_shr:4
  v += dpp_or_zero<0x118, 0xF>(v);       // row_shr:8   -> inclusive scan inside every row of 16
  v += dpp_or_zero<0x142, 0xA>(v);       // row_bcast:15 into rows 1 and 3: + total of the row before
  v += dpp_or_zero<0x143, 0xC>(v);       // row_bcast:31 into rows 2 and 3: + total of lanes 0..31
  return v;
}
// value of lane l (wave-uniform index) in every lane
__device__ __forceinline__ double lane_bcast(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wave_sum(double v) { return lane_bcast(wave_incl_scan(v, 0), 63); }

// q(ic): buffer-convolved charge of tick ic (fee.py:566-579), taps limited by last_reset and N_t.  S holds the ticks
// [s_lo, s_hi) of the pixel's waveform (element 0 = tick s_lo); it is zero outside them.
__device__ __forceinline__ double conv_q(const double* S, int NT, int ic, int last_reset, int ntap, const double* wtap,
                                         double dt, bool has_rt, int s_lo, int s_hi) {
  double q = 0;
  if (has_rt) {
    int cs = ic - ntap;
    if (cs < last_reset) cs = last_reset;
    if (cs < s_lo) cs = s_lo;
    int ce = ic + 1 < NT ? ic + 1 : NT;
    if (ce > s_hi) ce = s_hi;
    for (int jc = cs; jc < ce; jc++) q += S[jc - s_lo] * dt * wtap[ic - jc];
  } else if (ic < NT && ic >= s_lo && ic < s_hi) {
    q = S[ic - s_lo] * dt;
  }
  return q;
}

template <class K>
__device__ __forceinline__ double digitize_one(const K* c, double q, double gain) {
  const double mV = 1e-3 * (1e-6 * 1.0);
  double v = q * gain + c->v_pedestal * mV - c->v_cm * mV;
  v = v > 0 ? v : 0;
  v = rint(v * c->adc_counts / (c->v_ref * mV - c->v_cm * mV));
  double top = c->adc_counts - 1;
  return v < top ? v : top;
}

// ---- the scan itself, shared by the chain and the dense (materialising) kernels -------------------------------
// Runs on wave 0.  S = summed pixel waveform in LDS.  Writes hits into LDS arrays; returns n_hits.
struct HitRec {
  int lr, b;      // span [lr, b] of ticks whose charge entered the hit
  double q;       // adc_list value: integrated charge + the noise terms
  double tq;      // true_q: integrated charge alone, normalises the backtracking fractions (fee.py:633-635)
  double tick;    // adc_ticks_list value
};

// The noise source of the scan: draw i of the pixel's stream.  TableNoise reads what fee_noise_kernel drew ahead (z NULL: every
// noise charge is 0); KeyedNoise computes it where it is consumed (rng.h: draw i of stream `key`, FEE tag).  get2(i) = draws i, i+1.
struct TableNoise {
  const float* z;
  __device__ bool on() const { return z != nullptr; }
  __device__ float get(int i) const { return z[i]; }
  __device__ void get2(int i, float& a, float& b) const { a = z[i]; b = z[i + 1]; }
};
struct KeyedNoise {
  uint64_t seed, key;
  __device__ bool on() const { return true; }
  __device__ float get(int i) const { return keyed_normal(seed, RNG_TAG_FEE, key, (uint32_t)i); }
  __device__ void get2(int i, float& a, float& b) const { keyed_normal2(seed, RNG_TAG_FEE, key, (uint32_t)i, a, b); }
};

// z: this pixel's normal draws in stream order (the noise source above).  The reference
// draws one normal before the loop (reset noise, fee.py:557), two at every pass of the loop (uncorrelated + discriminator
// noise, :583-584, also on busy ticks), two after an integration (:616-617) and one at every reset (:621,649); *n_draws
// returns how many were consumed.  t_stop = time_ticks[-1] of linspace(0, t_stop, NT + 1) (cli/simulate_pixels.py:1072).
// [t_first, t_end): the ticks where S can be non-zero.  Without noise and with a positive threshold the scan's state does not
// change on ticks whose charge is zero while the ADC is idle and the sum below threshold, so it starts at t_first and stops
// once past t_end + ntap with the ADC idle (with noise every tick draws its normals and may trigger: all ticks are walked).
template <class K, class Z>
__device__ int adc_scan(const K* c, const double* S, int NT, double t_stop, double thr, double time_padding,
                        int lane, HitRec* hits /* LDS, [A] */, const double* wtap, int ntap, const Z zs,
                        int* n_draws, int t_first = 0, int t_end = 1 << 30, int s_lo = 0, int s_hi = 1 << 30) {
  const double dt = c->time_sampling;
  const bool has_rt = c->buffer_risetime > 0;
  const int A = c->max_adc_values;
  const int interval = (int)py_round((3 * c->clock_cycle + c->adc_hold_delay * c->clock_cycle) / dt);
  const int reset_ticks = (int)py_round(c->reset_cycles * c->clock_cycle / dt);
  const int busy_ticks = (int)py_round(c->adc_busy_delay * c->clock_cycle / dt);
  const int n_time_ticks = NT + 1;
  const double tstep = t_stop / (double)NT;
  const double s_reset = c->reset_noise_charge, s_unc = c->uncorrelated_noise_charge, s_disc = c->discriminator_noise;
  int ic = 0, iadc = 0, adc_busy = 0, last_reset = 0, cur = 0;
  double q_sum = 0, true_q = 0;
  const bool z = zs.on();
  if (z) q_sum = (double)zs.get(cur++) * s_reset;
  const bool skip_idle = !z && thr > 0;
  if (skip_idle && t_first > 0) ic = t_first < NT ? t_first : NT;
  const int t_quiet = t_end + ntap;            // from here on q(ic) = 0
  while ((ic < NT || adc_busy > 0) && iadc < A) {
    // one chunk of 64 consecutive ticks
    int my_ic = ic + lane;
    int busy_before = adc_busy - lane;           // busy value seen at the top of this lane's iteration
    bool live = (my_ic < NT) || (busy_before > 0);
    // liveness must be contiguous from lane 0: once a lane is dead the loop has ended
    unsigned long long live_mask = __ballot(live);
    int n_live = (live_mask == ~0ull) ? 64 : __ffsll((long long)~live_mask) - 1;
    double q = (lane < n_live) ? conv_q(S, NT, my_ic, last_reset, ntap, wtap, dt, has_rt, s_lo, s_hi) : 0.0;
    const double incl = wave_incl_scan(q, lane);
    double qs = q_sum + incl;
    double q_noise = 0.0, disc_noise = 0.0;
    if (z && lane < n_live) {
      float za, zb;
      zs.get2(cur + 2 * lane, za, zb);
      q_noise = (double)za * s_unc;
      disc_noise = (double)zb * s_disc;
    }
    int busy_after = busy_before > 0 ? busy_before - 1 : 0;
    bool trig = (lane < n_live) && (qs + q_noise >= thr + disc_noise) && (busy_after == 0);
    unsigned long long tm = __ballot(trig);
    if (tm == 0) {
      if (z) cur += 2 * n_live;
      if (n_live < 64) break;
      q_sum = lane_bcast(qs, 63);
      true_q += lane_bcast(incl, 63);
      ic += 64;
      adc_busy = adc_busy > 64 ? adc_busy - 64 : 0;
      if (skip_idle && adc_busy == 0 && ic >= t_quiet) break;      // (lane 63 was idle and below threshold: nothing can follow)
      continue;
    }
    int f = __ffsll((long long)tm) - 1;
    q_sum = lane_bcast(qs, f);
    true_q += lane_bcast(incl, f);
    if (z) cur += 2 * (f + 1);
    int ict = ic + f;
    int integrate_end = ict + interval;
    // integrate the next `interval` ticks (fee.py:590-614)
    double qi = 0;
    for (int base = ict + 1; base <= integrate_end; base += 64) {
      int t = base + lane;
      double v = (t <= integrate_end) ? conv_q(S, NT, t, last_reset, ntap, wtap, dt, has_rt, s_lo, s_hi) : 0.0;
      qi += wave_sum(v);
    }
    q_sum += qi;
    true_q += qi;
    ic = integrate_end + 1;
    double adc = q_sum, disc2 = 0.0;
    if (z) {
      float za, zb;
      zs.get2(cur, za, zb);
      adc = q_sum + (double)za * s_unc;
      disc2 = (double)zb * s_disc;
      cur += 2;
    }
    if (adc < thr + disc2) {  // fee.py:619-628
      ic += reset_ticks;
      q_sum = z ? (double)zs.get(cur++) * s_reset : 0.0;
      true_q = 0;
      last_reset = ic;
      adc_busy = 0;
      continue;
    }
    if (lane == 0) {
      int crossing = ic < n_time_ticks - 1 ? ic : n_time_ticks - 1;
      int post = ic - crossing > 0 ? ic - crossing : 0;
      double tt = (crossing == NT) ? t_stop : crossing * tstep;
      hits[iadc].lr = last_reset;
      hits[iadc].b = integrate_end;
      hits[iadc].q = adc;
      hits[iadc].tq = true_q;
      hits[iadc].tick = tt + time_padding - 2 + post;
    }
    ic += reset_ticks;
    last_reset = ic;
    adc_busy = busy_ticks;
    q_sum = z ? (double)zs.get(cur++) * s_reset : 0.0;
    true_q = 0;
    iadc++;
  }
  *n_draws = cur;
  return iadc;
}
