// kernels_seg.hip -- per-segment stages: record unpack/repack, quench, drift, pixel walk, time intervals.
// All of these are HBM-bound (184 B of compulsory traffic per segment); one thread per segment over
// SoA columns so every load/store is a coalesced 8-byte stream.
#include "launchers.h"
#include "rng.h"
#include "seg_charge.h"   // recomb_at, fmap_eval
#include "wave_ops.h"

// ---- AoS <-> SoA ------------------------------------------------------------------------------------------
__device__ __forceinline__ double load_field(const unsigned char* rec, int off, int code) {
  if (off < 0) return 0.0;
  const unsigned char* p = rec + off;
  switch (code) {
    case LDSIM_F4: return (double)*(const float*)p;
    case LDSIM_F8: return *(const double*)p;
    case LDSIM_I4: return (double)*(const int32_t*)p;
    case LDSIM_U4: return (double)*(const uint32_t*)p;
    case LDSIM_I8: return (double)*(const int64_t*)p;
    case LDSIM_U8: return (double)*(const uint64_t*)p;
  }
  return 0.0;
}

__device__ __forceinline__ void store_field(unsigned char* rec, int off, int code, double v) {
  if (off < 0) return;
  unsigned char* p = rec + off;
  switch (code) {
    case LDSIM_F4: *(float*)p = (float)v; break;
    case LDSIM_F8: *(double*)p = v; break;
    case LDSIM_I4: *(int32_t*)p = (int32_t)v; break;
    case LDSIM_U4: *(uint32_t*)p = (uint32_t)v; break;
    case LDSIM_I8: *(int64_t*)p = (int64_t)v; break;
    case LDSIM_U8: *(uint64_t*)p = (uint64_t)v; break;
  }
}

__global__ void __launch_bounds__(256) unpack_kernel(const unsigned char* __restrict__ raw, LdsimTrackLayout lay,
                                                     SegStore s, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned char* rec = raw + i * (int64_t)lay.itemsize;
#pragma unroll
  for (int f = 0; f < LDSIM_NFIELDS - 1; f++) s.f[f][i] = load_field(rec, lay.offset[f], lay.dtype[f]);
  s.pixel_plane[i] = (int32_t)load_field(rec, lay.offset[LDSIM_PIXEL_PLANE], lay.dtype[LDSIM_PIXEL_PLANE]);
}

// write back the fields quench/drift mutate (quenching.py:43-44, drifting.py:41-58)
__global__ void __launch_bounds__(256) repack_kernel(unsigned char* __restrict__ raw, LdsimTrackLayout lay, SegStore s,
                                                     int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned char* rec = raw + i * (int64_t)lay.itemsize;
  const int fields[] = {LDSIM_N_ELECTRONS, LDSIM_N_PHOTONS, LDSIM_LONG_DIFF, LDSIM_TRAN_DIFF,
                        LDSIM_T,           LDSIM_T_START,   LDSIM_T_END};
#pragma unroll
  for (int k = 0; k < 7; k++) store_field(rec, lay.offset[fields[k]], lay.dtype[fields[k]], s.f[fields[k]][i]);
  store_field(rec, lay.offset[LDSIM_PIXEL_PLANE], lay.dtype[LDSIM_PIXEL_PLANE], (double)s.pixel_plane[i]);
}

// ---- a2 quench (quenching.py:11-44) + a3 drift (drifting.py:11-58) -------------------------------------------
// quench_drift_kernel's arithmetic, operation for operation, as helpers of quench_drift_map_kernel (that kernel keeps its
// own text so the path without a map compiles exactly as before).
// Recombination at field e_field (kV/cm): 0 = n_electrons / n_photons written, 1 = unknown mode, 2 = NaN (nothing written)
__device__ __forceinline__ int quench_at(SegStore& s, const LdsimConsts* __restrict__ c, int mode, double e_field, int64_t i,
                                         double& n_e) {
  double dEdx = s.f[LDSIM_DEDX][i], dE = s.f[LDSIM_DE][i];
  double recomb = 0;
  if (mode == 1) {  // BOX
    double csi = c->box_beta * dEdx / (e_field * c->lar_density);
    double r = log(c->box_alpha + csi) / csi;
    recomb = (r > 0) ? r : 0;  // Python max(0, r): NaN -> 0
  } else if (mode == 2) {  // BIRKS
    recomb = c->birks_ab / (1 + c->birks_kb * dEdx / (e_field * c->lar_density));
  } else {
    return 1;
  }
  if (isnan(recomb)) return 2;
  n_e = narrow_store(recomb * dE / c->w_ion, s.store_code[LDSIM_N_ELECTRONS]);
  s.f[LDSIM_N_ELECTRONS][i] = n_e;
  s.f[LDSIM_N_PHOTONS][i] = narrow_store((dE / c->w_ph - n_e) * c->scint_prescale, s.store_code[LDSIM_N_PHOTONS]);
  return 0;
}

// the TPC of a midpoint: the first whose borders (2e-2 cm of slack) hold it, else default_plane_index
__device__ __forceinline__ int32_t tpc_of(const LdsimConsts* __restrict__ c, double x, double y, double z) {
  for (int ip = 0; ip < c->n_tpc; ip++) {
    const double(*p)[2] = c->tpc_borders[ip];
    double zlo = fmin(p[2][1] - 2e-2, p[2][0] - 2e-2), zhi = fmax(p[2][1] + 2e-2, p[2][0] + 2e-2);
    if (p[0][0] - 2e-2 <= x && x <= p[0][1] + 2e-2 && p[1][0] - 2e-2 <= y && y <= p[1][1] + 2e-2 && zlo <= z && z <= zhi)
      return ip;
  }
  return c->default_plane_index;
}

// drift of a segment in TPC `plane` whose charge starts at drift coordinates z (midpoint), zs, ze
__device__ __forceinline__ void drift_at(SegStore& s, const LdsimConsts* __restrict__ c, int32_t plane, int64_t i, double n_e,
                                         double z, double zs, double ze) {
  double z_anode = c->tpc_borders[plane][2][0];
  double t0 = s.f[LDSIM_T0][i];
  double drift_distance = fabs(z - z_anode);
  double drift_start = fabs(fmin(zs, ze) - z_anode);
  double drift_end = fabs(fmax(zs, ze) - z_anode);
  double drift_time = drift_distance / c->v_drift;
  double lifetime_red = exp(-drift_time / c->electron_lifetime);
  s.f[LDSIM_N_ELECTRONS][i] = narrow_store(n_e * lifetime_red, s.store_code[LDSIM_N_ELECTRONS]);
  s.f[LDSIM_LONG_DIFF][i] = narrow_store(sqrt(drift_time * 2 * c->long_diff), s.store_code[LDSIM_LONG_DIFF]);
  s.f[LDSIM_TRAN_DIFF][i] = narrow_store(sqrt(drift_time * 2 * c->tran_diff), s.store_code[LDSIM_TRAN_DIFF]);
  s.f[LDSIM_T][i] = narrow_store(s.f[LDSIM_T][i] + (drift_time + t0), s.store_code[LDSIM_T]);
  s.f[LDSIM_T_START][i] = narrow_store(s.f[LDSIM_T_START][i] + (fmin(drift_start, drift_end) / c->v_drift + t0),
                                       s.store_code[LDSIM_T_START]);
  s.f[LDSIM_T_END][i] = narrow_store(s.f[LDSIM_T_END][i] + (fmax(drift_start, drift_end) / c->v_drift + t0),
                                     s.store_code[LDSIM_T_END]);
}

// do_quench / do_drift select the stage(s); the chain runs both in one pass over the columns.
__global__ void __launch_bounds__(256) quench_drift_kernel(SegStore s, const LdsimConsts* __restrict__ c, int mode,
                                                           int do_quench, int do_drift, int* __restrict__ err) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n) return;
  double n_e = s.f[LDSIM_N_ELECTRONS][i];
  if (do_quench) {
    double dEdx = s.f[LDSIM_DEDX][i], dE = s.f[LDSIM_DE][i];
    double recomb = 0;
    if (mode == 1) {  // BOX
      double csi = c->box_beta * dEdx / (c->e_field * c->lar_density);
      double r = log(c->box_alpha + csi) / csi;
      recomb = (r > 0) ? r : 0;  // Python max(0, r): NaN -> 0
    } else if (mode == 2) {  // BIRKS
      recomb = c->birks_ab / (1 + c->birks_kb * dEdx / (c->e_field * c->lar_density));
    } else {
      *err = 1;
      return;
    }
    if (isnan(recomb)) {
      *err = 2;
    } else {
      n_e = narrow_store(recomb * dE / c->w_ion, s.store_code[LDSIM_N_ELECTRONS]);
      s.f[LDSIM_N_ELECTRONS][i] = n_e;
      s.f[LDSIM_N_PHOTONS][i] =
          narrow_store((dE / c->w_ph - n_e) * c->scint_prescale, s.store_code[LDSIM_N_PHOTONS]);
    }
  }
  if (do_drift) {
    double x = s.f[LDSIM_X][i], y = s.f[LDSIM_Y][i], z = s.f[LDSIM_Z][i];
    int32_t plane = c->default_plane_index;
    for (int ip = 0; ip < c->n_tpc; ip++) {
      const double(*p)[2] = c->tpc_borders[ip];
      double zlo = fmin(p[2][1] - 2e-2, p[2][0] - 2e-2), zhi = fmax(p[2][1] + 2e-2, p[2][0] + 2e-2);
      if (p[0][0] - 2e-2 <= x && x <= p[0][1] + 2e-2 && p[1][0] - 2e-2 <= y && y <= p[1][1] + 2e-2 && zlo <= z &&
          z <= zhi) {
        plane = ip;
        break;
      }
    }
    s.pixel_plane[i] = plane;
    if (plane != c->default_plane_index) {
      double z_anode = c->tpc_borders[plane][2][0];
      double zs = s.f[LDSIM_Z_START][i], ze = s.f[LDSIM_Z_END][i], t0 = s.f[LDSIM_T0][i];
      double drift_distance = fabs(z - z_anode);
      double drift_start = fabs(fmin(zs, ze) - z_anode);
      double drift_end = fabs(fmax(zs, ze) - z_anode);
      double drift_time = drift_distance / c->v_drift;
      double lifetime_red = exp(-drift_time / c->electron_lifetime);
      s.f[LDSIM_N_ELECTRONS][i] = narrow_store(n_e * lifetime_red, s.store_code[LDSIM_N_ELECTRONS]);
      s.f[LDSIM_LONG_DIFF][i] = narrow_store(sqrt(drift_time * 2 * c->long_diff), s.store_code[LDSIM_LONG_DIFF]);
      s.f[LDSIM_TRAN_DIFF][i] = narrow_store(sqrt(drift_time * 2 * c->tran_diff), s.store_code[LDSIM_TRAN_DIFF]);
      s.f[LDSIM_T][i] = narrow_store(s.f[LDSIM_T][i] + (drift_time + t0), s.store_code[LDSIM_T]);
      s.f[LDSIM_T_START][i] = narrow_store(
          s.f[LDSIM_T_START][i] + (fmin(drift_start, drift_end) / c->v_drift + t0), s.store_code[LDSIM_T_START]);
      s.f[LDSIM_T_END][i] = narrow_store(s.f[LDSIM_T_END][i] + (fmax(drift_start, drift_end) / c->v_drift + t0),
                                         s.store_code[LDSIM_T_END]);
    }
  }
}

// ---- drift-field map: quench at the local field, then drift the anode view ------------------------
// One thread per segment.  The TPC comes from the true midpoint; E at the midpoint replaces e_field in the recombination;
// the start, end and midpoint move by (dx, dy, dz) at themselves, clamped into the TPC's box (never further out than the
// true point already was) and rounded like the record's field; the drift reads the moved z.  The nine moved positions go
// to the anode view `view` ([LDSIM_NVIEW][cap]), the true ones stay in the store for the light leg and the output.
__global__ void __launch_bounds__(256) quench_drift_map_kernel(SegStore s, const LdsimConsts* __restrict__ c, int mode,
                                                               const FieldMapDesc* __restrict__ maps,
                                                               double* __restrict__ view, int64_t cap,
                                                               int* __restrict__ err) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n) return;
  double pos[LDSIM_NVIEW];   // start (x, y, z), end (x, y, z), midpoint (x, y, z): the order of enum ldsim_field
#pragma unroll
  for (int k = 0; k < LDSIM_NVIEW; k++) pos[k] = s.f[k][i];
  const int32_t plane = tpc_of(c, pos[LDSIM_X], pos[LDSIM_Y], pos[LDSIM_Z]);
  const bool in_tpc = plane != c->default_plane_index;
  const FieldMapDesc* m = (in_tpc && maps[plane].node) ? &maps[plane] : nullptr;
  double e_field = c->e_field;
  if (m) {
    double v[4];
    fmap_eval(*m, &pos[LDSIM_X], m->has_e != 0, v);
    if (m->has_e) e_field = v[0];
    double d[LDSIM_NVIEW] = {0, 0, 0, 0, 0, 0, v[1], v[2], v[3]};
    for (int p = 0; p < 2; p++) {
      fmap_eval(*m, &pos[3 * p], false, v);
      d[3 * p] = v[1];
      d[3 * p + 1] = v[2];
      d[3 * p + 2] = v[3];
    }
    const double(*b)[2] = c->tpc_borders[plane];
#pragma unroll
    for (int k = 0; k < LDSIM_NVIEW; k++) {
      const int a = k % 3;
      const double lo = fmin(fmin(b[a][0], b[a][1]), pos[k]), hi = fmax(fmax(b[a][0], b[a][1]), pos[k]);
      pos[k] = narrow_store(fmin(fmax(pos[k] + d[k], lo), hi), s.store_code[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < LDSIM_NVIEW; k++) view[k * cap + i] = pos[k];
  double n_e = s.f[LDSIM_N_ELECTRONS][i];
  const int q = quench_at(s, c, mode, e_field, i, n_e);
  if (q == 1) {
    *err = 1;
    return;
  }
  if (q == 2) *err = 2;
  s.pixel_plane[i] = plane;
  if (in_tpc) drift_at(s, c, plane, i, n_e, pos[LDSIM_Z], pos[LDSIM_Z_START], pos[LDSIM_Z_END]);
}

// ---- charge statistics: keyed binomial recombination and attachment ------------------------------
// binomial_draw: seg_charge.h (the light leg's SiPM after-pulses draw with it too)

// drift_at without n_electrons: widths and times written, the drift time returned
__device__ __forceinline__ double drift_times_at(SegStore& s, const LdsimConsts* __restrict__ c, int32_t plane, int64_t i,
                                                 double z, double zs, double ze) {
  double z_anode = c->tpc_borders[plane][2][0];
  double t0 = s.f[LDSIM_T0][i];
  double drift_distance = fabs(z - z_anode);
  double drift_start = fabs(fmin(zs, ze) - z_anode);
  double drift_end = fabs(fmax(zs, ze) - z_anode);
  double drift_time = drift_distance / c->v_drift;
  s.f[LDSIM_LONG_DIFF][i] = narrow_store(sqrt(drift_time * 2 * c->long_diff), s.store_code[LDSIM_LONG_DIFF]);
  s.f[LDSIM_TRAN_DIFF][i] = narrow_store(sqrt(drift_time * 2 * c->tran_diff), s.store_code[LDSIM_TRAN_DIFF]);
  s.f[LDSIM_T][i] = narrow_store(s.f[LDSIM_T][i] + (drift_time + t0), s.store_code[LDSIM_T]);
  s.f[LDSIM_T_START][i] = narrow_store(s.f[LDSIM_T_START][i] + (fmin(drift_start, drift_end) / c->v_drift + t0),
                                       s.store_code[LDSIM_T_START]);
  s.f[LDSIM_T_END][i] = narrow_store(s.f[LDSIM_T_END][i] + (fmax(drift_start, drift_end) / c->v_drift + t0),
                                     s.store_code[LDSIM_T_END]);
  return drift_time;
}

// One thread per segment; quench_drift_kernel (maps = view = NULL) or quench_drift_map_kernel with counted charge:
//   N_i = max(0, rint(dE / W_ion + sqrt(F dE / W_ion) z0)), n_q ~ Binomial(N_i, R), R the recombination factor in [0, 1],
//   n_photons = (dE / W_ph - n_q) scint_prescale, and inside a TPC n_electrons ~ Binomial(n_q, exp(-t_drift / lifetime)).
// Stream (RNG_TAG_CHARGE, key_mix(batch key, index of the segment within its batch)); draw 0 = Fano normal, 1 / 2 =
// recombination normal / uniform, 3 / 4 = attachment normal / uniform, whichever branch a sampler takes.  Segments that are
// not simulated (batch < 0) and a NaN recombination (err = 2) take the mean-value path.
__global__ void __launch_bounds__(256) quench_drift_stat_kernel(SegStore s, const LdsimConsts* __restrict__ c, int mode,
                                                                const FieldMapDesc* __restrict__ maps,
                                                                double* __restrict__ view, int64_t cap, uint64_t seed,
                                                                const uint64_t* __restrict__ batch_keys,
                                                                const int32_t* __restrict__ batch_first, int32_t batch0,
                                                                double fano, int* __restrict__ err) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n) return;
  double pos[LDSIM_NVIEW];
#pragma unroll
  for (int k = 0; k < LDSIM_NVIEW; k++) pos[k] = s.f[k][i];
  const int32_t plane = tpc_of(c, pos[LDSIM_X], pos[LDSIM_Y], pos[LDSIM_Z]);
  const bool in_tpc = plane != c->default_plane_index;
  const FieldMapDesc* m = (maps && in_tpc && maps[plane].node) ? &maps[plane] : nullptr;
  double e_field = c->e_field;
  if (m) {
    double v[4];
    fmap_eval(*m, &pos[LDSIM_X], m->has_e != 0, v);
    if (m->has_e) e_field = v[0];
    double d[LDSIM_NVIEW] = {0, 0, 0, 0, 0, 0, v[1], v[2], v[3]};
    for (int p = 0; p < 2; p++) {
      fmap_eval(*m, &pos[3 * p], false, v);
      d[3 * p] = v[1];
      d[3 * p + 1] = v[2];
      d[3 * p + 2] = v[3];
    }
    const double(*b)[2] = c->tpc_borders[plane];
#pragma unroll
    for (int k = 0; k < LDSIM_NVIEW; k++) {
      const int a = k % 3;
      const double lo = fmin(fmin(b[a][0], b[a][1]), pos[k]), hi = fmax(fmax(b[a][0], b[a][1]), pos[k]);
      pos[k] = narrow_store(fmin(fmax(pos[k] + d[k], lo), hi), s.store_code[k]);
    }
  }
  if (view) {
#pragma unroll
    for (int k = 0; k < LDSIM_NVIEW; k++) view[k * cap + i] = pos[k];
  }
  const int32_t b = s.batch[i];
  double n_e = s.f[LDSIM_N_ELECTRONS][i];
  float z_att = 0, u_att = 0;
  bool drawn = false;
  int q;
  if (b < 0) {
    q = quench_at(s, c, mode, e_field, i, n_e);
  } else {
    double recomb;
    q = recomb_at(c, mode, e_field, s.f[LDSIM_DEDX][i], recomb);
    if (q == 0) {
      const uint64_t key = key_mix(batch_keys[b], (uint64_t)(i - batch_first[b - batch0]));
      const double dE = s.f[LDSIM_DE][i], n0 = dE / c->w_ion;
      const double n_i = fmax(0.0, rint(n0 + sqrt(fano * n0) * (double)keyed_normal(seed, RNG_TAG_CHARGE, key, 0)));
      n_e = binomial_draw(n_i, fmin(fmax(recomb, 0.0), 1.0), keyed_normal(seed, RNG_TAG_CHARGE, key, 1),
                          keyed_uniform(seed, RNG_TAG_CHARGE, key, 2));
      z_att = keyed_normal(seed, RNG_TAG_CHARGE, key, 3);
      u_att = keyed_uniform(seed, RNG_TAG_CHARGE, key, 4);
      s.f[LDSIM_N_ELECTRONS][i] = narrow_store(n_e, s.store_code[LDSIM_N_ELECTRONS]);
      s.f[LDSIM_N_PHOTONS][i] = narrow_store((dE / c->w_ph - n_e) * c->scint_prescale, s.store_code[LDSIM_N_PHOTONS]);
      drawn = true;
    }
  }
  if (q == 1) {
    *err = 1;
    return;
  }
  if (q == 2) *err = 2;
  s.pixel_plane[i] = plane;
  if (!in_tpc) return;
  if (!drawn) {
    drift_at(s, c, plane, i, n_e, pos[LDSIM_Z], pos[LDSIM_Z_START], pos[LDSIM_Z_END]);
    return;
  }
  const double drift_time = drift_times_at(s, c, plane, i, pos[LDSIM_Z], pos[LDSIM_Z_START], pos[LDSIM_Z_END]);
  s.f[LDSIM_N_ELECTRONS][i] =
      narrow_store(binomial_draw(n_e, exp(-drift_time / c->electron_lifetime), z_att, u_att), s.store_code[LDSIM_N_ELECTRONS]);
}

// ---- pixel walk (pixels_from_track.py:43-65, 111-199) ----------------------------------------------------------
struct Walk {
  int64_t x0, y0, x1, y1, plane;
};

__device__ __forceinline__ bool walk_init(const SegStore& s, const LdsimConsts* c, int64_t i, Walk& w) {
  int32_t plane = s.pixel_plane[i];
  if (plane < 0 || plane >= c->n_tpc) return false;  // reference indexes TPC_BORDERS out of bounds here
  const double(*b)[2] = c->tpc_borders[plane];
  w.x0 = (int64_t)py_floordiv(s.f[LDSIM_X_START][i] - b[0][0], c->pixel_pitch);
  w.y0 = (int64_t)py_floordiv(s.f[LDSIM_Y_START][i] - b[1][0], c->pixel_pitch);
  w.x1 = (int64_t)py_floordiv(s.f[LDSIM_X_END][i] - b[0][0], c->pixel_pitch);
  w.y1 = (int64_t)py_floordiv(s.f[LDSIM_Y_END][i] - b[1][0], c->pixel_pitch);
  w.plane = plane;
  return true;
}

// Bresenham without diagonal moves; returns the number of in-range cells, writes ids at walk positions
__device__ __forceinline__ int64_t walk_pixels(const LdsimConsts* c, Walk w, int32_t* out, int64_t cap) {
  int64_t x0 = w.x0, y0 = w.y0;
  int64_t dx = llabs(w.x1 - x0), sx = x0 < w.x1 ? 1 : -1;
  int64_t dy = -llabs(w.y1 - y0), sy = y0 < w.y1 ? 1 : -1;
  int64_t err = dx + dy, n = 0, i = 0;
  if (pix_in_range(c, x0, y0, w.plane)) {
    if (out && i < cap) out[i] = (int32_t)pixel2id(c, x0, y0, w.plane);
    n++;
  }
  while (x0 != w.x1 || y0 != w.y1) {
    i++;
    int64_t e2 = 2 * err;
    if (e2 - dy > dx - e2) {
      err += dy;
      x0 += sx;
    } else {
      err += dx;
      y0 += sy;
    }
    if (pix_in_range(c, x0, y0, w.plane)) {
      if (out && i < cap) out[i] = (int32_t)pixel2id(c, x0, y0, w.plane);
      n++;
    }
  }
  return n;
}

// a5 max_pixels: atomic max of the in-range walk length; also the batch's max tran_diff (for max_radius,
// cli/simulate_pixels.py:918) as order-preserving float bits.
__global__ void __launch_bounds__(256) max_pixels_kernel(SegStore s, const LdsimConsts* __restrict__ c, int64_t begin,
                                                         int64_t end, int32_t* __restrict__ n_max,
                                                         unsigned long long* __restrict__ max_tran_bits) {
  int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int32_t k = 0;
  double td = 0;
  if (i < end) {
    Walk w;
    if (walk_init(s, c, i, w)) k = (int32_t)walk_pixels(c, w, nullptr, 0);
    td = s.f[LDSIM_TRAN_DIFF][i];
    if (!(td > 0)) td = 0;
  }
  // wave-64 reduction, then one atomic per wave
  for (int off = 32; off > 0; off >>= 1) {
    k = max(k, __shfl_down(k, off));
    td = fmax(td, __shfl_down(td, off));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(n_max, k);
    atomicMax(max_tran_bits, (unsigned long long)__double_as_longlong(td));
  }
}

// The chain's front in one pass over the segment columns of [begin, begin + n): a8 time_intervals per batch (starts; the batch's
// largest tick count by atomic max), the first relative segment index of every batch, a5 max_pixels over every segment of the
// range, and the batch's largest tran_diff (sets its max_radius, cli/simulate_pixels.py:918) as order-preserving float bits.
// n_max and the per-batch words are zeroed by the caller.
// Segments are sorted by batch, so nearly every wave holds one batch: one atomic per wave instead of one per segment on
// the few per-batch cells (50 k contended atomics cost 0.7 ms per launch).
__global__ void __launch_bounds__(256) seg_front_kernel(SegStore s, const LdsimConsts* __restrict__ c, int64_t begin, int64_t n,
                                                        int32_t batch0, double* __restrict__ starts, int32_t* __restrict__ n_max,
                                                        int32_t* __restrict__ tmax_b, int32_t* __restrict__ first_b,
                                                        unsigned long long* __restrict__ tran_b) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t b = -1, len_i = 0, k = 0;
  double td = 0;
  if (r < n) {
    const int64_t i = begin + r;
    double t_end = py_round((s.f[LDSIM_T_END][i] + 1) / c->time_sampling) * c->time_sampling;
    double t_start = py_round((s.f[LDSIM_T_START][i] - c->time_padding) / c->time_sampling) * c->time_sampling;
    starts[r] = t_start;
    b = s.batch[i];
    if (b >= 0) {
      double len = ceil((t_end - t_start) / c->time_sampling);
      if (len > 0 && len < 2.0e9) len_i = (int32_t)len;
      td = s.f[LDSIM_TRAN_DIFF][i];
      if (!(td > 0)) td = 0;
      if (r == 0 || s.batch[i - 1] != b) first_b[b - batch0] = (int32_t)r;
    }
    Walk w;
    if (walk_init(s, c, i, w)) k = (int32_t)walk_pixels(c, w, nullptr, 0);
  }
  const int km = wave_max_i32(k);
  if (lane == 0 && km > 0) atomicMax(n_max, km);
  const unsigned long long act = __ballot(b >= 0);
  if (act == 0) return;
  const int first = __ffsll((long long)act) - 1;
  const int bref = __builtin_amdgcn_readlane(b, first);
  if (__ballot(b >= 0 && b != bref) == 0) {
    const int m = wave_max_i32(len_i);
    const double tm = wave_max_f64(td);
    if (lane == first) {
      if (m > 0) atomicMax(&tmax_b[bref - batch0], m);
      if (tm > 0) atomicMax(&tran_b[bref - batch0], (unsigned long long)__double_as_longlong(tm));
    }
    return;
  }
  if (b < 0) return;
  if (len_i > 0) atomicMax(&tmax_b[b - batch0], len_i);
  if (td > 0) atomicMax(&tran_b[b - batch0], (unsigned long long)__double_as_longlong(td));
}

__device__ __forceinline__ int32_t ring_code(int x_r, int y_r) {  // pixels_from_track.py:246-269
  int dx = abs(x_r), dy = abs(y_r), dmax = max(dx, dy), dmin = min(dx, dy), dsum = dmax + dmin;
  if (dsum > 4) return -1;
  if (dsum <= 1) return dsum;
  if (dsum == 2) return dmax == 1 ? 2 : 3;
  if (dsum == 3) return dmax == 2 ? 4 : 5;
  return dmax == 2 ? 6 : (dmax == 3 ? 7 : 8);
}

// a6 get_pixels: active pixel ids (walk order, -1 gaps), first-seen-unique neighbour union, ring codes.
// The kernel writes every slot of its rows, the empty ones (-1, the reference's cp.full(..., -1)) too: the active rows of a
// workgroup's segments are cleared before the walk, which leaves gaps, and the slots of the neighbour and ring-code rows behind
// a segment's count are written after it -- by the whole workgroup, whose rows are one contiguous range.  No slot of
// [0, n * max_active) and [0, n * P) keeps what an earlier launch left in the buffers.
#define GP_THREADS 128
__global__ void __launch_bounds__(GP_THREADS) get_pixels_kernel(SegStore s, const LdsimConsts* __restrict__ c, int64_t begin,
                                                         int64_t end, int radius, int32_t* __restrict__ active,
                                                         int max_active, int32_t* __restrict__ neigh,
                                                         int32_t* __restrict__ nrad, int P,
                                                         double* __restrict__ n_list,
                                                         const int32_t* __restrict__ radius_b, int32_t batch0) {
  __shared__ int s_count[GP_THREADS];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * GP_THREADS;
  const int64_t left = end - begin - r0;
  const unsigned rows = (unsigned)(left < GP_THREADS ? left : GP_THREADS);      // (the grid covers the range: rows >= 1)
  {
    int32_t* a0 = active + r0 * max_active;
    const unsigned na = rows * (unsigned)max_active;
    for (unsigned e = tid; e < na; e += GP_THREADS) a0[e] = -1;
  }
  __syncthreads();
  const int64_t r = r0 + tid;
  const int64_t i = begin + r;
  int count = 0;
  Walk w;
  if (i < end && walk_init(s, c, i, w)) {
    // the reference derives max_radius per batch from max(tran_diff) (cli/simulate_pixels.py:918)
    if (radius_b) {
      int32_t b = s.batch[i];
      radius = b >= 0 ? radius_b[b - batch0] : 0;
    }
    int32_t* act = active + r * max_active;
    int32_t* ng = neigh + r * P;
    int32_t* nr = nrad + r * P;
    walk_pixels(c, w, act, max_active);
    for (int p = 0; p < max_active; p++) {
      int32_t a = act[p];
      if (a == -1) continue;
      int64_t ax, ay, pl;
      id2pixel(c, a, ax, ay, pl);
      for (int x_r = -radius; x_r <= radius; x_r++)
        for (int y_r = -radius; y_r <= radius; y_r++) {
          int64_t nx = ax + x_r, ny = ay + y_r;
          if (!pix_in_range(c, nx, ny, pl)) continue;
          int32_t np_ = (int32_t)pixel2id(c, nx, ny, pl);
          bool uniq = true;
          for (int q = 0; q < count; q++)  // (entries >= count are not read)
            if (ng[q] == np_) {
              uniq = false;
              break;
            }
          if (uniq && count < P) {
            ng[count] = np_;
            nr[count] = ring_code(x_r, y_r);
            count++;
          }
        }
    }
  }
  if (i < end && n_list) n_list[r] = (double)count;
  s_count[tid] = count;
  __syncthreads();
  {
    int32_t* g0 = neigh + r0 * P;
    int32_t* d0 = nrad + r0 * P;
    const unsigned ne = rows * (unsigned)P;
    for (unsigned e = tid; e < ne; e += GP_THREADS) {
      const unsigned row = e / (unsigned)P;
      if ((int)(e - row * (unsigned)P) >= s_count[row]) {
        g0[e] = -1;
        d0[e] = -1;
      }
    }
  }
}

// a8 time_intervals (detsim.py:18-40); max_length per launch via atomic max
__global__ void __launch_bounds__(256) time_intervals_kernel(SegStore s, const LdsimConsts* __restrict__ c,
                                                             int64_t begin, int64_t end, double* __restrict__ starts,
                                                             int32_t* __restrict__ tmax) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t i = begin + r;
  int32_t k = 0;
  if (i < end) {
    double t_end = py_round((s.f[LDSIM_T_END][i] + 1) / c->time_sampling) * c->time_sampling;
    double t_start = py_round((s.f[LDSIM_T_START][i] - c->time_padding) / c->time_sampling) * c->time_sampling;
    starts[r] = t_start;
    double len = ceil((t_end - t_start) / c->time_sampling);
    k = (len > 0 && len < 2.0e9) ? (int32_t)len : 0;
  }
  for (int off = 32; off > 0; off >>= 1) k = max(k, __shfl_down(k, off));
  if ((threadIdx.x & 63) == 0 && k > 0) atomicMax(tmax, k);
}

// ---- host launchers ----------------------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

int seg_launch_unpack(ldsim_ctx* ctx, const LdsimTrackLayout* lay, int64_t n) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(unpack_kernel, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream,
                     (const unsigned char*)ctx->raw.p, *lay, ctx->seg, n);
  HIPCHK(hipGetLastError());
  return 0;
}
int seg_launch_repack(ldsim_ctx* ctx, const LdsimTrackLayout* lay, int64_t n) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(repack_kernel, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, (unsigned char*)ctx->raw.p, *lay,
                     ctx->seg, n);
  HIPCHK(hipGetLastError());
  return 0;
}
int seg_launch_quench_drift(ldsim_ctx* ctx, int mode, int do_q, int do_d, int* d_err) {
  if (ctx->seg.n == 0) return 0;
  hipLaunchKernelGGL(quench_drift_kernel, dim3(nblk(ctx->seg.n, 256)), dim3(256), 0, ctx->stream, ctx->seg,
                     ctx->d_consts.as<LdsimConsts>(), mode, do_q, do_d, d_err);
  HIPCHK(hipGetLastError());
  return 0;
}
int seg_launch_quench_drift_map(ldsim_ctx* ctx, int mode, int* d_err) {
  if (ctx->seg.n == 0) return 0;
  hipLaunchKernelGGL(quench_drift_map_kernel, dim3(nblk(ctx->seg.n, 256)), dim3(256), 0, ctx->stream, ctx->seg,
                     ctx->d_consts.as<LdsimConsts>(), mode, (const FieldMapDesc*)ctx->d_fmap.as<FieldMapDesc>(), (double*)ctx->fmap_view.p, ctx->fmap_view_cap,
                     d_err);
  HIPCHK(hipGetLastError());
  return 0;
}
int seg_launch_quench_drift_stat(ldsim_ctx* ctx, int mode, bool map, const int32_t* d_first, int32_t batch0, int* d_err) {
  if (ctx->seg.n == 0) return 0;
  hipLaunchKernelGGL(quench_drift_stat_kernel, dim3(nblk(ctx->seg.n, 256)), dim3(256), 0, ctx->stream, ctx->seg,
                     ctx->d_consts.as<LdsimConsts>(), mode, map ? (const FieldMapDesc*)ctx->d_fmap.as<FieldMapDesc>() : nullptr,
                     map ? (double*)ctx->fmap_view.p : nullptr, ctx->fmap_view_cap, ctx->rng_seed,
                     (const uint64_t*)ctx->d_batch_keys.p, d_first, batch0, ctx->charge_stat_fano, d_err);
  HIPCHK(hipGetLastError());
  return 0;
}
int seg_launch_max_pixels(ldsim_ctx* ctx, int64_t b, int64_t e, int32_t* d_nmax, unsigned long long* d_tranbits) {
  if (e <= b) return 0;
  hipLaunchKernelGGL(max_pixels_kernel, dim3(nblk(e - b, 256)), dim3(256), 0, ctx->stream, charge_store(ctx), ctx->d_consts.as<LdsimConsts>(),
                     b, e, d_nmax, d_tranbits);
  HIPCHK(hipGetLastError());
  return 0;
}
int seg_launch_front(ldsim_ctx* ctx, int64_t b, int64_t e, int32_t batch0, double* starts, int32_t* d_nmax, int32_t* tmax_b,
                     int32_t* first_b, unsigned long long* tran_b) {
  if (e <= b) return 0;
  hipLaunchKernelGGL(seg_front_kernel, dim3(nblk(e - b, 256)), dim3(256), 0, ctx->stream, charge_store(ctx),
                     ctx->d_consts.as<LdsimConsts>(), b, e - b, batch0, starts, d_nmax, tmax_b, first_b, tran_b);
  HIPCHK(hipGetLastError());
  return 0;
}
int seg_launch_get_pixels(ldsim_ctx* ctx, int64_t b, int64_t e, int radius, int32_t* active, int max_active,
                          int32_t* neigh, int32_t* nrad, int P, double* n_list, const int32_t* radius_b,
                          int32_t batch0) {
  if (e <= b) return 0;
  hipLaunchKernelGGL(get_pixels_kernel, dim3(nblk(e - b, GP_THREADS)), dim3(GP_THREADS), 0, ctx->stream, charge_store(ctx), ctx->d_consts.as<LdsimConsts>(),
                     b, e, radius, active, max_active, neigh, nrad, P, n_list, radius_b, batch0);
  HIPCHK(hipGetLastError());
  return 0;
}
int seg_launch_time_intervals(ldsim_ctx* ctx, int64_t b, int64_t e, double* starts, int32_t* tmax) {
  if (e <= b) return 0;
  hipLaunchKernelGGL(time_intervals_kernel, dim3(nblk(e - b, 256)), dim3(256), 0, ctx->stream, charge_store(ctx),
                     ctx->d_consts.as<LdsimConsts>(), b, e, starts, tmax);
  HIPCHK(hipGetLastError());
  return 0;
}
