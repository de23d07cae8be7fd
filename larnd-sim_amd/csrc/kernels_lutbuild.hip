// kernels_lutbuild.hip -- the light LUT's producer: keyed photon transport in a TPC box (ldsim_light_lut_build,
// ldsim_light_lut_trace; include/ldsim.h states the model, larndsim_amd/lut_builder.py restates it in numpy).
//
// Scintillation photons are walked from a voxel of the box [0, Lu] x [0, Lv] x [0, Lw] to rectangular detectors on its walls
// under Rayleigh scattering, bulk absorption and diffuse wall reflection.  All geometry is f64; every uniform is a keyed_uniform
// of the stream (seed, RNG_TAG_LUT, key_mix(key_mix(RNG_KEY_ROOT, voxel), photon)), read serially: draws 0..4 emit, step s reads
// draws 5 + 4s .. 8 + 4s, so a step costs one Philox block (words 1, 2, 3 of block 1 + s and word 0 of block 2 + s).  A photon is
// a pure function of (seed, voxel, photon index): which lane walks it, how the photons are grouped into workgroups and how the
// voxels are sliced into calls cannot change a tally, and the tallies are integers.
//
// lut_build_kernel: one workgroup per (voxel, group of photons).  Lanes are persistent: the walk is ONE loop whose iteration is
// one step of the lane's current photon; a lane whose photon ended tallies it and takes the next index of the group from an LDS
// counter inside the same iteration, so a long walk does not idle the other lanes of its wave.  The rectangles are staged in LDS
// once, grouped by wall.  The group's count / hist / tmin / tsum tile lives in LDS when the workgroup's LDS stays within LUT_LDS_BYTES and is flushed as
// its non-zero cells with global integer atomics; otherwise every arrival goes to global atomics directly.
// lut_trace_kernel: one lane per photon of one voxel, the same lut_emit / lut_step, fate and end state written out.
#include <math.h>

#include "launchers.h"
#include "rng.h"

#define LUT_BLOCK 256
#define LUT_LDS_BYTES (60 * 1024)      // budget of a workgroup's LDS: staged geometry + control words + the tally tile
#define LUT_TMIN_NONE 0x7F800000u      // bits of +inf: tmin of a cell nothing reached

struct LutGeom {
  double L[3];                 // box extents
  double vsize[3];             // voxel extents
  double lambda_t, p_abs;      // 1 / (1/rayleigh + 1/absorption) (inf: no bulk interaction); lambda_t / absorption
  double inv_vg;               // 1 / group velocity, ns / cm
  double rho[6];               // wall reflectivities u0 u1 v0 v1 w0 w1
  int32_t n[3];                // grid
  int32_t emit_mode, max_steps, nprof, ndet;
  int32_t wall_first[7];       // rectangles of wall w: wall_first[w] .. wall_first[w + 1] of the staged list (ascending index)
};

// a rectangle of the staged list: in-plane bounds (cyclic axis order)
struct LutRect {
  double lo0, lo1, hi0, hi1;
};
// what a workgroup stages in LDS (lanes index these by the wall they hit: kept out of the kernel arguments and of registers)
struct LutLds {
  const double* rho;           // [6]
  const int32_t* wall_first;   // [7]
  const LutRect* rect;         // [ndet] grouped by wall
  const int32_t* id;           // [ndet] index of a staged rectangle in the caller's list
};
#define LUT_LDS_HEAD 80        // rho f64 [6] | wall_first i32 [8]

struct LutPhoton {
  double p[3], d[3], path;
  uint64_t key;
  uint32_t x[4];               // Philox block 1 + step of the stream
  int32_t step, fate;          // fate: LUT_WALKING while under way
};
#define LUT_WALKING (-100)

__device__ inline double lut_u(uint32_t x) { return (double)keyed_u01(x); }

// draws 0..4: emission point (uniform in the voxel, clamped into the box; or its centre, draws 0..2 unused) and direction
__device__ inline void lut_emit(const LutGeom& g, uint64_t seed, int64_t voxel, int64_t photon, LutPhoton& ph) {
  ph.key = key_mix(key_mix(RNG_KEY_ROOT, (uint64_t)voxel), (uint64_t)photon);
  uint32_t x0[4];
  keyed_block(seed, RNG_TAG_LUT, ph.key, 0, x0);
  keyed_block(seed, RNG_TAG_LUT, ph.key, 1, ph.x);
  const int64_t ij = voxel / g.n[2];
  const int32_t iv[3] = {(int32_t)(ij / g.n[1]), (int32_t)(ij % g.n[1]), (int32_t)(voxel % g.n[2])};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double lo = (double)iv[k] * g.vsize[k];
    double q = g.emit_mode ? lo + 0.5 * g.vsize[k] : lo + lut_u(x0[k]) * g.vsize[k];
    q = fmin(fmax(q, 0.0), g.L[k]);
    ph.p[k] = q;
  }
  const double mu = 1.0 - 2.0 * lut_u(x0[3]);
  const double phi = 6.283185307179586 * lut_u(ph.x[0]);
  const double s = sqrt(fmax(0.0, 1.0 - mu * mu));
  ph.d[0] = s * cos(phi);
  ph.d[1] = s * sin(phi);
  ph.d[2] = mu;
  ph.path = 0.0;
  ph.step = 0;
  ph.fate = LUT_WALKING;
}

// one step of the walk (include/ldsim.h, "One step"); sets ph.fate when the photon ends
__device__ inline void lut_step(const LutGeom& g, const LutLds& S, uint64_t seed, LutPhoton& ph) {
  const double ua = lut_u(ph.x[1]), ub = lut_u(ph.x[2]), uc = lut_u(ph.x[3]);
  keyed_block(seed, RNG_TAG_LUT, ph.key, (uint32_t)(2 + ph.step), ph.x);
  const double ue = lut_u(ph.x[0]);
  ph.step++;
  const double l = isinf(g.lambda_t) ? INFINITY : -g.lambda_t * log(ua);
  // distance to the walls along d (never negative; on a tie the lowest axis)
  double dw = INFINITY;
  int axis = 0;
  bool far = false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double t = INFINITY;
    if (ph.d[k] > 0) t = fmax((g.L[k] - ph.p[k]) / ph.d[k], 0.0);
    else if (ph.d[k] < 0) t = fmax(ph.p[k] / -ph.d[k], 0.0);
    if (t < dw) {
      dw = t;
      axis = k;
      far = ph.d[k] > 0;
    }
  }
  const double phi = 6.283185307179586 * ue;
  const double cp = cos(phi), sp = sin(phi);
  if (l < dw) {                                  // bulk interaction
#pragma unroll
    for (int k = 0; k < 3; k++) ph.p[k] = ph.p[k] + l * ph.d[k];
    ph.path += l;
    if (ub <= g.p_abs) {
      ph.fate = -1;
      return;
    }
    // Rayleigh: exact inverse of the (1 + mu^2) law, then the usual rotation of d by (mu, phi)
    const double q = 4.0 * uc - 2.0;
    const double A = cbrt(q + sqrt(q * q + 1.0));
    const double mu = fmin(fmax(A - 1.0 / A, -1.0), 1.0);
    const double st = sqrt(fmax(0.0, 1.0 - mu * mu));
    const double dx = ph.d[0], dy = ph.d[1], dz = ph.d[2];
    double nx, ny, nz;
    if (fabs(dz) > 0.99999) {
      nx = st * cp;
      ny = st * sp;
      nz = dz > 0 ? mu : -mu;
    } else {
      const double den = sqrt(1.0 - dz * dz);
      nx = st * (dx * dz * cp - dy * sp) / den + dx * mu;
      ny = st * (dy * dz * cp + dx * sp) / den + dy * mu;
      nz = -st * cp * den + dz * mu;
    }
    const double nn = sqrt(nx * nx + ny * ny + nz * nz);
    ph.d[0] = nx / nn;
    ph.d[1] = ny / nn;
    ph.d[2] = nz / nn;
    return;
  }
  // wall hit
  ph.path += dw;
#pragma unroll
  for (int k = 0; k < 3; k++) ph.p[k] = ph.p[k] + dw * ph.d[k];
  const int a1 = axis == 2 ? 0 : axis + 1, a2 = a1 == 2 ? 0 : a1 + 1;
  // (runtime-indexed registers would go to scratch: select the components instead)
  const double pa = a1 == 0 ? ph.p[0] : a1 == 1 ? ph.p[1] : ph.p[2];
  const double pb = a2 == 0 ? ph.p[0] : a2 == 1 ? ph.p[1] : ph.p[2];
  const double on = far ? (axis == 0 ? g.L[0] : axis == 1 ? g.L[1] : g.L[2]) : 0.0;
  if (axis == 0) ph.p[0] = on; else if (axis == 1) ph.p[1] = on; else ph.p[2] = on;
  const int wall = 2 * axis + (far ? 1 : 0);
  for (int r = S.wall_first[wall]; r < S.wall_first[wall + 1]; r++) {
    const LutRect R = S.rect[r];
    if (R.lo0 <= pa && pa < R.hi0 && R.lo1 <= pb && pb < R.hi1) {
      ph.fate = S.id[r];
      return;
    }
  }
  if (!(ub <= S.rho[wall])) {
    ph.fate = -2;
    return;
  }
  // Lambertian about the inward normal
  const double ct = sqrt(uc), sl = sqrt(1.0 - uc);
  const double dn = far ? -ct : ct, da = sl * cp, db = sl * sp;
  ph.d[0] = axis == 0 ? dn : a1 == 0 ? da : db;
  ph.d[1] = axis == 1 ? dn : a1 == 1 ? da : db;
  ph.d[2] = axis == 2 ? dn : a1 == 2 ? da : db;
}

// geometry into LDS: rho [6] | wall_first [8] | rect [ndet] | ids [ndet] (the dynamic region starts 16-byte aligned: no static
// LDS in these kernels); the caller's barrier publishes it
__device__ inline LutLds lut_stage(const LutGeom& g, const LutRect* __restrict__ d_rect, const int32_t* __restrict__ d_id,
                                   unsigned char* smem) {
  double* rho = (double*)smem;
  int32_t* wf = (int32_t*)(smem + 48);
  LutRect* rect = (LutRect*)(smem + LUT_LDS_HEAD);
  int32_t* id = (int32_t*)(smem + LUT_LDS_HEAD + (size_t)g.ndet * sizeof(LutRect));
  if (threadIdx.x < 6) rho[threadIdx.x] = g.rho[threadIdx.x];
  if (threadIdx.x < 7) wf[threadIdx.x] = g.wall_first[threadIdx.x];
  for (int i = threadIdx.x; i < g.ndet; i += blockDim.x) {
    rect[i] = d_rect[i];
    id[i] = d_id[i];
  }
  return LutLds{rho, wf, rect, id};
}

__host__ __device__ static inline size_t lut_stage_bytes(int ndet) { return (LUT_LDS_HEAD + (size_t)ndet * (sizeof(LutRect) + 4) + 15) & ~(size_t)15; }

// LDS behind the staged rectangles: control words u32 [8] (next photon, three fate counts) | with `tile`: u32 cnt [ndet] |
// u32 tmin [ndet] | u64 tsum [ndet] | u32 hist [ndet][nprof]
__global__ void __launch_bounds__(LUT_BLOCK)
lut_build_kernel(const LutGeom g, const LutRect* __restrict__ d_rect, const int32_t* __restrict__ d_id, uint64_t seed,
                 int64_t voxel_begin, int64_t n_photons, int32_t group, int32_t n_groups, int32_t tile, unsigned* __restrict__ counts,
                 unsigned* __restrict__ hist, unsigned* __restrict__ tmin, unsigned long long* __restrict__ tsum,
                 unsigned long long* __restrict__ fates) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const LutLds S = lut_stage(g, d_rect, d_id, smem);
  unsigned* ctl = (unsigned*)(smem + lut_stage_bytes(g.ndet));
  unsigned long long* t_sum = (unsigned long long*)(ctl + 8);
  unsigned* t_cnt = (unsigned*)(t_sum + g.ndet);
  unsigned* t_min = t_cnt + g.ndet;
  unsigned* t_hist = t_min + g.ndet;
  const int64_t vrel = blockIdx.x / n_groups;
  const int64_t voxel = voxel_begin + vrel;
  const int64_t first = (int64_t)(blockIdx.x % n_groups) * group;
  const unsigned mine = (unsigned)min((int64_t)group, n_photons - first);
  if (threadIdx.x < 8) ctl[threadIdx.x] = 0;
  if (tile) {
    for (int i = threadIdx.x; i < g.ndet; i += LUT_BLOCK) {
      t_sum[i] = 0;
      t_cnt[i] = 0;
      t_min[i] = LUT_TMIN_NONE;
    }
    for (int i = threadIdx.x; i < g.ndet * g.nprof; i += LUT_BLOCK) t_hist[i] = 0;
  }
  __syncthreads();
  const size_t cell0 = (size_t)vrel * g.ndet;
  unsigned n_bulk = 0, n_wall = 0, n_trunc = 0;
  LutPhoton ph;
  ph.fate = 0;                                   // (no photon in hand)
  bool have = false;
  while (true) {
    if (!have) {
      const unsigned i = atomicAdd(&ctl[0], 1u);
      if (i >= mine) break;
      lut_emit(g, seed, voxel, first + i, ph);
      have = true;
    }
    lut_step(g, S, seed, ph);
    if (ph.fate == LUT_WALKING && ph.step >= g.max_steps) ph.fate = -3;
    if (ph.fate != LUT_WALKING) {
      have = false;
      if (ph.fate >= 0) {
        const double t = ph.path * g.inv_vg;
        const int bin = t >= (double)(g.nprof - 1) ? g.nprof - 1 : (int)t;
        const unsigned tb = __float_as_uint((float)t);
        const unsigned long long ts = (unsigned long long)llrint(1024.0 * t);
        if (tile) {
          atomicAdd(&t_cnt[ph.fate], 1u);
          atomicAdd(&t_hist[ph.fate * g.nprof + bin], 1u);
          atomicMin(&t_min[ph.fate], tb);
          atomicAdd(&t_sum[ph.fate], ts);
        } else {
          const size_t c = cell0 + ph.fate;
          atomicAdd(&counts[c], 1u);
          atomicAdd(&hist[c * g.nprof + bin], 1u);
          atomicMin(&tmin[c], tb);
          atomicAdd(&tsum[c], ts);
        }
      } else if (ph.fate == -1) n_bulk++;
      else if (ph.fate == -2) n_wall++;
      else n_trunc++;
    }
  }
  if (n_bulk) atomicAdd(&ctl[1], n_bulk);
  if (n_wall) atomicAdd(&ctl[2], n_wall);
  if (n_trunc) atomicAdd(&ctl[3], n_trunc);
  __syncthreads();
  if (threadIdx.x < 3 && ctl[1 + threadIdx.x]) atomicAdd(&fates[(size_t)vrel * 3 + threadIdx.x], (unsigned long long)ctl[1 + threadIdx.x]);
  if (tile) {
    for (int i = threadIdx.x; i < g.ndet; i += LUT_BLOCK)
      if (t_cnt[i]) {
        atomicAdd(&counts[cell0 + i], t_cnt[i]);
        atomicMin(&tmin[cell0 + i], t_min[i]);
        atomicAdd(&tsum[cell0 + i], t_sum[i]);
      }
    for (int i = threadIdx.x; i < g.ndet * g.nprof; i += LUT_BLOCK)
      if (t_hist[i]) atomicAdd(&hist[cell0 * g.nprof + i], t_hist[i]);
  }
}

// photons [photon_begin, photon_begin + n) of one voxel, a lane each: fate (detector index, or -1 bulk / -2 wall / -3
// truncated), steps, arrival time path / v_g, end point
__global__ void __launch_bounds__(LUT_BLOCK)
lut_trace_kernel(const LutGeom g, const LutRect* __restrict__ d_rect, const int32_t* __restrict__ d_id, uint64_t seed, int64_t voxel,
                 int64_t photon_begin, int64_t n, int32_t* __restrict__ fate, int32_t* __restrict__ steps, double* __restrict__ time,
                 double* __restrict__ end) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const LutLds S = lut_stage(g, d_rect, d_id, smem);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * LUT_BLOCK + threadIdx.x;
  if (i >= n) return;
  LutPhoton ph;
  lut_emit(g, seed, voxel, photon_begin + i, ph);
  while (ph.fate == LUT_WALKING) {
    lut_step(g, S, seed, ph);
    if (ph.fate == LUT_WALKING && ph.step >= g.max_steps) ph.fate = -3;
  }
  fate[i] = ph.fate;
  steps[i] = ph.step;
  time[i] = ph.path * g.inv_vg;
  end[3 * i + 0] = ph.p[0];
  end[3 * i + 1] = ph.p[1];
  end[3 * i + 2] = ph.p[2];
}

__global__ void lut_fill_u32_kernel(unsigned* p, size_t n, unsigned v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static const char* const LUT_WALL_NAME[6] = {"u0", "u1", "v0", "v1", "w0", "w1"};

// checks the parameters, the grid and the rectangles; fills the kernel's geometry and the staged list (grouped by wall, in
// index order inside a wall) in ctx->lb_dets
static int lut_prepare(ldsim_ctx* ctx, const char* who, const LdsimLutBuildParams* P, const LdsimLutDetector* dets, int32_t ndet,
                       int32_t nx, int32_t ny, int32_t nz, LutGeom* g) {
  if (!P || (ndet > 0 && !dets)) {
    ldsim_set_error("%s: null argument", who);
    return LDSIM_EINVAL;
  }
#define LUT_NEED(cond, ...)                 \
  do {                                      \
    if (!(cond)) {                          \
      ldsim_set_error(__VA_ARGS__);         \
      return LDSIM_EINVAL;                  \
    }                                       \
  } while (0)
  LUT_NEED(ndet >= 1 && ndet <= LDSIM_LUT_MAX_DETECTORS, "%s: %d detectors, need 1 .. %d", who, ndet, LDSIM_LUT_MAX_DETECTORS);
  LUT_NEED(P->nprof >= 1 && P->nprof <= LDSIM_LUT_MAX_NPROF, "%s: nprof %d, need 1 .. %d", who, P->nprof, LDSIM_LUT_MAX_NPROF);
  LUT_NEED(nx >= 1 && ny >= 1 && nz >= 1, "%s: zero-sized grid (%d, %d, %d)", who, nx, ny, nz);
  LUT_NEED((int64_t)nx * ny * nz <= 2147483647LL, "%s: more than 2^31 - 1 voxels", who);
  for (int k = 0; k < 3; k++)
    LUT_NEED(std::isfinite(P->box[k]) && P->box[k] > 0, "%s: zero-sized box (extent %d is %g cm)", who, k, P->box[k]);
  LUT_NEED(P->rayleigh_cm > 0 && P->absorption_cm > 0, "%s: rayleigh_cm and absorption_cm must be > 0 (inf allowed)", who);
  LUT_NEED(std::isfinite(P->group_velocity_cm_ns) && P->group_velocity_cm_ns > 0, "%s: group_velocity_cm_ns must be > 0", who);
  for (int w = 0; w < 6; w++)
    LUT_NEED(P->wall_reflectivity[w] >= 0 && P->wall_reflectivity[w] < 1, "%s: wall_reflectivity[%s] = %g, need [0, 1)", who,
             LUT_WALL_NAME[w], P->wall_reflectivity[w]);
  LUT_NEED(P->emit_mode == 0 || P->emit_mode == 1, "%s: emit_mode must be 0 (volume) or 1 (centre)", who);
  LUT_NEED(P->max_steps >= 1, "%s: max_steps must be >= 1", who);
  for (int i = 0; i < ndet; i++) {
    const LdsimLutDetector& d = dets[i];
    LUT_NEED(d.wall >= 0 && d.wall < 6, "%s: detector %d on unknown wall %d", who, i, d.wall);
    const int axis = d.wall / 2;
    for (int c = 0; c < 2; c++) {
      const double ext = P->box[(axis + 1 + c) % 3];
      LUT_NEED(d.lo[c] < d.hi[c], "%s: detector %d is a zero-sized rectangle (lo[%d] = %g, hi[%d] = %g)", who, i, c, d.lo[c], c,
               d.hi[c]);
      LUT_NEED(d.lo[c] >= 0 && d.hi[c] <= ext, "%s: detector %d lies outside wall %s ([%g, %g) of [0, %g] cm)", who, i,
               LUT_WALL_NAME[d.wall], d.lo[c], d.hi[c], ext);
    }
    for (int j = 0; j < i; j++) {
      const LdsimLutDetector& e = dets[j];
      LUT_NEED(!(e.wall == d.wall && e.lo[0] < d.hi[0] && d.lo[0] < e.hi[0] && e.lo[1] < d.hi[1] && d.lo[1] < e.hi[1]),
               "%s: detectors %d and %d overlap on wall %s", who, j, i, LUT_WALL_NAME[d.wall]);
    }
  }
#undef LUT_NEED
  const int32_t n[3] = {nx, ny, nz};
  for (int k = 0; k < 3; k++) {
    g->L[k] = P->box[k];
    g->vsize[k] = P->box[k] / n[k];
    g->n[k] = n[k];
  }
  g->lambda_t = 1.0 / (1.0 / P->rayleigh_cm + 1.0 / P->absorption_cm);
  g->p_abs = std::isinf(g->lambda_t) ? 0.0 : g->lambda_t / P->absorption_cm;
  g->inv_vg = 1.0 / P->group_velocity_cm_ns;
  for (int w = 0; w < 6; w++) g->rho[w] = P->wall_reflectivity[w];
  g->emit_mode = P->emit_mode;
  g->max_steps = P->max_steps;
  g->nprof = P->nprof;
  g->ndet = ndet;
  std::vector<LutRect> rect(ndet);
  std::vector<int32_t> id(ndet);
  int r = 0;
  for (int w = 0; w < 6; w++) {
    g->wall_first[w] = r;
    for (int i = 0; i < ndet; i++)
      if (dets[i].wall == w) {
        rect[r] = {dets[i].lo[0], dets[i].lo[1], dets[i].hi[0], dets[i].hi[1]};
        id[r++] = i;
      }
  }
  g->wall_first[6] = r;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t rb = (size_t)ndet * sizeof(LutRect);
  CK(ctx->lb_dets.ensure(rb + (size_t)ndet * 4));
  HIPCHK(hipMemcpyAsync(ctx->lb_dets.p, rect.data(), rb, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync((char*)ctx->lb_dets.p + rb, id.data(), (size_t)ndet * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));       // (the host vectors go out of scope)
  return 0;
}

int lutbuild_build(ldsim_ctx* ctx, const LdsimLutBuildParams* P, const LdsimLutDetector* dets, int32_t ndet, int32_t nx,
                   int32_t ny, int32_t nz, int64_t voxel_begin, int64_t voxel_end, int64_t n_photons, uint64_t seed,
                   uint32_t* counts, uint32_t* hist, float* tmin, uint64_t* tsum, uint64_t* fates) {
  static const char who[] = "ldsim_light_lut_build";
  LutGeom g;
  CK(lut_prepare(ctx, who, P, dets, ndet, nx, ny, nz, &g));
  const int64_t nvox = (int64_t)nx * ny * nz;
  if (!(voxel_begin >= 0 && voxel_begin <= voxel_end && voxel_end <= nvox)) {
    ldsim_set_error("%s: voxel range [%lld, %lld) outside [0, %lld]", who, (long long)voxel_begin, (long long)voxel_end,
                    (long long)nvox);
    return LDSIM_EINVAL;
  }
  if (!(n_photons >= 1 && n_photons <= 2147483647LL)) {
    ldsim_set_error("%s: n_photons %lld per voxel, need 1 .. 2^31 - 1", who, (long long)n_photons);
    return LDSIM_EINVAL;
  }
  const int64_t nv = voxel_end - voxel_begin;
  ctx->ms_lb = 0;
  if (nv == 0) return 0;
  if (!counts || !hist || !tmin || !tsum || !fates) {
    ldsim_set_error("%s: null output array", who);
    return LDSIM_EINVAL;
  }
  const int32_t group = ctx->lb_group;
  const int64_t n_groups = (n_photons + group - 1) / group;
  if (nv * n_groups > 2147483647LL) {
    ldsim_set_error("%s: %lld voxels x %lld photon groups exceed one launch: build fewer voxels per call or raise "
                    "lut_build_group_photons", who, (long long)nv, (long long)n_groups);
    return LDSIM_EINVAL;
  }
  const size_t cells = (size_t)nv * ndet;
  const size_t tile_bytes = (size_t)ndet * (16 + 4 * (size_t)g.nprof);
  const int tile = ctx->lb_tile && lut_stage_bytes(ndet) + 32 + tile_bytes <= LUT_LDS_BYTES;
  const size_t lds = lut_stage_bytes(ndet) + 32 + (tile ? tile_bytes : 0);
  CK(ctx->lb_counts.ensure(cells * 4));
  CK(ctx->lb_hist.ensure(cells * g.nprof * 4));
  CK(ctx->lb_tmin.ensure(cells * 4));
  CK(ctx->lb_tsum.ensure(cells * 8));
  CK(ctx->lb_fates.ensure((size_t)nv * 24));
  for (Event& e : ctx->lb_ev) CK(e.ensure());
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemsetAsync(ctx->lb_counts.p, 0, cells * 4, st));
  HIPCHK(hipMemsetAsync(ctx->lb_hist.p, 0, cells * g.nprof * 4, st));
  HIPCHK(hipMemsetAsync(ctx->lb_tsum.p, 0, cells * 8, st));
  HIPCHK(hipMemsetAsync(ctx->lb_fates.p, 0, (size_t)nv * 24, st));
  hipLaunchKernelGGL(lut_fill_u32_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, ctx->lb_tmin.as<unsigned>(),
                     cells, LUT_TMIN_NONE);
  const LutRect* d_rect = ctx->lb_dets.as<LutRect>();
  const int32_t* d_id = (const int32_t*)((const char*)ctx->lb_dets.p + (size_t)ndet * sizeof(LutRect));
  HIPCHK(hipEventRecord(ctx->lb_ev[0], st));
  hipLaunchKernelGGL(lut_build_kernel, dim3((unsigned)(nv * n_groups)), dim3(LUT_BLOCK), lds, st, g, d_rect, d_id, seed, voxel_begin,
                     n_photons, group, (int32_t)n_groups, tile, ctx->lb_counts.as<unsigned>(), ctx->lb_hist.as<unsigned>(),
                     ctx->lb_tmin.as<unsigned>(), ctx->lb_tsum.as<unsigned long long>(), ctx->lb_fates.as<unsigned long long>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->lb_ev[1], st));
  HIPCHK(hipMemcpyAsync(counts, ctx->lb_counts.p, cells * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hist, ctx->lb_hist.p, cells * g.nprof * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(tmin, ctx->lb_tmin.p, cells * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(tsum, ctx->lb_tsum.p, cells * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(fates, ctx->lb_fates.p, (size_t)nv * 24, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->lb_ev[0], ctx->lb_ev[1]));
  ctx->ms_lb = ms;
  return 0;
}

int lutbuild_trace(ldsim_ctx* ctx, const LdsimLutBuildParams* P, const LdsimLutDetector* dets, int32_t ndet, int32_t nx,
                   int32_t ny, int32_t nz, int64_t voxel, int64_t photon_begin, int64_t photon_end, uint64_t seed, int32_t* fate,
                   int32_t* steps, double* time, double* end) {
  static const char who[] = "ldsim_light_lut_trace";
  LutGeom g;
  CK(lut_prepare(ctx, who, P, dets, ndet, nx, ny, nz, &g));
  if (!(voxel >= 0 && voxel < (int64_t)nx * ny * nz)) {
    ldsim_set_error("%s: voxel %lld outside the grid", who, (long long)voxel);
    return LDSIM_EINVAL;
  }
  if (!(photon_begin >= 0 && photon_begin <= photon_end && photon_end <= 2147483647LL)) {
    ldsim_set_error("%s: photon range [%lld, %lld) outside [0, 2^31 - 1]", who, (long long)photon_begin, (long long)photon_end);
    return LDSIM_EINVAL;
  }
  const int64_t n = photon_end - photon_begin;
  if (n == 0) return 0;
  if (!fate || !steps || !time || !end) {
    ldsim_set_error("%s: null output array", who);
    return LDSIM_EINVAL;
  }
  // fate i32 [n] | steps i32 [n] | time f64 [n] | end f64 [n][3]
  CK(ctx->lb_trace.ensure((size_t)n * 40));
  int32_t* d_fate = ctx->lb_trace.as<int32_t>();
  int32_t* d_steps = d_fate + n;
  double* d_time = (double*)(d_steps + n);
  double* d_end = d_time + n;
  hipStream_t st = ctx->stream;
  const LutRect* d_rect = ctx->lb_dets.as<LutRect>();
  const int32_t* d_id = (const int32_t*)((const char*)ctx->lb_dets.p + (size_t)ndet * sizeof(LutRect));
  hipLaunchKernelGGL(lut_trace_kernel, dim3((unsigned)((n + LUT_BLOCK - 1) / LUT_BLOCK)), dim3(LUT_BLOCK), lut_stage_bytes(ndet), st, g,
                     d_rect, d_id, seed, voxel, photon_begin, n, d_fate, d_steps, d_time, d_end);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(fate, d_fate, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(steps, d_steps, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(time, d_time, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(end, d_end, (size_t)n * 24, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
