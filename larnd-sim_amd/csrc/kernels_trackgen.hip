// kernels_trackgen.hip -- the segments' producer: keyed transport of muons, pions and protons through liquid argon
// (ldsim_track_gen_count, ldsim_track_gen; include/ldsim.h states the model, larndsim_amd/track_generator.py restates it in numpy).
//
// A primary is walked step by step under Bethe energy loss (restricted mean, Gaussian soft fluctuation, sampled hard collisions)
// and Highland scattering; every step is one segment.  All arithmetic is f64; every draw is a word of the stream (seed,
// RNG_TAG_GEN, key_mix(key_mix(RNG_KEY_ROOT, event_id), track_in_event)), step s owning the Philox blocks 32 s .. 32 s + 31: block
// 0 gives the soft normal (words 0, 1) and the two scattering normals (words 2, 3), block 1 word 0 the Poisson uniform, blocks
// 2 + 2 j, 3 + 2 j the four (energy, acceptance) pairs of hard collision j.  A walk is a pure function of (parameters, primary,
// seed): which lane walks it, how the primaries are grouped into workgroups and what else is in the call cannot change it.
//
// gen_kernel<WRITE>: one workgroup per group of primaries.  Lanes are persistent: the walk is ONE loop whose iteration is one step
// of the lane's current primary; a lane whose walk ended takes the next primary of the group from an LDS counter inside the same
// iteration, so a long walk does not idle the other lanes of its wave before the group runs out.  The count pass (WRITE = false)
// writes every primary's number of segments and end state; after an exclusive scan the write pass walks again and stores segment
// (primary, step) at offset[primary] + step: the output order is fixed whatever the scheduling.
#include <math.h>

#include "launchers.h"
#include "rng.h"

#define GEN_BLOCK 256
#define GEN_C_LIGHT 29979.2458        // cm / us
#define GEN_TWO_PI 6.283185307179586
#define GEN_WALKING (-1)

struct GenConst {
  double lo[3], hi[3];
  double step, min_step, frac, t_cut, t_min;
  double kzr;                         // K (Z/A) rho, MeV / cm
  double i2;                          // I^2, MeV^2
  double x0cm;                        // X0 / rho, cm
  double sa, sk, sx0, sx1, scbar, sd0;   // Sternheimer
  int32_t straggling, mcs, eloss, max_steps;
};

struct GenWalk {
  double px, py, pz, dx, dy, dz;
  double T, t, path, M;
  uint64_t key;
  int32_t step, state, pdg, event;
};

struct GenSeg {
  double xs, ys, zs, xe, ye, ze, h, dE, t0, t1;
};

struct GenKin {
  double bg2, beta2, gamma, tmax;
};

__host__ __device__ inline double gen_mass(int32_t pdg) {
  const int32_t a = pdg < 0 ? -pdg : pdg;
  return a == 13 ? LDSIM_TRACK_GEN_M_MUON : a == 211 ? LDSIM_TRACK_GEN_M_PION : LDSIM_TRACK_GEN_M_PROTON;
}

__host__ __device__ inline GenKin gen_kin(double T, double M) {
  GenKin k;
  const double tau = T / M;
  k.bg2 = tau * (tau + 2.0);
  k.gamma = tau + 1.0;
  k.beta2 = k.bg2 / (k.gamma * k.gamma);
  const double r = LDSIM_TRACK_GEN_ME / M;
  k.tmax = 2.0 * LDSIM_TRACK_GEN_ME * k.bg2 / (1.0 + 2.0 * k.gamma * r + r * r);
  return k;
}

__host__ __device__ inline double gen_delta(const GenConst& g, double bg2) {
  const double x = 0.5 * log10(bg2);
  const double hi = 2.0 * 2.302585092994046 * x - g.scbar;
  if (x >= g.sx1) return hi;
  if (x >= g.sx0) return hi + g.sa * pow(g.sx1 - x, g.sk);
  return g.sd0 * pow(10.0, 2.0 * (x - g.sx0));
}

// MeV / cm lost to collisions below tc (tc = k.tmax: the unrestricted Bethe mean)
__host__ __device__ inline double gen_rate(const GenConst& g, const GenKin& k, double tc) {
  return g.kzr / k.beta2 *
         (0.5 * log(2.0 * LDSIM_TRACK_GEN_ME * k.bg2 * tc / g.i2) - 0.5 * k.beta2 * (1.0 + tc / k.tmax) - 0.5 * gen_delta(g, k.bg2));
}

__device__ inline double gen_u(uint32_t x) { return (double)keyed_u01(x); }

// one step of the walk (include/ldsim.h, "One step"); sets w.state when the walk ends
__device__ inline void gen_step(const GenConst& g, uint64_t seed, GenWalk& w, GenSeg& sg) {
  const uint32_t blk = (uint32_t)LDSIM_TRACK_GEN_STEP_BLOCKS * (uint32_t)w.step;
  GenKin k = gen_kin(w.T, w.M);
  const double s_full = gen_rate(g, k, k.tmax);
  double h = fmax(fmin(g.step, g.frac * w.T / s_full), g.min_step);
  // distance to the walls along d (never negative; on a tie the lowest axis)
  double dw = INFINITY;
  int axis = 0;
  bool far = false;
  {
    const double p[3] = {w.px, w.py, w.pz}, d[3] = {w.dx, w.dy, w.dz};
#pragma unroll
    for (int a = 0; a < 3; a++) {
      double t = INFINITY;
      if (d[a] > 0) t = fmax((g.hi[a] - p[a]) / d[a], 0.0);
      else if (d[a] < 0) t = fmax((p[a] - g.lo[a]) / -d[a], 0.0);
      if (t < dw) {
        dw = t;
        axis = a;
        far = d[a] > 0;
      }
    }
  }
  bool leaves = dw <= h;
  if (leaves) h = dw;
  uint32_t x0[4] = {0, 0, 0, 0};
  if ((g.straggling && g.eloss) || g.mcs) keyed_block(seed, RNG_TAG_GEN, w.key, blk, x0);
  double Tm = w.T, dE = 0.0;
  bool stops = false;
  if (g.eloss) {
    Tm = fmax(w.T - 0.5 * s_full * h, g.t_min);
    k = gen_kin(Tm, w.M);
    const double tc = g.straggling ? fmin(g.t_cut, k.tmax) : k.tmax;
    const double s_mean = gen_rate(g, k, tc);
    dE = s_mean * h;
    if (g.straggling) {
      const double xi = 0.5 * g.kzr * h / k.beta2;
      const double var = xi * tc * (1.0 - k.beta2 * tc / (2.0 * k.tmax));
      const double z0 = sqrt(-2.0 * log(gen_u(x0[0]))) * cos(GEN_TWO_PI * gen_u(x0[1]));
      dE = fmax(dE + sqrt(var) * z0, 0.0);
      if (k.tmax > g.t_cut) {
        uint32_t x1[4];
        keyed_block(seed, RNG_TAG_GEN, w.key, blk + 1, x1);
        const double lam = xi * ((1.0 / g.t_cut - 1.0 / k.tmax) - (k.beta2 / k.tmax) * log(k.tmax / g.t_cut));
        const double up = gen_u(x1[0]) - 2.98023223876953125e-08;      // 2^-25
        double pk = exp(-lam), c = pk;
        int nh = 0;
        for (int q = 1; q <= LDSIM_TRACK_GEN_HARD_CAP; q++) {
          if (!(up > c)) break;
          nh = q;
          pk = pk * lam / (double)q;
          c = c + pk;
        }
        for (int j = 0; j < nh; j++) {
          uint32_t xj[4];
          double th = 0.0;
          for (int r = 0; r < LDSIM_TRACK_GEN_HARD_TRIES; r++) {
            if ((r & 1) == 0) keyed_block(seed, RNG_TAG_GEN, w.key, blk + 2 + 2 * j + (r >> 1), xj);
            const double ue = gen_u((r & 1) ? xj[2] : xj[0]), ua = gen_u((r & 1) ? xj[3] : xj[1]);
            th = 1.0 / (1.0 / g.t_cut - ue * (1.0 / g.t_cut - 1.0 / k.tmax));
            if (ua > k.beta2 * th / k.tmax || r == LDSIM_TRACK_GEN_HARD_TRIES - 1) break;
          }
          dE = dE + th;
        }
      }
    }
    stops = dE >= w.T || w.T - dE < g.t_min;
    if (stops) {
      dE = w.T;
      h = fmin(h, w.T / s_mean);
    }
  }
  leaves = leaves && !stops;
  const double E = Tm + w.M;
  const double beta = sqrt(k.beta2);
  double ex = w.px + h * w.dx, ey = w.py + h * w.dy, ez = w.pz + h * w.dz;
  if (leaves) {
    // (runtime-indexed registers would go to scratch: select the components instead)
    const double on = far ? (axis == 0 ? g.hi[0] : axis == 1 ? g.hi[1] : g.hi[2]) : (axis == 0 ? g.lo[0] : axis == 1 ? g.lo[1] : g.lo[2]);
    if (axis == 0) ex = on; else if (axis == 1) ey = on; else ez = on;
  }
  ex = fmin(fmax(ex, g.lo[0]), g.hi[0]);
  ey = fmin(fmax(ey, g.lo[1]), g.hi[1]);
  ez = fmin(fmax(ez, g.lo[2]), g.hi[2]);
  const double t1 = w.t + h / (beta * GEN_C_LIGHT);
  sg.xs = w.px; sg.ys = w.py; sg.zs = w.pz;
  sg.xe = ex; sg.ye = ey; sg.ze = ez;
  sg.h = h;
  sg.dE = dE;
  sg.t0 = w.t;
  sg.t1 = t1;
  w.step++;
  if (stops) w.state = 0;
  else if (leaves) w.state = 1;
  else if (w.step >= g.max_steps) w.state = 2;
  if (g.mcs && w.state == GEN_WALKING) {
    const double th0 = 13.6 / (k.beta2 * E) * sqrt(h / g.x0cm) * fmax(1.0 + 0.038 * log(h / (g.x0cm * k.beta2)), 0.0);
    const double rr = sqrt(-2.0 * log(gen_u(x0[2]))), aa = GEN_TWO_PI * gen_u(x0[3]);
    const double ax = th0 * (rr * cos(aa)), ay = th0 * (rr * sin(aa));
    const double nrm = sqrt(1.0 + ax * ax + ay * ay);
    const double a = ax / nrm, b = ay / nrm, mu = 1.0 / nrm;
    // the light LUT builder's rotation; where d is within 0.99999 of the z axis its polar shortcut (which replaces d by the local
    // vector: right for a photon's wide angles, wrong for milliradians) gives way to the same rotation about the x axis, by a
    // cyclic permutation of the components
    const bool polar = fabs(w.dz) > 0.99999;
    const double dx = polar ? w.dy : w.dx, dy = polar ? w.dz : w.dy, dz = polar ? w.dx : w.dz;
    const double den = sqrt(1.0 - dz * dz);
    const double rx = (dx * dz * a - dy * b) / den + dx * mu;
    const double ry = (dy * dz * a + dx * b) / den + dy * mu;
    const double rz = -a * den + dz * mu;
    const double nx = polar ? rz : rx, ny = polar ? rx : ry, nz = polar ? ry : rz;
    const double nn = sqrt(nx * nx + ny * ny + nz * nz);
    w.dx = nx / nn;
    w.dy = ny / nn;
    w.dz = nz / nn;
  }
  w.px = ex; w.py = ey; w.pz = ez;
  w.t = t1;
  w.T = w.T - dE;
  w.path = w.path + h;
}

__device__ inline void gen_start(const LdsimTrackGenPrimary& P, GenWalk& w) {
  const double n = sqrt(P.dir[0] * P.dir[0] + P.dir[1] * P.dir[1] + P.dir[2] * P.dir[2]);
  w.px = P.pos[0]; w.py = P.pos[1]; w.pz = P.pos[2];
  w.dx = P.dir[0] / n; w.dy = P.dir[1] / n; w.dz = P.dir[2] / n;
  w.T = P.kinetic_energy;
  w.t = P.time;
  w.path = 0.0;
  w.M = gen_mass(P.pdg);
  w.key = key_mix(key_mix(RNG_KEY_ROOT, (uint64_t)(int64_t)P.event_id), (uint64_t)(int64_t)P.track_in_event);
  w.step = 0;
  w.state = GEN_WALKING;
  w.pdg = P.pdg;
  w.event = P.event_id;
}

// WRITE = false: counts u64 [n], state i32 [n], end f64 [n][6] (end point, end time, path, remaining T).
// WRITE = true: segment (i, s) into column element offsets[i] + s (< cap, checked) of fcol [NF64][cap] and icol [NI32][cap].
template <bool WRITE>
__global__ void __launch_bounds__(GEN_BLOCK)
gen_kernel(const GenConst g, const LdsimTrackGenPrimary* __restrict__ prim, int64_t n, uint64_t seed, int32_t group,
           unsigned long long* __restrict__ counts, int32_t* __restrict__ state, double* __restrict__ end,
           const unsigned long long* __restrict__ offsets, int64_t cap, double* __restrict__ fcol, int32_t* __restrict__ icol) {
  __shared__ unsigned next;
  const int64_t first = (int64_t)blockIdx.x * group;
  const unsigned mine = (unsigned)min((int64_t)group, n - first);
  if (threadIdx.x == 0) next = 0;
  __syncthreads();
  GenWalk w;
  GenSeg sg;
  int64_t idx = 0;
  unsigned long long off = 0;
  bool have = false;
  while (true) {
    if (!have) {
      const unsigned i = atomicAdd(&next, 1u);
      if (i >= mine) break;
      idx = first + i;
      gen_start(prim[idx], w);
      if (WRITE) off = offsets[idx];
      have = true;
    }
    gen_step(g, seed, w, sg);
    if (WRITE) {
      const unsigned long long o = off + (unsigned)(w.step - 1);
      if (o < (unsigned long long)cap) {
        double* f = fcol + o;
        const size_t c = (size_t)cap;
        f[0 * c] = sg.xs; f[1 * c] = sg.ys; f[2 * c] = sg.zs;
        f[3 * c] = sg.xe; f[4 * c] = sg.ye; f[5 * c] = sg.ze;
        f[6 * c] = 0.5 * (sg.xs + sg.xe); f[7 * c] = 0.5 * (sg.ys + sg.ye); f[8 * c] = 0.5 * (sg.zs + sg.ze);
        f[9 * c] = sg.h;
        f[10 * c] = sg.dE;
        f[11 * c] = sg.h > 0 ? sg.dE / sg.h : 0.0;
        f[12 * c] = sg.t0; f[13 * c] = sg.t1; f[14 * c] = 0.5 * (sg.t0 + sg.t1);
        int32_t* q = icol + o;
        q[0 * c] = (int32_t)idx; q[1 * c] = w.step - 1; q[2 * c] = w.pdg; q[3 * c] = w.event;
      }
    }
    if (w.state != GEN_WALKING) {
      have = false;
      if (!WRITE) {
        counts[idx] = (unsigned long long)w.step;
        state[idx] = w.state;
        double* e = end + 6 * idx;
        e[0] = w.px; e[1] = w.py; e[2] = w.pz; e[3] = w.t; e[4] = w.path; e[5] = w.T;
      }
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
#define GEN_NEED(cond, ...)               \
  do {                                    \
    if (!(cond)) {                        \
      ldsim_set_error(__VA_ARGS__);       \
      return LDSIM_EINVAL;                \
    }                                     \
  } while (0)

static inline bool gen_pos(double v) { return std::isfinite(v) && v > 0; }

static uint64_t gen_hash(uint64_t h, const void* data, size_t bytes) {      // (bytes: a multiple of 8)
  const uint64_t* q = (const uint64_t*)data;
  for (size_t i = 0; i < bytes / 8; i++) h = (h ^ q[i]) * 0x100000001B3ULL + (h >> 29);
  return h;
}

// checks parameters and primaries, fills the kernel's constants
static int gen_prepare(const char* who, const LdsimTrackGenParams* P, const LdsimTrackGenPrimary* prim, int64_t n, GenConst* g) {
  GEN_NEED(P && (n == 0 || prim), "%s: null argument", who);
  GEN_NEED(n >= 0 && n <= 2147483647LL, "%s: %lld primaries, need 0 .. 2^31 - 1", who, (long long)n);
  GEN_NEED(gen_pos(P->step), "%s: step %g cm must be finite and > 0", who, P->step);
  GEN_NEED(gen_pos(P->min_step), "%s: min_step %g cm must be finite and > 0", who, P->min_step);
  GEN_NEED(P->min_step <= P->step, "%s: min_step %g exceeds step %g", who, P->min_step, P->step);
  GEN_NEED(gen_pos(P->max_loss_fraction) && P->max_loss_fraction <= 1, "%s: max_loss_fraction %g must lie in (0, 1]", who,
           P->max_loss_fraction);
  GEN_NEED(gen_pos(P->t_cut), "%s: t_cut %g MeV must be finite and > 0", who, P->t_cut);
  GEN_NEED(gen_pos(P->t_min), "%s: t_min %g MeV must be finite and > 0", who, P->t_min);
  GEN_NEED(gen_pos(P->density) && gen_pos(P->z_over_a) && gen_pos(P->mean_excitation) && gen_pos(P->rad_length) && gen_pos(P->k_coeff),
           "%s: density, z_over_a, mean_excitation, rad_length and k_coeff must be finite and > 0", who);
  GEN_NEED(P->t_cut > P->mean_excitation, "%s: t_cut %g MeV must exceed the mean excitation energy %g MeV", who, P->t_cut,
           P->mean_excitation);
  for (int k = 0; k < 6; k++) GEN_NEED(std::isfinite(P->sternheimer[k]), "%s: sternheimer[%d] is not finite", who, k);
  for (int k = 0; k < 3; k++)
    GEN_NEED(std::isfinite(P->world_lo[k]) && std::isfinite(P->world_hi[k]) && P->world_lo[k] < P->world_hi[k],
             "%s: the world box is empty or inverted along axis %d: [%g, %g]", who, k, P->world_lo[k], P->world_hi[k]);
  GEN_NEED(P->max_steps >= 1 && P->max_steps <= LDSIM_TRACK_GEN_MAX_STEPS, "%s: max_steps %d, need 1 .. %d", who, P->max_steps,
           LDSIM_TRACK_GEN_MAX_STEPS);
  for (int k = 0; k < 3; k++) {
    g->lo[k] = P->world_lo[k];
    g->hi[k] = P->world_hi[k];
  }
  g->step = P->step;
  g->min_step = P->min_step;
  g->frac = P->max_loss_fraction;
  g->t_cut = P->t_cut;
  g->t_min = P->t_min;
  g->kzr = P->k_coeff * P->z_over_a * P->density;
  g->i2 = P->mean_excitation * P->mean_excitation;
  g->x0cm = P->rad_length / P->density;
  g->sa = P->sternheimer[0]; g->sk = P->sternheimer[1]; g->sx0 = P->sternheimer[2];
  g->sx1 = P->sternheimer[3]; g->scbar = P->sternheimer[4]; g->sd0 = P->sternheimer[5];
  g->straggling = P->straggling != 0;
  g->mcs = P->mcs != 0;
  g->eloss = P->energy_loss != 0;
  g->max_steps = P->max_steps;
  static const int32_t kinds[3] = {13, 211, 2212};
  for (int32_t pdg : kinds) {
    const GenKin k = gen_kin(P->t_min, gen_mass(pdg));
    GEN_NEED(gen_rate(*g, k, fmin(P->t_cut, k.tmax)) > 0, "%s: the stopping power of pdg %d is not positive at t_min %g MeV: raise "
             "t_min", who, pdg, P->t_min);
  }
  for (int64_t i = 0; i < n; i++) {
    const LdsimTrackGenPrimary& r = prim[i];
    GEN_NEED(r.pdg == 13 || r.pdg == -13 || r.pdg == 211 || r.pdg == -211 || r.pdg == 2212,
             "%s: primary %lld has unknown pdg %d (13, -13, 211, -211 and 2212 are transported)", who, (long long)i, r.pdg);
    GEN_NEED(gen_pos(r.kinetic_energy), "%s: primary %lld: kinetic energy %g MeV must be finite and > 0", who, (long long)i,
             r.kinetic_energy);
    for (int k = 0; k < 3; k++)
      GEN_NEED(std::isfinite(r.pos[k]) && r.pos[k] >= P->world_lo[k] && r.pos[k] <= P->world_hi[k],
               "%s: primary %lld starts outside the world box (coordinate %d = %g, box [%g, %g])", who, (long long)i, k, r.pos[k],
               P->world_lo[k], P->world_hi[k]);
    const double nn = sqrt(r.dir[0] * r.dir[0] + r.dir[1] * r.dir[1] + r.dir[2] * r.dir[2]);
    GEN_NEED(std::isfinite(nn) && nn > 0, "%s: primary %lld has a zero direction", who, (long long)i);
    GEN_NEED(std::isfinite(r.time), "%s: primary %lld: time is not finite", who, (long long)i);
  }
  return 0;
}

// primaries per workgroup: the option, or by itself (0) enough groups to spread a short list over the device -- n / 2048, at
// least 64 (one wave's worth) and at most 1024 (four primaries per lane, so that lanes take over from one another)
static int32_t gen_group(const ldsim_ctx* ctx, int64_t n) {
  if (ctx->tg_group > 0) return ctx->tg_group;
  const int64_t g = (n + 2047) / 2048;
  return (int32_t)(g < 64 ? 64 : g > 1024 ? 1024 : g);
}

// the count pass and the scan; leaves counts / states / end rows / offsets in the ctx and the total in ctx->tg_total.  Skipped when
// the ctx holds them for the same (parameters, primaries, seed) already.
static int gen_count_pass(ldsim_ctx* ctx, const char* who, const GenConst& g, const LdsimTrackGenParams* P,
                          const LdsimTrackGenPrimary* prim, int64_t n, uint64_t seed) {
  uint64_t h = gen_hash(0xCBF29CE484222325ULL ^ seed, P, sizeof(*P));
  h = gen_hash(h ^ (uint64_t)n, prim, (size_t)n * sizeof(*prim));
  if (ctx->tg_valid && ctx->tg_hash == h && ctx->tg_n == n) return 0;
  ctx->tg_valid = 0;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  CK(ctx->tg_prim.ensure((size_t)n * sizeof(*prim)));
  CK(ctx->tg_counts.ensure((size_t)n * 8));
  CK(ctx->tg_off.ensure((size_t)n * 8));
  CK(ctx->tg_state.ensure((size_t)n * 4));
  CK(ctx->tg_end.ensure((size_t)n * 48));
  ctx->tg_total = 0;
  if (n) {
    HIPCHK(hipMemcpyAsync(ctx->tg_prim.p, prim, (size_t)n * sizeof(*prim), hipMemcpyHostToDevice, st));
    const int32_t group = gen_group(ctx, n);
    const unsigned blocks = (unsigned)((n + group - 1) / group);
    hipLaunchKernelGGL(gen_kernel<false>, dim3(blocks), dim3(GEN_BLOCK), 0, st, g, ctx->tg_prim.as<LdsimTrackGenPrimary>(), n, seed,
                       group, ctx->tg_counts.as<unsigned long long>(), ctx->tg_state.as<int32_t>(), ctx->tg_end.as<double>(),
                       (const unsigned long long*)nullptr, (int64_t)0, (double*)nullptr, (int32_t*)nullptr);
    HIPCHK(hipGetLastError());
    CK(sort_exclusive_scan_u64(ctx, ctx->tg_counts.as<unsigned long long>(), ctx->tg_off.as<unsigned long long>(), n));
    unsigned long long last[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&last[0], ctx->tg_counts.as<unsigned long long>() + (n - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&last[1], ctx->tg_off.as<unsigned long long>() + (n - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ctx->tg_total = (int64_t)(last[0] + last[1]);
  }
  ctx->tg_hash = h;
  ctx->tg_n = n;
  ctx->tg_valid = 1;
  return 0;
}

int trackgen_count(ldsim_ctx* ctx, const LdsimTrackGenParams* P, const LdsimTrackGenPrimary* prim, int64_t n, uint64_t seed,
                   int32_t* counts, int32_t* end_state, double* end) {
  static const char who[] = "ldsim_track_gen_count";
  GenConst g;
  CK(gen_prepare(who, P, prim, n, &g));
  if (n == 0) return 0;
  GEN_NEED(counts && end_state && end, "%s: null output array", who);
  CK(gen_count_pass(ctx, who, g, P, prim, n, seed));
  std::vector<unsigned long long> c64((size_t)n);
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(c64.data(), ctx->tg_counts.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(end_state, ctx->tg_state.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(end, ctx->tg_end.p, (size_t)n * 48, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; i++) counts[i] = (int32_t)c64[(size_t)i];      // (<= LDSIM_TRACK_GEN_MAX_STEPS each)
  return 0;
}

int trackgen_generate(ldsim_ctx* ctx, const LdsimTrackGenParams* P, const LdsimTrackGenPrimary* prim, int64_t n, uint64_t seed,
                      int64_t capacity, double* f64_columns, int32_t* i32_columns, int64_t* n_segments) {
  static const char who[] = "ldsim_track_gen";
  GenConst g;
  CK(gen_prepare(who, P, prim, n, &g));
  GEN_NEED(n_segments, "%s: null n_segments", who);
  GEN_NEED(capacity >= 0, "%s: negative capacity", who);
  *n_segments = 0;
  ctx->ms_tg = 0;
  if (n == 0) return 0;
  CK(gen_count_pass(ctx, who, g, P, prim, n, seed));
  const int64_t total = ctx->tg_total;
  GEN_NEED(total <= 2147483647LL, "%s: %lld segments, more than 2^31 - 1: walk fewer primaries per call", who, (long long)total);
  GEN_NEED(capacity >= total, "%s: capacity %lld is too small: %lld segments are needed", who, (long long)capacity, (long long)total);
  GEN_NEED(f64_columns && i32_columns, "%s: null output array", who);
  hipStream_t st = ctx->stream;
  CK(ctx->tg_f64.ensure((size_t)total * 8 * LDSIM_TRACK_GEN_NF64));
  CK(ctx->tg_i32.ensure((size_t)total * 4 * LDSIM_TRACK_GEN_NI32));
  for (Event& e : ctx->tg_ev) CK(e.ensure());
  const int32_t group = gen_group(ctx, n);
  const unsigned blocks = (unsigned)((n + group - 1) / group);
  HIPCHK(hipEventRecord(ctx->tg_ev[0], st));
  hipLaunchKernelGGL(gen_kernel<true>, dim3(blocks), dim3(GEN_BLOCK), 0, st, g, ctx->tg_prim.as<LdsimTrackGenPrimary>(), n, seed, group,
                     (unsigned long long*)nullptr, (int32_t*)nullptr, (double*)nullptr, ctx->tg_off.as<unsigned long long>(), total,
                     ctx->tg_f64.as<double>(), ctx->tg_i32.as<int32_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->tg_ev[1], st));
  for (int c = 0; c < LDSIM_TRACK_GEN_NF64; c++)
    HIPCHK(hipMemcpyAsync(f64_columns + (size_t)c * capacity, ctx->tg_f64.as<double>() + (size_t)c * total, (size_t)total * 8,
                          hipMemcpyDeviceToHost, st));
  for (int c = 0; c < LDSIM_TRACK_GEN_NI32; c++)
    HIPCHK(hipMemcpyAsync(i32_columns + (size_t)c * capacity, ctx->tg_i32.as<int32_t>() + (size_t)c * total, (size_t)total * 4,
                          hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->tg_ev[0], ctx->tg_ev[1]));
  ctx->ms_tg = ms;
  *n_segments = total;
  return 0;
}
