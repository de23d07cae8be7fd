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
//
// The cascade (ldsim_track_cascade_count, ldsim_track_cascade; larndsim_amd/track_cascade.py): gen_step<true> is the same step for
// electrons too (Moller loss and collisions) and hands hard collisions above t_track to an emitter instead of the segment;
// cas_kernel<WRITE> is gen_kernel's loop over LdsimTrackGenParticle records that also counts / stores the secondaries of every
// walk (delta rays in the order (step, collision), the decay electron of a stopped muon last) at soffset[particle] + running
// index.  One call walks one generation; the host loops.  gen_step<false> is the step gen_kernel has always made.
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

// the cascade's switches (LdsimTrackGenCascadeParams; delta and decays are 0 in a last generation, emit = 0)
struct CasConst {
  double t_track, tau_plus, tau_minus, capture;
  int32_t delta, decays;
};

// where a walk's secondaries go: out = the walk's first record (nullptr in the count pass), room = records that fit behind it
struct GenEmit {
  LdsimTrackGenParticle* out;
  unsigned long long room;
  unsigned n;                         // emitted so far
  int32_t parent, generation, tie;    // the walking particle's index, generation and track_in_event
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

// electrons (include/ldsim.h, "Electrons"): MeV / cm lost to Moller collisions below tc (tc = T / 2: the unrestricted ICRU-37 mean)
__host__ __device__ inline double gen_rate_e(const GenConst& g, const GenKin& k, double T, double tc) {
  const double tau = T / LDSIM_TRACK_GEN_ME, d = fmin(tc, 0.5 * T) / LDSIM_TRACK_GEN_ME;
  const double e2 = g.i2 / (LDSIM_TRACK_GEN_ME * LDSIM_TRACK_GEN_ME);
  return 0.5 * g.kzr / k.beta2 *
         (log(2.0 * (tau + 2.0) / e2) - 1.0 - k.beta2 + log((tau - d) * d) + tau / (tau - d) +
          (0.5 * d * d + (2.0 * tau + 1.0) * log(1.0 - d / tau)) / (k.gamma * k.gamma) - gen_delta(g, k.bg2));
}

// Moller collisions above t_cut per unit of xi = (K / 2)(Z/A) rho h / beta^2, at kinetic energy T > 2 t_cut
__host__ __device__ inline double gen_lambda_e(const GenKin& k, double T, double t_cut) {
  const double gm = (2.0 * k.gamma - 1.0) / (k.gamma * k.gamma), x0 = t_cut / T, x1 = 0.5;
  return ((x1 - x0) * (1.0 - gm + 1.0 / (x0 * x1) + 1.0 / ((1.0 - x0) * (1.0 - x1))) - gm * log(x1 * (1.0 - x0) / (x0 * (1.0 - x1)))) / T;
}

// Moller's shape over the proposal 1 / x^2 + 1 / (1 - x)^2, as a function of x (1 - x): falls, then rises (largest at an end)
__host__ __device__ inline double gen_moller_ratio(double gm, double x) {
  const double y = x * (1.0 - x);
  return 1.0 + ((1.0 - gm) * y * y - gm * y) / (1.0 - 2.0 * y);
}

__host__ __device__ inline double cas_mass(int32_t pdg) {
  const int32_t a = pdg < 0 ? -pdg : pdg;
  return a == 11 ? LDSIM_TRACK_GEN_ME : gen_mass(pdg);
}

// the local direction (a, b, mu) turned into the frame of the unit vector w and renormalised: the light LUT builder's rotation;
// where w is within 0.99999 of the z axis its polar shortcut (which replaces w by the local vector: right for a photon's wide
// angles, wrong for milliradians) gives way to the same rotation about the x axis, by a cyclic permutation of the components
__host__ __device__ inline void gen_rotate(double wx, double wy, double wz, double a, double b, double mu, double& ox, double& oy,
                                           double& oz) {
  const bool polar = fabs(wz) > 0.99999;
  const double dx = polar ? wy : wx, dy = polar ? wz : wy, dz = polar ? wx : wz;
  const double den = sqrt(1.0 - dz * dz);
  const double rx = (dx * dz * a - dy * b) / den + dx * mu;
  const double ry = (dy * dz * a + dx * b) / den + dy * mu;
  const double rz = -a * den + dz * mu;
  const double nx = polar ? rz : rx, ny = polar ? rx : ry, nz = polar ? ry : rz;
  const double nn = sqrt(nx * nx + ny * ny + nz * nz);
  ox = nx / nn;
  oy = ny / nn;
  oz = nz / nn;
}

__device__ inline double gen_u(uint32_t x) { return (double)keyed_u01(x); }

// draw i of the step whose first block is blk
__device__ inline double cas_u(uint64_t seed, uint64_t key, uint32_t blk, int i) {
  uint32_t x[4];
  keyed_block(seed, RNG_TAG_GEN, key, blk + (uint32_t)(i >> 2), x);
  const int q = i & 3;
  return gen_u(q == 0 ? x[0] : q == 1 ? x[1] : q == 2 ? x[2] : x[3]);
}

// a delta ray of kinetic energy th from collision j of the step that starts at w (Tm: the parent's midpoint energy).  The
// record's pos[0] holds the draw u of its place on the segment until gen_step knows the segment's final length.
__device__ inline void cas_emit_delta(uint64_t seed, const GenWalk& w, double Tm, double th, int j, uint32_t blk, GenEmit& em) {
  if (em.out && em.n < em.room) {
    const double E = Tm + w.M, p = sqrt(Tm * (Tm + 2.0 * w.M)), pe = sqrt(th * (th + 2.0 * LDSIM_TRACK_GEN_ME));
    const double ct = fmin(th * (E + LDSIM_TRACK_GEN_ME) / (p * pe), 1.0);
    const double st = sqrt(1.0 - ct * ct), phi = GEN_TWO_PI * cas_u(seed, w.key, blk, LDSIM_TRACK_GEN_DRAW_AZIMUTH + j);
    LdsimTrackGenParticle& r = em.out[em.n];
    gen_rotate(w.dx, w.dy, w.dz, st * cos(phi), st * sin(phi), ct, r.dir[0], r.dir[1], r.dir[2]);
    r.pos[0] = cas_u(seed, w.key, blk, LDSIM_TRACK_GEN_DRAW_PLACE + j);
    r.kinetic_energy = th;
    r.pdg = 11;
    r.event_id = w.event;
    r.track_in_event = em.tie;
    r._pad = 0;
    r.key = key_mix(key_mix(w.key, (uint64_t)(1 + w.step)), (uint64_t)(1 + j));
    r.parent = em.parent;
    r.generation = em.generation + 1;
    r.process = 1;
    r.parent_step = w.step;
  }
  em.n++;
}

// one step of the walk (include/ldsim.h, "One step"); sets w.state when the walk ends
// CAS: electrons too, and hard collisions above cg->t_track leave as secondaries through em (cg, em: nullptr without CAS)
template <bool CAS>
__device__ inline void gen_step(const GenConst& g, const CasConst* cg, uint64_t seed, GenWalk& w, GenSeg& sg, GenEmit* em) {
  const uint32_t blk = (uint32_t)LDSIM_TRACK_GEN_STEP_BLOCKS * (uint32_t)w.step;
  GenKin k = gen_kin(w.T, w.M);
  bool el = false;
  double eem = 0.0;                   // energy that left as secondaries
  unsigned em0 = 0;
  if constexpr (CAS) {
    el = w.pdg == 11 || w.pdg == -11;
    if (el) k.tmax = 0.5 * w.T;
    em0 = em->n;
  }
  double s_full = gen_rate(g, k, k.tmax);
  if constexpr (CAS) s_full = el ? gen_rate_e(g, k, w.T, k.tmax) : s_full;
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
    if constexpr (CAS) if (el) k.tmax = 0.5 * Tm;
    const double tc = g.straggling ? fmin(g.t_cut, k.tmax) : k.tmax;
    double s_mean = gen_rate(g, k, tc);
    if constexpr (CAS) s_mean = el ? gen_rate_e(g, k, Tm, tc) : s_mean;
    dE = s_mean * h;
    if (g.straggling) {
      const double xi = 0.5 * g.kzr * h / k.beta2;
      const double var = xi * tc * (1.0 - k.beta2 * tc / (2.0 * k.tmax));
      const double z0 = sqrt(-2.0 * log(gen_u(x0[0]))) * cos(GEN_TWO_PI * gen_u(x0[1]));
      dE = fmax(dE + sqrt(var) * z0, 0.0);
      if (k.tmax > g.t_cut) {
        uint32_t x1[4];
        keyed_block(seed, RNG_TAG_GEN, w.key, blk + 1, x1);
        double lam = xi * ((1.0 / g.t_cut - 1.0 / k.tmax) - (k.beta2 / k.tmax) * log(k.tmax / g.t_cut));
        if constexpr (CAS) lam = el ? xi * gen_lambda_e(k, Tm, g.t_cut) : lam;
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
          if (CAS && el) {
            // Moller: x = T_h / Tm on [x0, 1/2] from the proposal 1 / x^2 + 1 / (1 - x)^2 by its quadratic, kept with
            // probability ratio / (the ratio's larger end value); the last try is kept whatever u_a says (and draws none)
            const double gm = (2.0 * k.gamma - 1.0) / (k.gamma * k.gamma), xl = g.t_cut / Tm;
            const double g0 = (2.0 * xl - 1.0) / (xl * (1.0 - xl));
            const double top = fmax(gen_moller_ratio(gm, xl), gen_moller_ratio(gm, 0.5));
            for (int r = 0; r < LDSIM_TRACK_GEN_MOLLER_TRIES; r++) {
              const int i = r < LDSIM_TRACK_GEN_HARD_TRIES ? 8 + 8 * j + 2 * r
                                                          : LDSIM_TRACK_GEN_DRAW_MOLLER + 5 * j + 2 * (r - LDSIM_TRACK_GEN_HARD_TRIES);
              const double c = g0 * (1.0 - cas_u(seed, w.key, blk, i));
              const double x = 2.0 / ((2.0 - c) + sqrt(4.0 + c * c));
              th = x * Tm;
              if (r == LDSIM_TRACK_GEN_MOLLER_TRIES - 1) break;
              if (cas_u(seed, w.key, blk, i + 1) * top <= gen_moller_ratio(gm, x)) break;
            }
          } else {
            for (int r = 0; r < LDSIM_TRACK_GEN_HARD_TRIES; r++) {
              if ((r & 1) == 0) keyed_block(seed, RNG_TAG_GEN, w.key, blk + 2 + 2 * j + (r >> 1), xj);
              const double ue = gen_u((r & 1) ? xj[2] : xj[0]), ua = gen_u((r & 1) ? xj[3] : xj[1]);
              th = 1.0 / (1.0 / g.t_cut - ue * (1.0 / g.t_cut - 1.0 / k.tmax));
              if (ua > k.beta2 * th / k.tmax || r == LDSIM_TRACK_GEN_HARD_TRIES - 1) break;
            }
          }
          // a secondary of its own from t_track on, while what has left stays below T (else deposited, in the order j)
          bool leaves_track = false;
          if constexpr (CAS) leaves_track = cg->delta && th >= cg->t_track && eem + th < w.T;
          if (leaves_track) {
            eem = eem + th;
            cas_emit_delta(seed, w, Tm, th, j, blk, *em);
          } else {
            dE = dE + th;
          }
        }
      }
    }
    double spent = dE;
    if constexpr (CAS) spent = dE + eem;
    stops = spent >= w.T || w.T - spent < g.t_min;
    if (stops) {
      dE = w.T;
      if constexpr (CAS) dE = w.T - eem;
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
  if constexpr (CAS) {
    // the secondaries' places on the segment as it ended: p + u h d (held in the box), the time interpolated
    if (em->out)
      for (unsigned q = em0; q < em->n && q < em->room; q++) {
        LdsimTrackGenParticle& r = em->out[q];
        const double u = r.pos[0];
        r.pos[0] = fmin(fmax(w.px + u * h * w.dx, g.lo[0]), g.hi[0]);
        r.pos[1] = fmin(fmax(w.py + u * h * w.dy, g.lo[1]), g.hi[1]);
        r.pos[2] = fmin(fmax(w.pz + u * h * w.dz, g.lo[2]), g.hi[2]);
        r.time = w.t + u * (t1 - w.t);
      }
  }
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
    gen_rotate(w.dx, w.dy, w.dz, a, b, mu, w.dx, w.dy, w.dz);
  }
  w.px = ex; w.py = ey; w.pz = ez;
  w.t = t1;
  w.T = w.T - dE;
  if constexpr (CAS) w.T = stops ? 0.0 : w.T - eem;
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
    gen_step<false>(g, nullptr, seed, w, sg, nullptr);
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

__device__ inline void cas_start(const LdsimTrackGenParticle& P, GenWalk& w) {
  const double n = sqrt(P.dir[0] * P.dir[0] + P.dir[1] * P.dir[1] + P.dir[2] * P.dir[2]);
  w.px = P.pos[0]; w.py = P.pos[1]; w.pz = P.pos[2];
  w.dx = P.dir[0] / n; w.dy = P.dir[1] / n; w.dz = P.dir[2] / n;
  w.T = P.kinetic_energy;
  w.t = P.time;
  w.path = 0.0;
  w.M = cas_mass(P.pdg);
  w.key = P.key;
  w.step = 0;
  w.state = GEN_WALKING;
  w.pdg = P.pdg;
  w.event = P.event_id;
}

// a muon that stopped (include/ldsim.h, "Decay"): draws of the step index after its last, w.step
__device__ inline void cas_decay(const CasConst& cg, uint64_t seed, const GenWalk& w, GenEmit& em) {
  const uint32_t blk = (uint32_t)LDSIM_TRACK_GEN_STEP_BLOCKS * (uint32_t)w.step;
  uint32_t x0[4], xr[4];
  keyed_block(seed, RNG_TAG_GEN, w.key, blk, x0);
  const bool minus = w.pdg == 13;
  if (minus && gen_u(x0[0]) <= cg.capture) return;
  // the Michel x: F(x) = x^3 (2 - x) = u by Newton from cbrt(u / 2) (F is convex and rising: from the second iterate on the
  // sequence falls onto the root)
  keyed_block(seed, RNG_TAG_GEN, w.key, blk + 1, xr);
  const double u = gen_u(xr[0]);
  double x = cbrt(0.5 * u);
  for (int r = 0; r < LDSIM_TRACK_GEN_MICHEL_NEWTON; r++) x = x - (x * x * x * (2.0 - x) - u) / (2.0 * x * x * (3.0 - 2.0 * x));
  x = fmin(x, 1.0);
  const double wmax = (LDSIM_TRACK_GEN_M_MUON * LDSIM_TRACK_GEN_M_MUON + LDSIM_TRACK_GEN_ME * LDSIM_TRACK_GEN_ME) / (2.0 * LDSIM_TRACK_GEN_M_MUON);
  const double etot = x * wmax;
  if (etot <= LDSIM_TRACK_GEN_ME) return;
  if (em.out && em.n < em.room) {
    const double mu = 1.0 - 2.0 * gen_u(x0[2]), phi = GEN_TWO_PI * gen_u(x0[3]);
    const double st = sqrt(fmax(0.0, 1.0 - mu * mu));
    LdsimTrackGenParticle& r = em.out[em.n];
    r.pos[0] = w.px; r.pos[1] = w.py; r.pos[2] = w.pz;
    r.dir[0] = st * cos(phi); r.dir[1] = st * sin(phi); r.dir[2] = mu;
    r.kinetic_energy = etot - LDSIM_TRACK_GEN_ME;
    r.time = w.t - (minus ? cg.tau_minus : cg.tau_plus) * log(gen_u(x0[1]));
    r.pdg = minus ? 11 : -11;
    r.event_id = w.event;
    r.track_in_event = em.tie;
    r._pad = 0;
    r.key = key_mix(key_mix(w.key, (uint64_t)(1 + w.step)), (uint64_t)LDSIM_TRACK_GEN_DECAY_KEY);
    r.parent = em.parent;
    r.generation = em.generation + 1;
    r.process = 2;
    r.parent_step = w.step;
  }
  em.n++;
}

// gen_kernel's loop over one generation of a cascade.  WRITE = false: counts and scounts u64 [n] (segments, secondaries), state,
// end as gen_kernel.  WRITE = true: segments as gen_kernel; secondary q of particle i into sec[soffsets[i] + q] (< scap, checked).
template <bool WRITE>
__global__ void __launch_bounds__(GEN_BLOCK)
cas_kernel(const GenConst g, const CasConst cg, const LdsimTrackGenParticle* __restrict__ part, int64_t n, uint64_t seed, int32_t group,
           unsigned long long* __restrict__ counts, unsigned long long* __restrict__ scounts, int32_t* __restrict__ state,
           double* __restrict__ end, const unsigned long long* __restrict__ offsets, const unsigned long long* __restrict__ soffsets,
           int64_t cap, int64_t scap, double* __restrict__ fcol, int32_t* __restrict__ icol, LdsimTrackGenParticle* __restrict__ sec) {
  __shared__ unsigned next;
  const int64_t first = (int64_t)blockIdx.x * group;
  const unsigned mine = (unsigned)min((int64_t)group, n - first);
  if (threadIdx.x == 0) next = 0;
  __syncthreads();
  GenWalk w;
  GenSeg sg;
  GenEmit em;
  int64_t idx = 0;
  unsigned long long off = 0;
  bool have = false;
  while (true) {
    if (!have) {
      const unsigned i = atomicAdd(&next, 1u);
      if (i >= mine) break;
      idx = first + i;
      cas_start(part[idx], w);
      em.out = nullptr;
      em.room = 0;
      em.n = 0;
      em.parent = (int32_t)idx;
      em.generation = part[idx].generation;
      em.tie = part[idx].track_in_event;
      if (WRITE) {
        off = offsets[idx];
        const unsigned long long so = soffsets[idx];
        em.room = so < (unsigned long long)scap ? (unsigned long long)scap - so : 0;
        em.out = sec + (so < (unsigned long long)scap ? so : 0);
      }
      have = true;
    }
    gen_step<true>(g, &cg, seed, w, sg, &em);
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
      if (w.state == 0 && cg.decays && (w.pdg == 13 || w.pdg == -13)) cas_decay(cg, seed, w, em);
      have = false;
      if (!WRITE) {
        counts[idx] = (unsigned long long)w.step;
        scounts[idx] = (unsigned long long)em.n;
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

// checks the parameters, fills the kernel's constants; electrons: the cascade's entries, which walk them
static int gen_prepare_params(const char* who, const LdsimTrackGenParams* P, GenConst* g, bool electrons) {
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
  if (electrons) {
    GenKin k = gen_kin(P->t_min, LDSIM_TRACK_GEN_ME);
    k.tmax = 0.5 * P->t_min;
    GEN_NEED(gen_rate_e(*g, k, P->t_min, fmin(P->t_cut, k.tmax)) > 0, "%s: the stopping power of pdg 11 is not positive at t_min %g "
             "MeV: raise t_min", who, P->t_min);
  }
  return 0;
}

// checks the records to walk (Rec: LdsimTrackGenPrimary, or LdsimTrackGenParticle with what = "particle" and electrons allowed)
template <class Rec>
static int gen_check_records(const char* who, const LdsimTrackGenParams* P, const Rec* prim, int64_t n, const char* what,
                             bool electrons) {
  for (int64_t i = 0; i < n; i++) {
    const Rec& r = prim[i];
    GEN_NEED(r.pdg == 13 || r.pdg == -13 || r.pdg == 211 || r.pdg == -211 || r.pdg == 2212 || (electrons && (r.pdg == 11 || r.pdg == -11)),
             "%s: %s %lld has unknown pdg %d (%s13, -13, 211, -211 and 2212 are transported)", who, what, (long long)i, r.pdg,
             electrons ? "11, -11, " : "");
    GEN_NEED(gen_pos(r.kinetic_energy), "%s: %s %lld: kinetic energy %g MeV must be finite and > 0", who, what, (long long)i,
             r.kinetic_energy);
    for (int k = 0; k < 3; k++)
      GEN_NEED(std::isfinite(r.pos[k]) && r.pos[k] >= P->world_lo[k] && r.pos[k] <= P->world_hi[k],
               "%s: %s %lld starts outside the world box (coordinate %d = %g, box [%g, %g])", who, what, (long long)i, k, r.pos[k],
               P->world_lo[k], P->world_hi[k]);
    const double nn = sqrt(r.dir[0] * r.dir[0] + r.dir[1] * r.dir[1] + r.dir[2] * r.dir[2]);
    GEN_NEED(std::isfinite(nn) && nn > 0, "%s: %s %lld has a zero direction", who, what, (long long)i);
    GEN_NEED(std::isfinite(r.time), "%s: %s %lld: time is not finite", who, what, (long long)i);
  }
  return 0;
}

// checks parameters and primaries, fills the kernel's constants
static int gen_prepare(const char* who, const LdsimTrackGenParams* P, const LdsimTrackGenPrimary* prim, int64_t n, GenConst* g) {
  GEN_NEED(P && (n == 0 || prim), "%s: null argument", who);
  GEN_NEED(n >= 0 && n <= 2147483647LL, "%s: %lld primaries, need 0 .. 2^31 - 1", who, (long long)n);
  CK(gen_prepare_params(who, P, g, false));
  return gen_check_records(who, P, prim, n, "primary", false);
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

// ---- the cascade: one generation per call ----------------------------------------------------------------------------------------
static int cas_prepare(const char* who, const LdsimTrackGenParams* P, const LdsimTrackGenCascadeParams* CP,
                       const LdsimTrackGenParticle* part, int64_t n, GenConst* g, CasConst* cg) {
  GEN_NEED(P && CP && (n == 0 || part), "%s: null argument", who);
  GEN_NEED(n >= 0 && n <= 2147483647LL, "%s: %lld particles, need 0 .. 2^31 - 1", who, (long long)n);
  CK(gen_prepare_params(who, P, g, true));
  GEN_NEED(std::isfinite(CP->t_track) && CP->t_track >= P->t_cut && CP->t_track >= P->t_min,
           "%s: t_track %g MeV must be finite and at least t_cut %g and t_min %g", who, CP->t_track, P->t_cut, P->t_min);
  GEN_NEED(CP->capture_fraction >= 0 && CP->capture_fraction <= 1, "%s: capture_fraction %g must lie in [0, 1]", who,
           CP->capture_fraction);
  GEN_NEED(gen_pos(CP->mu_plus_lifetime), "%s: mu_plus_lifetime %g us must be finite and > 0", who, CP->mu_plus_lifetime);
  GEN_NEED(gen_pos(CP->mu_minus_lifetime), "%s: mu_minus_lifetime %g us must be finite and > 0", who, CP->mu_minus_lifetime);
  cg->t_track = CP->t_track;
  cg->tau_plus = CP->mu_plus_lifetime;
  cg->tau_minus = CP->mu_minus_lifetime;
  cg->capture = CP->capture_fraction;
  cg->delta = CP->emit != 0 && CP->delta_tracks != 0;
  cg->decays = CP->emit != 0 && CP->decays != 0;
  return gen_check_records(who, P, part, n, "particle", true);
}

// the count pass and its two scans; leaves the per-particle results in the ctx (tc_*), the totals in tc_total / tc_stotal.  Skipped
// when the ctx holds them for the same (parameters, cascade parameters, particles, seed) already.
static int cas_count_pass(ldsim_ctx* ctx, const GenConst& g, const CasConst& cg, const LdsimTrackGenParams* P,
                          const LdsimTrackGenCascadeParams* CP, const LdsimTrackGenParticle* part, int64_t n, uint64_t seed) {
  uint64_t h = gen_hash(0xCBF29CE484222325ULL ^ seed, P, sizeof(*P));
  h = gen_hash(h, CP, sizeof(*CP));
  h = gen_hash(h ^ (uint64_t)n, part, (size_t)n * sizeof(*part));
  if (ctx->tc_valid && ctx->tc_hash == h && ctx->tc_n == n) return 0;
  ctx->tc_valid = 0;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  CK(ctx->tc_part.ensure((size_t)n * sizeof(*part)));
  CK(ctx->tc_counts.ensure((size_t)n * 16));
  CK(ctx->tc_off.ensure((size_t)n * 16));
  CK(ctx->tc_state.ensure((size_t)n * 4));
  CK(ctx->tc_end.ensure((size_t)n * 48));
  ctx->tc_total = ctx->tc_stotal = 0;
  if (n) {
    unsigned long long* cnt = ctx->tc_counts.as<unsigned long long>();
    unsigned long long* off = ctx->tc_off.as<unsigned long long>();
    HIPCHK(hipMemcpyAsync(ctx->tc_part.p, part, (size_t)n * sizeof(*part), hipMemcpyHostToDevice, st));
    const int32_t group = gen_group(ctx, n);
    const unsigned blocks = (unsigned)((n + group - 1) / group);
    hipLaunchKernelGGL(cas_kernel<false>, dim3(blocks), dim3(GEN_BLOCK), 0, st, g, cg, ctx->tc_part.as<LdsimTrackGenParticle>(), n, seed,
                       group, cnt, cnt + n, ctx->tc_state.as<int32_t>(), ctx->tc_end.as<double>(), (const unsigned long long*)nullptr,
                       (const unsigned long long*)nullptr, (int64_t)0, (int64_t)0, (double*)nullptr, (int32_t*)nullptr,
                       (LdsimTrackGenParticle*)nullptr);
    HIPCHK(hipGetLastError());
    CK(sort_exclusive_scan_u64(ctx, cnt, off, n));
    CK(sort_exclusive_scan_u64(ctx, cnt + n, off + n, n));
    unsigned long long last[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(&last[0], cnt + (n - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&last[1], off + (n - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&last[2], cnt + (2 * n - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&last[3], off + (2 * n - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ctx->tc_total = (int64_t)(last[0] + last[1]);
    ctx->tc_stotal = (int64_t)(last[2] + last[3]);
  }
  ctx->tc_hash = h;
  ctx->tc_n = n;
  ctx->tc_valid = 1;
  return 0;
}

int trackgen_cascade_count(ldsim_ctx* ctx, const LdsimTrackGenParams* P, const LdsimTrackGenCascadeParams* CP,
                           const LdsimTrackGenParticle* part, int64_t n, uint64_t seed, int32_t* counts, int32_t* secondary_counts,
                           int32_t* end_state, double* end) {
  static const char who[] = "ldsim_track_cascade_count";
  GenConst g;
  CasConst cg;
  CK(cas_prepare(who, P, CP, part, n, &g, &cg));
  if (n == 0) return 0;
  GEN_NEED(counts && secondary_counts && end_state && end, "%s: null output array", who);
  CK(cas_count_pass(ctx, g, cg, P, CP, part, n, seed));
  std::vector<unsigned long long> c64((size_t)n * 2);
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(c64.data(), ctx->tc_counts.p, (size_t)n * 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(end_state, ctx->tc_state.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(end, ctx->tc_end.p, (size_t)n * 48, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; i++) {
    counts[i] = (int32_t)c64[(size_t)i];                        // (<= LDSIM_TRACK_GEN_MAX_STEPS each)
    secondary_counts[i] = (int32_t)c64[(size_t)(n + i)];        // (<= LDSIM_TRACK_GEN_HARD_CAP a step, + 1)
  }
  return 0;
}

int trackgen_cascade(ldsim_ctx* ctx, const LdsimTrackGenParams* P, const LdsimTrackGenCascadeParams* CP,
                     const LdsimTrackGenParticle* part, int64_t n, uint64_t seed, int64_t capacity, double* f64_columns,
                     int32_t* i32_columns, int64_t* n_segments, int64_t secondary_capacity, LdsimTrackGenParticle* secondaries,
                     int64_t* n_secondaries) {
  static const char who[] = "ldsim_track_cascade";
  GenConst g;
  CasConst cg;
  CK(cas_prepare(who, P, CP, part, n, &g, &cg));
  GEN_NEED(n_segments && n_secondaries, "%s: null n_segments or n_secondaries", who);
  GEN_NEED(capacity >= 0 && secondary_capacity >= 0, "%s: negative capacity", who);
  *n_segments = *n_secondaries = 0;
  ctx->ms_tc = 0;
  if (n == 0) return 0;
  CK(cas_count_pass(ctx, g, cg, P, CP, part, n, seed));
  const int64_t total = ctx->tc_total, stotal = ctx->tc_stotal;
  GEN_NEED(total <= 2147483647LL, "%s: %lld segments, more than 2^31 - 1: walk fewer particles per call", who, (long long)total);
  GEN_NEED(stotal <= 2147483647LL, "%s: %lld secondaries, more than 2^31 - 1: walk fewer particles per call", who, (long long)stotal);
  GEN_NEED(capacity >= total, "%s: capacity %lld is too small: %lld segments are needed", who, (long long)capacity, (long long)total);
  GEN_NEED(secondary_capacity >= stotal, "%s: secondary capacity %lld is too small: %lld secondaries are needed", who,
           (long long)secondary_capacity, (long long)stotal);
  GEN_NEED(f64_columns && i32_columns && (stotal == 0 || secondaries), "%s: null output array", who);
  hipStream_t st = ctx->stream;
  CK(ctx->tc_f64.ensure((size_t)total * 8 * LDSIM_TRACK_GEN_NF64));
  CK(ctx->tc_i32.ensure((size_t)total * 4 * LDSIM_TRACK_GEN_NI32));
  CK(ctx->tc_sec.ensure((size_t)(stotal ? stotal : 1) * sizeof(LdsimTrackGenParticle)));
  for (Event& e : ctx->tc_ev) CK(e.ensure());
  const int32_t group = gen_group(ctx, n);
  const unsigned blocks = (unsigned)((n + group - 1) / group);
  const unsigned long long* off = ctx->tc_off.as<unsigned long long>();
  HIPCHK(hipEventRecord(ctx->tc_ev[0], st));
  hipLaunchKernelGGL(cas_kernel<true>, dim3(blocks), dim3(GEN_BLOCK), 0, st, g, cg, ctx->tc_part.as<LdsimTrackGenParticle>(), n, seed, group,
                     (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int32_t*)nullptr, (double*)nullptr, off, off + n, total,
                     stotal, ctx->tc_f64.as<double>(), ctx->tc_i32.as<int32_t>(), ctx->tc_sec.as<LdsimTrackGenParticle>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->tc_ev[1], st));
  for (int c = 0; c < LDSIM_TRACK_GEN_NF64; c++)
    HIPCHK(hipMemcpyAsync(f64_columns + (size_t)c * capacity, ctx->tc_f64.as<double>() + (size_t)c * total, (size_t)total * 8,
                          hipMemcpyDeviceToHost, st));
  for (int c = 0; c < LDSIM_TRACK_GEN_NI32; c++)
    HIPCHK(hipMemcpyAsync(i32_columns + (size_t)c * capacity, ctx->tc_i32.as<int32_t>() + (size_t)c * total, (size_t)total * 4,
                          hipMemcpyDeviceToHost, st));
  if (stotal)
    HIPCHK(hipMemcpyAsync(secondaries, ctx->tc_sec.p, (size_t)stotal * sizeof(LdsimTrackGenParticle), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->tc_ev[0], ctx->tc_ev[1]));
  ctx->ms_tc = ms;
  *n_segments = total;
  *n_secondaries = stotal;
  return 0;
}

// generation 0 of a cascade: the primaries with the stream keys gen_start gives them (host only)
int trackgen_cascade_particles(const LdsimTrackGenPrimary* prim, int64_t n, LdsimTrackGenParticle* out) {
  static const char who[] = "ldsim_track_cascade_particles";
  GEN_NEED(n >= 0 && (n == 0 || (prim && out)), "%s: null argument or negative n", who);
  for (int64_t i = 0; i < n; i++) {
    const LdsimTrackGenPrimary& r = prim[i];
    LdsimTrackGenParticle& o = out[i];
    for (int k = 0; k < 3; k++) {
      o.pos[k] = r.pos[k];
      o.dir[k] = r.dir[k];
    }
    o.kinetic_energy = r.kinetic_energy;
    o.time = r.time;
    o.pdg = r.pdg;
    o.event_id = r.event_id;
    o.track_in_event = r.track_in_event;
    o._pad = 0;
    o.key = key_mix(key_mix(RNG_KEY_ROOT, (uint64_t)(int64_t)r.event_id), (uint64_t)(int64_t)r.track_in_event);
    o.parent = -1;
    o.generation = 0;
    o.process = 0;
    o.parent_step = -1;
  }
  return 0;
}
