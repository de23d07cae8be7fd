// Drift-field map builder: the perturbation potential of a space charge in one TPC box by conjugate gradients, the field at the
// nodes, and the drift paths from every node to the anode (include/ldsim.h states the model; larndsim_amd/field_map_builder.py
// restates it in numpy).
//
// Solve.  All vectors span every node; the face nodes of r, p and A p hold zeros, those of psi the boundary values, so one
// uniform stencil serves the reduced system.  An iteration k is two ordinary launches:
//   fb_step_a  |r|^2 from the chunk partials of the launch before; the end test; beta; p = r + beta p_old at a node and its six
//              neighbours (p is kept in two buffers by the parity of k, so no workgroup reads what another one writes in the
//              same launch); A p; the chunk partials of p . A p
//   fb_step_b  p . A p from those partials; alpha; psi += alpha p, r -= alpha A p; the chunk partials of |r|^2
// Every workgroup adds the chunk partials itself, in the same fixed order, so the scalars need no launch of their own and no
// workgroup waits for another one inside a launch.  The scalars stay on the device (FbState): once the end test passes in
// fb_step_a, workgroup 0 records it, and every later launch returns at its first read of that record.  The host queues
// check_every iterations, then reads FbState through the context's page-locked buffer.  A dot product is a sum over fixed chunks
// of 256 node indices followed by the sum of the partials, both in one fixed order: a workgroup walks chunks blockIdx.x,
// blockIdx.x + gridDim.x, .., so the bytes of psi do not depend on the grid (option fmap_build_wgs).  No atomics on floats, no
// cooperative launch, no flag that anything spins on.
// fb_residual_kernel forms the true residual s - L psi (the boundary values enter through L): it starts the iteration, and when
// the recurrence's residual has met the tolerance it is what the tolerance is held to (missed: the iteration restarts from it
// with beta = 0).
//
// Field and trace.  fb_field_kernel, one thread per node: (Ex, Ey, En, |E|) as one 32-byte record, so a corner of a cell is
// one read in fb_trace_kernel.  fb_trace_kernel, one thread per node, RK4 from the node to the anode plane: the threads are laid
// out so that the 64 lanes of a wave share the node's k, hence its step count N.  The grids of a TPC (2 MB of psi, 8 MB of
// records at 63 x 125 x 31) stay in L2.  Arithmetic in the twin's order (the library is built without contraction).
#include <math.h>

#include <vector>

#include "launchers.h"

#define FB_BLOCK 256
#define FB_MAX_WGS 1024

struct FbState {
  double bb;          // |b|^2
  double rr;          // |r|^2 of the recurrence at iteration `iters`
  double rr_true;     // |s - L psi|^2 of the last fb_residual_kernel
  double ring[4];     // |r|^2 of iteration k at k & 3 (+inf in front of a restart: beta = 0)
  int32_t done;       // 0: iterating; 1: tolerance met at `iters`; 2: max_iters reached; 3: a norm is not finite
  int32_t iters;
  int32_t ok;         // the true residual meets the tolerance
  int32_t pad;
};

struct FbGrid {
  double ih2[3];      // 1 / h^2
  int32_t n[3];
  int32_t nchunks;
  int64_t N;
};

// ---- fixed-order sums -----------------------------------------------------------------------------------------------------
// a wave's 64 values folded by halves; the four waves' sums added in order; every thread gets the result
__device__ __forceinline__ double fb_block_sum(double v, double* lds) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  __syncthreads();
  return s;
}

__device__ __forceinline__ double fb_sum_partials(const double* __restrict__ part, int nchunks, double* lds) {
  double acc = 0.0;
  for (int c = threadIdx.x; c < nchunks; c += FB_BLOCK) acc += part[c];
  return fb_block_sum(acc, lds);
}

__device__ __forceinline__ bool fb_interior(const FbGrid& g, int64_t idx, int64_t& sy, int64_t& sx) {
  const int nz = g.n[2], ny = g.n[1];
  const int k = (int)(idx % nz);
  const int64_t ij = idx / nz;
  const int j = (int)(ij % ny), i = (int)(ij / ny);
  sy = nz;
  sx = (int64_t)ny * nz;
  return i > 0 && i < g.n[0] - 1 && j > 0 && j < ny - 1 && k > 0 && k < nz - 1;
}

// (L v)(c) = sum over the axes of (2 v(c) - v(c - e) - v(c + e)) * (1 / h^2), at an interior node
__device__ __forceinline__ double fb_stencil(const FbGrid& g, double c, double xm, double xp, double ym, double yp, double zm,
                                             double zp) {
  const double c2 = 2.0 * c;
  return ((c2 - xm - xp) * g.ih2[0] + (c2 - ym - yp) * g.ih2[1]) + (c2 - zm - zp) * g.ih2[2];
}

// ---- the solve's kernels --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FB_BLOCK)
fb_residual_kernel(FbGrid g, const double* __restrict__ s, const double* __restrict__ x, double* __restrict__ r,
                   double* __restrict__ part_rr) {
  __shared__ double lds[4];
  for (int c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
    const int64_t idx = (int64_t)c * FB_BLOCK + threadIdx.x;
    double v = 0.0;
    if (idx < g.N) {
      int64_t sy, sx;
      double rv = 0.0;
      if (fb_interior(g, idx, sy, sx))
        rv = s[idx] - fb_stencil(g, x[idx], x[idx - sx], x[idx + sx], x[idx - sy], x[idx + sy], x[idx - 1], x[idx + 1]);
      r[idx] = rv;
      v = rv * rv;
    }
    const double sum = fb_block_sum(v, lds);
    if (threadIdx.x == 0) part_rr[c] = sum;
  }
}

// one workgroup.  mode 0: the start (|b|^2, nothing done); mode 1: the true residual at iteration k against the tolerance
__global__ void __launch_bounds__(FB_BLOCK)
fb_state_kernel(FbGrid g, const double* __restrict__ part_rr, FbState* __restrict__ st, int mode, int k, double tol2) {
  __shared__ double lds[4];
  const double rr = fb_sum_partials(part_rr, g.nchunks, lds);
  if (threadIdx.x != 0) return;
  st->rr_true = rr;
  if (mode == 0) {
    st->bb = rr;
    st->rr = rr;
    st->iters = 0;
    st->done = 0;
    st->ok = 0;
    st->pad = 0;
    for (int q = 0; q < 4; q++) st->ring[q] = HUGE_VAL;
  } else if (rr <= tol2 * st->bb) {
    st->ok = 1;
  } else {
    st->ok = 0;
    st->done = 0;
    st->ring[(k + 3) & 3] = HUGE_VAL;
  }
}

__global__ void __launch_bounds__(FB_BLOCK)
fb_step_a(FbGrid g, FbState* __restrict__ st, const double* __restrict__ r, const double* __restrict__ p_old,
          double* __restrict__ p_new, double* __restrict__ Ap, const double* __restrict__ part_rr, double* __restrict__ part_pAp,
          int k, int last, double tol2) {
  __shared__ double lds[4];
  __shared__ int s_done;
  // recorded by an earlier launch, or by workgroup 0 of this one, which saw the same partials as this workgroup is about to:
  // either answer leads to the same end, but the workgroup must take one answer as a whole (barriers follow)
  if (threadIdx.x == 0) s_done = st->done;
  __syncthreads();
  if (s_done) return;
  const double rr = fb_sum_partials(part_rr, g.nchunks, lds);
  const bool conv = rr <= tol2 * st->bb, fin = rr < HUGE_VAL;
  if (conv || last || !fin) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      st->rr = rr;
      st->iters = k;
      st->done = conv ? 1 : (fin ? 2 : 3);
    }
    return;
  }
  const double beta = rr / st->ring[(k + 3) & 3];          // iteration k - 1's, written by its launch
  if (blockIdx.x == 0 && threadIdx.x == 0) st->ring[k & 3] = rr;
  for (int c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
    const int64_t idx = (int64_t)c * FB_BLOCK + threadIdx.x;
    double v = 0.0;
    if (idx < g.N) {
      int64_t sy, sx;
      double pc = 0.0, ap = 0.0;
      if (fb_interior(g, idx, sy, sx)) {
        auto pn = [&](int64_t q) { return r[q] + beta * p_old[q]; };
        pc = pn(idx);
        ap = fb_stencil(g, pc, pn(idx - sx), pn(idx + sx), pn(idx - sy), pn(idx + sy), pn(idx - 1), pn(idx + 1));
      }
      p_new[idx] = pc;
      Ap[idx] = ap;
      v = pc * ap;
    }
    const double sum = fb_block_sum(v, lds);
    if (threadIdx.x == 0) part_pAp[c] = sum;
  }
}

__global__ void __launch_bounds__(FB_BLOCK)
fb_step_b(FbGrid g, const FbState* __restrict__ st, double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
          const double* __restrict__ Ap, const double* __restrict__ part_pAp, double* __restrict__ part_rr, int k) {
  __shared__ double lds[4];
  if (st->done) return;                                    // (by fb_step_a of this iteration: an earlier launch)
  const double pAp = fb_sum_partials(part_pAp, g.nchunks, lds);
  const double alpha = st->ring[k & 3] / pAp;
  for (int c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
    const int64_t idx = (int64_t)c * FB_BLOCK + threadIdx.x;
    double v = 0.0;
    if (idx < g.N) {
      x[idx] += alpha * p[idx];                            // (p and A p are 0 on the faces: the boundary values stay)
      const double rv = r[idx] - alpha * Ap[idx];
      r[idx] = rv;
      v = rv * rv;
    }
    const double sum = fb_block_sum(v, lds);
    if (threadIdx.x == 0) part_rr[c] = sum;
  }
}

// ---- field and trace ------------------------------------------------------------------------------------------------------
struct alignas(32) FbNode {
  double ex, ey, en, em;
};

struct FbTrace {
  double origin[3], h[3], ih[3];   // ih = 1 / h
  double hi[2];                    // origin + (n - 1) h in x and y
  double z_anode, nsign, e0, a[6], rT, step;
  int32_t n[3];
  int32_t nxy_pad;                 // nx ny rounded up to a multiple of 64
  int64_t N;
};

// d psi / d axis at a node: `pos` its index along the axis, `s` the axis's stride
__device__ __forceinline__ double fb_deriv(const double* __restrict__ psi, int64_t idx, int64_t s, int pos, int n, double ih) {
  if (n == 2) {
    const int64_t b = idx - pos * s;
    return (psi[b + s] - psi[b]) * ih;
  }
  const double hih = 0.5 * ih;
  // (differences from the face node first: a potential that does not vary along the axis gives exactly 0)
  if (pos == 0) return (4.0 * (psi[idx + s] - psi[idx]) - (psi[idx + 2 * s] - psi[idx])) * hih;
  if (pos == n - 1) return ((psi[idx - 2 * s] - psi[idx]) - 4.0 * (psi[idx - s] - psi[idx])) * hih;
  return (psi[idx + s] - psi[idx - s]) * hih;
}

__global__ void __launch_bounds__(FB_BLOCK) fb_field_kernel(FbTrace g, const double* __restrict__ psi, FbNode* __restrict__ node) {
  const int64_t idx = (int64_t)blockIdx.x * FB_BLOCK + threadIdx.x;
  if (idx >= g.N) return;
  const int nz = g.n[2], ny = g.n[1];
  const int k = (int)(idx % nz);
  const int64_t ij = idx / nz;
  const int j = (int)(ij % ny), i = (int)(ij / ny);
  FbNode o;
  o.ex = -fb_deriv(psi, idx, (int64_t)ny * nz, i, g.n[0], g.ih[0]);
  o.ey = -fb_deriv(psi, idx, nz, j, ny, g.ih[1]);
  o.en = g.e0 - g.nsign * fb_deriv(psi, idx, 1, k, nz, g.ih[2]);
  o.em = (o.ex == 0.0 && o.ey == 0.0) ? fabs(o.en) : sqrt((o.ex * o.ex + o.ey * o.ey) + o.en * o.en);
  node[idx] = o;
}

struct FbMob {
  double a0, a1, a2, a3, a4, a5, a10, tc;
};
__device__ __forceinline__ double fb_mu(const FbMob& m, double e) {
  const double se = sqrt(e), e2 = e * e;
  const double num = ((m.a0 + m.a1 * e) + m.a2 * (e * se)) + m.a3 * (e2 * se);
  const double den = ((1.0 + m.a10 * e) + m.a4 * e2) + m.a5 * (e2 * e);
  return ((num / den) * m.tc) * 1e-3;
}

// the right-hand side at (x, y, q): false where the field reverses
__device__ __forceinline__ bool fb_rhs(const FbTrace& g, const FbNode* __restrict__ node, const FbMob& m, double vd, double x,
                                       double y, double q, double f[3]) {
  const double p[3] = {x, y, g.z_anode + g.nsign * q};
  int64_t i0[3];
  double w[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    double u = (p[a] - g.origin[a]) * g.ih[a];
    u = fmin(fmax(u, 0.0), (double)(g.n[a] - 1));
    const int c = min((int)u, g.n[a] - 2);
    i0[a] = c;
    w[a] = u - (double)c;
  }
  const int64_t sz = g.n[2], sy = (int64_t)g.n[1] * g.n[2];
  const FbNode* b = node + i0[0] * sy + i0[1] * sz + i0[2];
  FbNode c[8];
#pragma unroll
  for (int t = 0; t < 8; t++) c[t] = b[((t >> 2) & 1) * sy + ((t >> 1) & 1) * sz + (t & 1)];
  auto lerp = [](double a0, double a1, double t) { return a0 + t * (a1 - a0); };
  auto tri = [&](double FbNode::*ch) {
    const double c00 = lerp(c[0].*ch, c[1].*ch, w[2]), c01 = lerp(c[2].*ch, c[3].*ch, w[2]);
    const double c10 = lerp(c[4].*ch, c[5].*ch, w[2]), c11 = lerp(c[6].*ch, c[7].*ch, w[2]);
    return lerp(lerp(c00, c01, w[1]), lerp(c10, c11, w[1]), w[0]);
  };
  const double ex = tri(&FbNode::ex), ey = tri(&FbNode::ey), en = tri(&FbNode::en), em = tri(&FbNode::em);
  if (!(en > 0.0)) return false;
  f[0] = -(ex / en);
  f[1] = -(ey / en);
  f[2] = vd / (fb_mu(m, em) * en) - 1.0;
  return true;
}

__global__ void __launch_bounds__(FB_BLOCK)
fb_trace_kernel(FbTrace g, const FbNode* __restrict__ node, double* __restrict__ out, unsigned* __restrict__ err,
                uint8_t* __restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * FB_BLOCK + threadIdx.x;
  const int k = (int)(t / g.nxy_pad);
  const int ij = (int)(t - (int64_t)k * g.nxy_pad);
  if (k >= g.n[2] || ij >= g.n[0] * g.n[1]) return;
  const int i = ij / g.n[1], j = ij - i * g.n[1];
  const int64_t idx = (int64_t)ij * g.n[2] + k;
  FbMob m;
  m.a0 = g.a[0]; m.a1 = g.a[1]; m.a2 = g.a[2]; m.a3 = g.a[3]; m.a4 = g.a[4]; m.a5 = g.a[5];
  m.a10 = g.a[1] / g.a[0];
  m.tc = 1.0 / (g.rT * sqrt(g.rT));
  const double vd = g.e0 * fb_mu(m, g.e0);
  const double x0 = g.origin[0] + i * g.h[0], y0 = g.origin[1] + j * g.h[1];
  const double qn = fabs((g.origin[2] + k * g.h[2]) - g.z_anode);
  double x = x0, y = y0, tau = 0.0;
  if (qn > 0.0) {
    const int n_steps = (int)fmax(1.0, ceil(qn / g.step));   // <= LDSIM_FIELD_MAP_BUILD_MAX_STEPS (the launcher's check)
    const double ds = qn / (double)n_steps, hds = 0.5 * ds, ds6 = ds / 6.0;
    for (int s = 0; s < n_steps; s++) {
      const double q0 = qn - (double)s * ds, qh = qn - ((double)s + 0.5) * ds, q1 = qn - ((double)s + 1.0) * ds;
      double k1[3], k2[3], k3[3], k4[3];
      const bool ok = fb_rhs(g, node, m, vd, x, y, q0, k1) && fb_rhs(g, node, m, vd, x + hds * k1[0], y + hds * k1[1], qh, k2) &&
                      fb_rhs(g, node, m, vd, x + hds * k2[0], y + hds * k2[1], qh, k3) &&
                      fb_rhs(g, node, m, vd, x + ds * k3[0], y + ds * k3[1], q1, k4);
      if (!ok) {
        atomicMin(err, (unsigned)idx);                     // (an integer: the lowest reversed node, whatever the order)
        return;
      }
      x = x + ds6 * (((k1[0] + 2.0 * k2[0]) + 2.0 * k3[0]) + k4[0]);
      y = y + ds6 * (((k1[1] + 2.0 * k2[1]) + 2.0 * k3[1]) + k4[1]);
      tau = tau + ds6 * (((k1[2] + 2.0 * k2[2]) + 2.0 * k3[2]) + k4[2]);
    }
  }
  out[idx] = node[idx].em;
  out[g.N + idx] = x - x0;
  out[2 * g.N + idx] = y - y0;
  out[3 * g.N + idx] = g.nsign * tau;
  flags[idx] = (x < g.origin[0] || x > g.hi[0] || y < g.origin[1] || y > g.hi[1]) ? 1 : 0;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
#define FB_NEED(cond, ...)                  \
  do {                                      \
    if (!(cond)) {                          \
      ldsim_set_error(__VA_ARGS__);         \
      return LDSIM_EINVAL;                  \
    }                                       \
  } while (0)

static int fb_check_params(const LdsimFieldMapBuildParams* P, const char* who) {
  static const char axis[] = "xyz";
  for (int a = 0; a < 3; a++) {
    FB_NEED(std::isfinite(P->spacing[a]) && P->spacing[a] > 0, "%s: spacing[%c] %g cm, need a finite pitch > 0", who, axis[a],
            P->spacing[a]);
    FB_NEED(std::isfinite(P->origin[a]), "%s: origin[%c] %g is not finite", who, axis[a], P->origin[a]);
    FB_NEED(P->n[a] >= 2, "%s: dimension n%c = %d, every dimension must be >= 2", who, axis[a], P->n[a]);
  }
  FB_NEED((int64_t)P->n[0] * P->n[1] * P->n[2] <= 2147483647LL, "%s: %d x %d x %d nodes exceed 2^31 - 1", who, P->n[0], P->n[1],
          P->n[2]);
  FB_NEED(std::isfinite(P->e0) && P->e0 > 0, "%s: E0 %g kV/cm, need a finite field > 0", who, P->e0);
  FB_NEED(std::isfinite(P->temperature) && P->temperature > 0, "%s: temperature %g K, need a finite temperature > 0", who,
          P->temperature);
  FB_NEED(std::isfinite(P->tol) && P->tol > 0, "%s: tol %g, need a finite tolerance > 0", who, P->tol);
  FB_NEED(std::isfinite(P->step) && P->step > 0, "%s: step %g cm, need a finite step > 0", who, P->step);
  FB_NEED(std::isfinite(P->mobility[0]) && P->mobility[0] != 0, "%s: mobility[0] %g, need a finite value other than 0", who,
          P->mobility[0]);
  for (int q = 1; q < 6; q++) FB_NEED(std::isfinite(P->mobility[q]), "%s: mobility[%d] %g is not finite", who, q, P->mobility[q]);
  FB_NEED(std::isfinite(P->z_anode) && std::isfinite(P->z_cathode), "%s: z_anode %g, z_cathode %g: need finite planes", who,
          P->z_anode, P->z_cathode);
  FB_NEED(P->z_anode != P->z_cathode, "%s: z_anode == z_cathode (%g): the drift direction is undefined", who, P->z_anode);
  FB_NEED(P->max_iters >= 1, "%s: max_iters %d, need >= 1", who, P->max_iters);
  FB_NEED(P->check_every >= 1, "%s: check_every %d, need >= 1", who, P->check_every);
  const double z_far = P->origin[2] + (P->n[2] - 1) * P->spacing[2];
  const double q_max = fmax(fabs(P->origin[2] - P->z_anode), fabs(z_far - P->z_anode));
  FB_NEED(q_max / P->step <= (double)LDSIM_FIELD_MAP_BUILD_MAX_STEPS, "%s: step %g cm makes %g steps on the longest path (%g cm), "
          "more than %d", who, P->step, ceil(q_max / P->step), q_max, LDSIM_FIELD_MAP_BUILD_MAX_STEPS);
  return 0;
}

static bool fb_on_face(const LdsimFieldMapBuildParams* P, int64_t idx) {
  const int nz = P->n[2], ny = P->n[1];
  const int k = (int)(idx % nz), j = (int)((idx / nz) % ny), i = (int)(idx / nz / ny);
  return i == 0 || i == P->n[0] - 1 || j == 0 || j == ny - 1 || k == 0 || k == nz - 1;
}

static int fb_event_ms(ldsim_ctx* ctx, int first, double* ms) {
  float v = 0;
  HIPCHK(hipEventElapsedTime(&v, ctx->fb_ev[first], ctx->fb_ev[first + 1]));
  *ms = v;
  return 0;
}

int fmapbuild_solve(ldsim_ctx* ctx, const LdsimFieldMapBuildParams* P, const double* source, double* psi_inout, int32_t* iterations,
                    double* residual) {
  static const char who[] = "ldsim_field_map_solve";
  FB_NEED(P && source && psi_inout && iterations && residual, "%s: null argument", who);
  CK(fb_check_params(P, who));
  const int64_t N = (int64_t)P->n[0] * P->n[1] * P->n[2];
  std::vector<double> x0((size_t)N, 0.0);
  for (int64_t q = 0; q < N; q++) {
    FB_NEED(std::isfinite(source[q]), "%s: source[%lld] = %g is not finite", who, (long long)q, source[q]);
    if (fb_on_face(P, q)) {
      FB_NEED(std::isfinite(psi_inout[q]), "%s: boundary value psi[%lld] = %g is not finite", who, (long long)q, psi_inout[q]);
      x0[(size_t)q] = psi_inout[q];
    }
  }
  FbGrid g;
  for (int a = 0; a < 3; a++) {
    g.ih2[a] = 1.0 / (P->spacing[a] * P->spacing[a]);
    g.n[a] = P->n[a];
  }
  g.N = N;
  g.nchunks = (int)((N + FB_BLOCK - 1) / FB_BLOCK);
  const double tol2 = P->tol * P->tol;
  const int wgs = ctx->fb_wgs > 0 ? ctx->fb_wgs : (g.nchunks < FB_MAX_WGS ? g.nchunks : FB_MAX_WGS);
  const size_t vb = (size_t)N * sizeof(double);
  ctx->ms_fb[0] = 0;
  HIPCHK(hipSetDevice(ctx->device));
  CK(ctx->fb_vec.ensure(6 * vb));
  CK(ctx->fb_part.ensure(2 * (size_t)g.nchunks * sizeof(double)));
  CK(ctx->fb_state.ensure(sizeof(FbState)));
  CK(ctx->readback.ensure(sizeof(ChainReadback) > sizeof(FbState) ? sizeof(ChainReadback) : sizeof(FbState)));
  CK(ctx->fb_ev[0].ensure());
  CK(ctx->fb_ev[1].ensure());
  double* d_s = ctx->fb_vec.as<double>();
  double *d_x = d_s + N, *d_r = d_s + 2 * N, *d_Ap = d_s + 3 * N;
  double* d_p[2] = {d_s + 4 * N, d_s + 5 * N};
  double *d_prr = ctx->fb_part.as<double>(), *d_ppap = d_prr + g.nchunks;
  FbState* d_st = ctx->fb_state.as<FbState>();
  const FbState* h = (const FbState*)ctx->readback.p;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(d_s, source, vb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_x, x0.data(), vb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_p[0], 0, 2 * vb, st));
  HIPCHK(hipStreamSynchronize(st));                          // (x0 is pageable: gone from here on)
  HIPCHK(hipEventRecord(ctx->fb_ev[0], st));
  hipLaunchKernelGGL(fb_residual_kernel, dim3(wgs), dim3(FB_BLOCK), 0, st, g, d_s, d_x, d_r, d_prr);
  hipLaunchKernelGGL(fb_state_kernel, dim3(1), dim3(FB_BLOCK), 0, st, g, d_prr, d_st, 0, 0, tol2);
  HIPCHK(hipGetLastError());
  int k = 0, rc = 0;
  for (;;) {
    for (int c = 0; c < P->check_every && k <= P->max_iters; c++, k++) {
      hipLaunchKernelGGL(fb_step_a, dim3(wgs), dim3(FB_BLOCK), 0, st, g, d_st, d_r, d_p[(k + 1) & 1], d_p[k & 1], d_Ap, d_prr, d_ppap,
                         k, k == P->max_iters ? 1 : 0, tol2);
      if (k < P->max_iters)
        hipLaunchKernelGGL(fb_step_b, dim3(wgs), dim3(FB_BLOCK), 0, st, g, d_st, d_x, d_r, d_p[k & 1], d_Ap, d_ppap, d_prr, k);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctx->readback.p, d_st, sizeof(FbState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h->done == 1) {
      // the recurrence's residual has met the tolerance at h->iters: hold the true one to it
      const int at = h->iters;
      hipLaunchKernelGGL(fb_residual_kernel, dim3(wgs), dim3(FB_BLOCK), 0, st, g, d_s, d_x, d_r, d_prr);
      hipLaunchKernelGGL(fb_state_kernel, dim3(1), dim3(FB_BLOCK), 0, st, g, d_prr, d_st, 1, at, tol2);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(ctx->readback.p, d_st, sizeof(FbState), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (h->ok) break;
      if (at >= P->max_iters) {
        rc = LDSIM_ENOCONV;
        break;
      }
      k = at;                                                // restart from the true residual (beta = 0 at iteration `at`)
      continue;
    }
    if (h->done || k > P->max_iters) {
      rc = LDSIM_ENOCONV;
      break;
    }
  }
  HIPCHK(hipEventRecord(ctx->fb_ev[1], st));
  if (rc) {
    HIPCHK(hipStreamSynchronize(st));
    CK(fb_event_ms(ctx, 0, &ctx->ms_fb[0]));
    const double rr = h->done == 1 ? h->rr_true : h->rr;
    ldsim_set_error("%s: relative residual %.3e after %d iterations, above tol %.3e (max_iters %d)%s", who,
                    h->bb > 0 ? sqrt(rr / h->bb) : rr, (int)h->iters, P->tol, P->max_iters,
                    h->done == 3 ? ": a norm is not finite" : "");
    return rc;
  }
  *iterations = h->iters;
  *residual = h->bb > 0 ? sqrt(h->rr_true / h->bb) : 0.0;
  HIPCHK(hipMemcpyAsync(psi_inout, d_x, vb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  CK(fb_event_ms(ctx, 0, &ctx->ms_fb[0]));
  return 0;
}

int fmapbuild_trace(ldsim_ctx* ctx, const LdsimFieldMapBuildParams* P, const double* psi, double* E, double* dx, double* dy,
                    double* dz, uint8_t* flags) {
  static const char who[] = "ldsim_field_map_trace";
  FB_NEED(P && psi && E && dx && dy && dz && flags, "%s: null argument", who);
  CK(fb_check_params(P, who));
  const int64_t N = (int64_t)P->n[0] * P->n[1] * P->n[2];
  for (int64_t q = 0; q < N; q++) FB_NEED(std::isfinite(psi[q]), "%s: psi[%lld] = %g is not finite", who, (long long)q, psi[q]);
  FbTrace g;
  for (int a = 0; a < 3; a++) {
    g.origin[a] = P->origin[a];
    g.h[a] = P->spacing[a];
    g.ih[a] = 1.0 / P->spacing[a];
    g.n[a] = P->n[a];
  }
  for (int a = 0; a < 2; a++) g.hi[a] = P->origin[a] + (P->n[a] - 1) * P->spacing[a];
  g.z_anode = P->z_anode;
  g.nsign = P->z_cathode > P->z_anode ? 1.0 : -1.0;
  g.e0 = P->e0;
  for (int q = 0; q < 6; q++) g.a[q] = P->mobility[q];
  g.rT = P->temperature / 89.0;
  g.step = P->step;
  const int64_t nxy = (int64_t)P->n[0] * P->n[1];
  g.nxy_pad = (int32_t)((nxy + 63) / 64 * 64);
  g.N = N;
  const int64_t threads = (int64_t)g.nxy_pad * P->n[2];
  FB_NEED(threads / FB_BLOCK + 1 <= 2147483647LL && nxy <= 2147483584LL, "%s: %d x %d x %d nodes exceed one launch", who, P->n[0],
          P->n[1], P->n[2]);
  const size_t vb = (size_t)N * sizeof(double);
  ctx->ms_fb[1] = ctx->ms_fb[2] = 0;
  HIPCHK(hipSetDevice(ctx->device));
  CK(ctx->fb_field.ensure((size_t)N * sizeof(FbNode) + vb));
  CK(ctx->fb_out.ensure(4 * vb + 8 + (size_t)N));
  for (int e = 2; e < 6; e++) CK(ctx->fb_ev[e].ensure());
  CK(ctx->readback.ensure(sizeof(ChainReadback)));
  FbNode* d_node = ctx->fb_field.as<FbNode>();
  double* d_psi = (double*)(d_node + N);
  double* d_out = ctx->fb_out.as<double>();
  unsigned* d_err = (unsigned*)(d_out + 4 * N);
  uint8_t* d_flags = (uint8_t*)(d_err + 2);
  unsigned* h_err = (unsigned*)ctx->readback.p;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(d_psi, psi, vb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_err, 0xFF, 8, st));
  HIPCHK(hipEventRecord(ctx->fb_ev[2], st));
  hipLaunchKernelGGL(fb_field_kernel, dim3((unsigned)((N + FB_BLOCK - 1) / FB_BLOCK)), dim3(FB_BLOCK), 0, st, g, d_psi, d_node);
  HIPCHK(hipEventRecord(ctx->fb_ev[3], st));
  HIPCHK(hipEventRecord(ctx->fb_ev[4], st));
  hipLaunchKernelGGL(fb_trace_kernel, dim3((unsigned)((threads + FB_BLOCK - 1) / FB_BLOCK)), dim3(FB_BLOCK), 0, st, g, d_node, d_out,
                     d_err, d_flags);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->fb_ev[5], st));
  HIPCHK(hipMemcpyAsync(h_err, d_err, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  CK(fb_event_ms(ctx, 2, &ctx->ms_fb[1]));
  CK(fb_event_ms(ctx, 4, &ctx->ms_fb[2]));
  if (*h_err != 0xFFFFFFFFu) {
    const int64_t q = *h_err;
    ldsim_set_error("%s: field reverses on the path of node %lld (i, j, k) = (%lld, %lld, %lld): En <= 0, the space charge "
                    "outweighs E0 = %g kV/cm", who, (long long)q, (long long)(q / P->n[2] / P->n[1]),
                    (long long)(q / P->n[2] % P->n[1]), (long long)(q % P->n[2]), P->e0);
    return LDSIM_EINVAL;
  }
  HIPCHK(hipMemcpyAsync(E, d_out, vb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(dx, d_out + N, vb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(dy, d_out + 2 * N, vb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(dz, d_out + 3 * N, vb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(flags, d_flags, (size_t)N, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
