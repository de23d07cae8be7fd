// Field-response builder: the induction table of a pixelated anode by the Shockley-Ramo theorem (include/ldsim.h states the
// model; larndsim_amd/response_builder.py restates it in numpy).
//
// table[i][j][k] = (phibar(i, j, k + 1) - phibar(i, j, k)) / sampling, phibar the mean over n_sub x n_sub transverse midpoints of
// the pad's weighting potential at the height of tick edge m.  The cost is n_i n_j (n_k + 1) n_sub^2 evaluations of four f64
// atan2 and square roots: f64 vector arithmetic, no memory traffic beyond the one store per entry.
//
// response_build_kernel: one workgroup per (i, j) row, lanes over the tick edges.  A lane keeps phibar of its edge in registers
// over the sub-samples (p outer, q inner: one fixed order, so a row's bytes do not depend on the launch), the row's n_k + 1
// edges go to LDS, and after one barrier the lanes difference neighbours and store along k (coalesced).  Nothing is read from
// global memory.  The row must fit the workgroup's LDS: the launcher refuses n_k > LDSIM_RESPONSE_BUILD_MAX_K by name.
#include <math.h>

#include "launchers.h"

#define RB_BLOCK 256
#define RB_LDS_BYTES (60 * 1024)       // budget of a workgroup's LDS: (n_k + 1) f64 edges
static_assert((LDSIM_RESPONSE_BUILD_MAX_K + 1) * sizeof(double) <= RB_LDS_BYTES, "a row of edges must fit the LDS budget");

#define RB_INV_2PI 0.15915494309189535   // 1 / (2 pi), rounded to nearest

struct RbGeom {
  double a;          // pad_size / 2
  double bin;        // transverse bin, cm
  double v;          // drift velocity, cm / us
  double dt;         // tick, us
  int32_t n_j, n_k, n_sub, arrival;
};

// the weighting potential of the square pad |x|, |y| <= a in the grounded plane z = 0, at (x, y, z >= 0): its solid angle / 2 pi
__device__ __forceinline__ double rb_phi(double x, double y, double z, double a) {
  const double xm = x - a, xp = x + a, ym = y - a, yp = y + a;
  const double zz = z * z, xm2 = xm * xm, xp2 = xp * xp, ym2 = ym * ym, yp2 = yp * yp;
  double s = atan2(xm * ym, z * sqrt(xm2 + ym2 + zz));        // sx = -1, sy = -1
  s -= atan2(xm * yp, z * sqrt(xm2 + yp2 + zz));              // sx = -1, sy = +1
  s -= atan2(xp * ym, z * sqrt(xp2 + ym2 + zz));              // sx = +1, sy = -1
  s += atan2(xp * yp, z * sqrt(xp2 + yp2 + zz));              // sx = +1, sy = +1
  return s * RB_INV_2PI;
}

__global__ void __launch_bounds__(RB_BLOCK)
response_build_kernel(RbGeom g, double* __restrict__ table) {
  extern __shared__ double rb_edge[];                          // phibar of the row's edges m = 0 .. n_k
  const int i = blockIdx.x / g.n_j, j = blockIdx.x - i * g.n_j;
  const int n = g.n_sub;
  const double t_arrive = (g.arrival + 0.5) * g.dt;
  const double n2 = (double)(n * n);
  for (int m = threadIdx.x; m <= g.n_k; m += RB_BLOCK) {
    const double z = g.v * fmax(0.0, t_arrive - (m - 0.5) * g.dt);     // exactly 0 from edge arrival + 1 on
    double acc = 0.0;
    for (int p = 0; p < n; p++) {
      const double x = (i + (p + 0.5) / n) * g.bin;
      for (int q = 0; q < n; q++) {
        const double y = (j + (q + 0.5) / n) * g.bin;
        acc += rb_phi(x, y, z, g.a);
      }
    }
    rb_edge[m] = acc / n2;
  }
  __syncthreads();
  double* row = table + (size_t)blockIdx.x * g.n_k;
  for (int k = threadIdx.x; k < g.n_k; k += RB_BLOCK) row[k] = (rb_edge[k + 1] - rb_edge[k]) / g.dt;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
int respbuild_build(ldsim_ctx* ctx, const LdsimResponseBuildParams* P, double* table) {
  static const char who[] = "ldsim_response_build";
  if (!P || !table) {
    ldsim_set_error("%s: null argument", who);
    return LDSIM_EINVAL;
  }
#define RB_NEED(cond, ...)                  \
  do {                                      \
    if (!(cond)) {                          \
      ldsim_set_error(__VA_ARGS__);         \
      return LDSIM_EINVAL;                  \
    }                                       \
  } while (0)
  RB_NEED(std::isfinite(P->pad_size) && P->pad_size > 0, "%s: pad_size %g cm, need a finite size > 0", who, P->pad_size);
  RB_NEED(std::isfinite(P->bin_size) && P->bin_size > 0, "%s: bin_size %g cm, need a finite size > 0", who, P->bin_size);
  RB_NEED(std::isfinite(P->v_drift) && P->v_drift > 0, "%s: v_drift %g cm/us, need a finite velocity > 0", who, P->v_drift);
  RB_NEED(std::isfinite(P->sampling) && P->sampling > 0, "%s: sampling %g us, need a finite tick > 0", who, P->sampling);
  RB_NEED(P->n_i >= 1 && P->n_j >= 1 && P->n_k >= 1, "%s: zero-sized table (n_i, n_j, n_k) = (%d, %d, %d)", who, P->n_i, P->n_j,
          P->n_k);
  RB_NEED(P->n_k <= LDSIM_RESPONSE_BUILD_MAX_K, "%s: n_k %d, a row of n_k + 1 tick edges must fit the kernel's LDS: n_k <= %d", who,
          P->n_k, LDSIM_RESPONSE_BUILD_MAX_K);
  RB_NEED(P->n_sub >= 1 && P->n_sub <= LDSIM_RESPONSE_BUILD_MAX_NSUB, "%s: n_sub %d, need 1 .. %d", who, P->n_sub,
          LDSIM_RESPONSE_BUILD_MAX_NSUB);
  RB_NEED(P->arrival_tick >= 0 && P->arrival_tick < P->n_k, "%s: arrival_tick %d outside [0, n_k = %d)", who, P->arrival_tick,
          P->n_k);
  const int64_t rows = (int64_t)P->n_i * P->n_j;
  RB_NEED(rows <= 2147483647LL, "%s: n_i x n_j = %lld rows exceed one launch (2^31 - 1)", who, (long long)rows);
#undef RB_NEED
  RbGeom g;
  g.a = 0.5 * P->pad_size;
  g.bin = P->bin_size;
  g.v = P->v_drift;
  g.dt = P->sampling;
  g.n_j = P->n_j;
  g.n_k = P->n_k;
  g.n_sub = P->n_sub;
  g.arrival = P->arrival_tick;
  const size_t bytes = (size_t)rows * P->n_k * sizeof(double);
  const size_t lds = ((size_t)P->n_k + 1) * sizeof(double);
  ctx->ms_rb = 0;
  HIPCHK(hipSetDevice(ctx->device));
  CK(ctx->rb_table.ensure(bytes));
  for (Event& e : ctx->rb_ev) CK(e.ensure());
  hipStream_t st = ctx->stream;
  HIPCHK(hipEventRecord(ctx->rb_ev[0], st));
  hipLaunchKernelGGL(response_build_kernel, dim3((unsigned)rows), dim3(RB_BLOCK), lds, st, g, ctx->rb_table.as<double>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->rb_ev[1], st));
  HIPCHK(hipMemcpyAsync(table, ctx->rb_table.p, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->rb_ev[0], ctx->rb_ev[1]));
  ctx->ms_rb = ms;
  return 0;
}
