// seg_charge.h -- the charge arithmetic of the resident quench/drift (kernels_seg.hip) that charge_weights_kernel
// (kernels_feeuni.hip) replays under a universe's constants: the recombination factor, the drift-field map's interpolation and
// the two truncating stores of n_electrons.  The helpers are templates over the constants block, so the quench/drift kernels
// instantiate them with LdsimConsts exactly as when the text stood in kernels_seg.hip, and the replay with ChargeK.
#pragma once
#include "ldsim_dev.h"

// quench_at's recombination factor alone: 0 = recomb set, 1 = unknown mode, 2 = NaN
template <class K>
__device__ __forceinline__ int recomb_at(const K* __restrict__ c, int mode, double e_field, double dEdx, double& recomb) {
  recomb = 0;
  if (mode == 1) {  // BOX
    double csi = c->box_beta * dEdx / (e_field * c->lar_density);
    double r = log(c->box_alpha + csi) / csi;
    recomb = (r > 0) ? r : 0;
  } else if (mode == 2) {  // BIRKS
    recomb = c->birks_ab / (1 + c->birks_kb * dEdx / (e_field * c->lar_density));
  } else {
    return 1;
  }
  return isnan(recomb) ? 2 : 0;
}

// Trilinear interpolation of the map at p, clamped to the edge nodes; a + f * (b - a) per axis (z, then y, then x), so a
// constant map returns its constant exactly.  with_e = 0 leaves v[0] unset.
__device__ __forceinline__ void fmap_eval(const FieldMapDesc& m, const double p[3], bool with_e, double v[4]) {
  int64_t i0[3];
  double f[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    double u = (p[a] - m.origin[a]) * m.inv_spacing[a];
    u = fmin(fmax(u, 0.0), (double)(m.n[a] - 1));   // (fmax(NaN, 0) = 0: every index stays inside the grid)
    const int k = min((int)u, m.n[a] - 2);
    i0[a] = k;
    f[a] = u - (double)k;
  }
  const int64_t sz = m.n[2], sy = (int64_t)m.n[1] * m.n[2];
  const FieldMapNode* b = m.node + i0[0] * sy + i0[1] * sz + i0[2];
  FieldMapNode q[8];
#pragma unroll
  for (int k = 0; k < 8; k++) q[k] = b[((k >> 2) & 1) * sy + ((k >> 1) & 1) * sz + (k & 1)];
  auto lerp = [](double a0, double a1, double t) { return a0 + t * (a1 - a0); };
  auto tri = [&](double FieldMapNode::*ch) {
    const double c00 = lerp(q[0].*ch, q[1].*ch, f[2]), c01 = lerp(q[2].*ch, q[3].*ch, f[2]);
    const double c10 = lerp(q[4].*ch, q[5].*ch, f[2]), c11 = lerp(q[6].*ch, q[7].*ch, f[2]);
    return lerp(lerp(c00, c01, f[1]), lerp(c10, c11, f[1]), f[0]);
  };
  if (with_e) v[0] = tri(&FieldMapNode::e);
  v[1] = tri(&FieldMapNode::dx);
  v[2] = tri(&FieldMapNode::dy);
  v[3] = tri(&FieldMapNode::dz);
}

// The constants of the charge arithmetic that one charge universe holds (LdsimChargeVariation) beside the two it keeps from
// the launch; the member names are LdsimConsts' so that recomb_at reads either.
struct ChargeK {
  double box_alpha, box_beta, birks_ab, birks_kb, w_ion, electron_lifetime;
  double lar_density, v_drift;
  int32_t mode, pad;
};

// What quench_drift_kernel / quench_drift_map_kernel store in n_electrons for a segment inside a TPC: recombination at e_field,
// the store, the lifetime factor over the drift from z to the anode at z_anode, the store again (`code`: the column's store
// code).  Returns false where the launch's kernels refuse (unknown mode, NaN recombination).
__device__ __forceinline__ bool charge_replay(const ChargeK* __restrict__ c, double e_field, double dE, double dEdx, double z,
                                              double z_anode, int code, double& n_k) {
  double recomb;
  if (recomb_at(c, c->mode, e_field, dEdx, recomb) != 0) return false;
  const double n_e = narrow_store(recomb * dE / c->w_ion, code);
  double drift_distance = fabs(z - z_anode);
  double drift_time = drift_distance / c->v_drift;
  double lifetime_red = exp(-drift_time / c->electron_lifetime);
  n_k = narrow_store(n_e * lifetime_red, code);
  return true;
}

// ---- the charge statistics' binomial sampler (quench_drift_stat_kernel, kernels_seg.hip; light_sipm_count_kernel, light_wvfm.hip) ----
// Binomial(n, p) from one normal draw z and one uniform draw u, n a whole number held in a double.  Design constants:
// BINOM_NORMAL_MIN = 30 (n * min(p, 1 - p) from which the rounded normal is drawn) and BINOM_WALK_MAX = 256 (where the
// inversion walk stops).  Below 30: inversion on the minority outcome at the centre u - 2^-25 of the uniform's 24-bit cell,
// P(0) = exp(n log1p(-pm)), P(j + 1) = P(j) (n - j) / (j + 1) * (pm / (1 - pm)), j = the first running sum >= the centre.
// larndsim_amd/charge_stats.py restates this operation for operation.
#define BINOM_NORMAL_MIN 30.0
#define BINOM_WALK_MAX 256.0
__device__ __forceinline__ double binomial_draw(double n, double p, float z, float u) {
  if (!(n > 0) || !(p > 0)) return 0;
  if (p >= 1) return n;
  const double pm = fmin(p, 1 - p);
  if (n * pm >= BINOM_NORMAL_MIN) return fmin(fmax(rint(n * p + sqrt(n * p * (1 - p)) * (double)z), 0.0), n);
  const double centre = (double)u - 0x1p-25, ratio = pm / (1 - pm), jmax = fmin(n, BINOM_WALK_MAX);
  double q = exp(n * log1p(-pm)), sum = q, j = 0;
  while (sum < centre && j < jmax) {
    q = q * (n - j) / (j + 1) * ratio;
    j += 1;
    sum += q;
  }
  return p <= 0.5 ? j : n - j;
}
