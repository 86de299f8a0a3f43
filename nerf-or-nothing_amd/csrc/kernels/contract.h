// Scene contraction for unbounded scenes (nof_mipnerf_set_contraction): mip-NeRF 360's map of space
// into the ball of radius 2,
//   contract(x) = x                       |x| <= 1
//               = (2 - 1 / |x|) x / |x|   |x| >  1,
// applied to a sample's Gaussian with the covariance linearised, cov' = J cov J^T, and kept diagonal as mip-NeRF's
// IPE is: v' = diag(J diag(v) J^T) with
//   J = a (I - u u^T) + b u u^T,  u = m / n,  n = |m|,  a = (2 n - 1) / n^2,  b = 1 / n^2.
// With c = b - a = -2 (n - 1) / n^2 (formed without a subtraction of a and b), q_j = u_j^2 and sum_j q_j = 1:
//   J_ii = a + c q_i = a (q_{i+1} + q_{i+2}) + b q_i,   J_ik = c u_i u_k,
//   v'_i = J_ii^2 v_i + c^2 q_i (q_{i+1} v_{i+1} + q_{i+2} v_{i+2}):
// non-negative terms only.  (The expansion a^2 v_i + 2 a c q_i v_i + c^2 q_i sum_k q_k v_k cancels along the radial
// axis, a relative error of eps n^2.)  The forward's operation order is a bit-exactness contract (tests restate it
// in fp32 numpy): contraction off, correctly rounded division and square root.
#pragma once
#include "common.h"

namespace nof {

// (mean, cov) of frustum_gaussian -> the contracted Gaussian, in place.  !(|m|^2 > 1), NaN included: untouched.
__device__ __forceinline__ void contract_gaussian(float m[3], float v[3]) {
#pragma clang fp contract(off)
  const float n2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
  if (!(n2 > 1.0f)) return;
  const float n = sqrtf(n2);
  const float inv = 1.0f / n;
  const float b = inv * inv;
  const float a = (2.0f * n - 1.0f) * b;
  const float c = -2.0f * (n - 1.0f) * b;
  const float u[3] = {m[0] * inv, m[1] * inv, m[2] * inv};
  const float q[3] = {u[0] * u[0], u[1] * u[1], u[2] * u[2]};
  const float v0[3] = {v[0], v[1], v[2]};
  const float cc = c * c;
  const float ms = 2.0f - inv;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    const float D = a * (q[i1] + q[i2]) + b * q[i];
    m[i] = ms * u[i];
    v[i] = (D * D) * v0[i] + (cc * q[i]) * (q[i1] * v0[i1] + q[i2] * v0[i2]);
  }
}

// The adjoint at the uncontracted (m, v): (dL/dm', dL/dv') -> (dL/dm, dL/dv), in place.  The branch is held at its
// forward decision (the map is C^1 at n = 1: J = I there).
//   dv_k = J_kk^2 dv'_k + c^2 q_k sum_{i != k} q_i dv'_i
//   dm_k = a dm'_k + c u_k (u . dm')  +  Gn u_k + (Gu_k - u_k (u . Gu)) / n
// with Gn = sum_i dv'_i dv'_i/dn (a' = 2 (1 - n) / n^3, b' = -2 / n^3, c' = b' - a' = 2 (n - 2) / n^3) and
// Gu_j = 2 u_j sum_i dv'_i dv'_i/dq_j (dJ_ii/dq_j = c delta_ij), through dn/dm_k = u_k and
// du_i/dm_k = (delta_ik - u_i u_k) / n.
__device__ __forceinline__ void contract_adjoint(const float m[3], const float v[3], float dm[3], float dv[3]) {
  const float n2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
  if (!(n2 > 1.0f)) return;
  const float n = sqrtf(n2);
  const float inv = 1.0f / n;
  const float b = inv * inv;
  const float a = (2.0f * n - 1.0f) * b;
  const float c = -2.0f * (n - 1.0f) * b;
  const float inv3 = b * inv;
  const float da = -2.0f * (n - 1.0f) * inv3, db = -2.0f * inv3, dc = 2.0f * (n - 2.0f) * inv3;
  const float u[3] = {m[0] * inv, m[1] * inv, m[2] * inv};
  const float q[3] = {u[0] * u[0], u[1] * u[1], u[2] * u[2]};
  const float gm[3] = {dm[0], dm[1], dm[2]};
  const float gv[3] = {dv[0], dv[1], dv[2]};
  const float cc = c * c;
  float D[3], E[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    D[i] = a * (q[i1] + q[i2]) + b * q[i];
    E[i] = q[i1] * v[i1] + q[i2] * v[i2];
  }
  float Gn = 0.0f, Gu[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    Gn += gv[i] * (2.0f * D[i] * v[i] * (da * (q[i1] + q[i2]) + db * q[i]) + 2.0f * c * dc * q[i] * E[i]);
    const float gq = c * (gv[i] * (2.0f * D[i] * v[i] + c * E[i]) + c * v[i] * (gv[i1] * q[i1] + gv[i2] * q[i2]));
    Gu[i] = 2.0f * u[i] * gq;
    dv[i] = (D[i] * D[i]) * gv[i] + (cc * q[i]) * (q[i1] * gv[i1] + q[i2] * gv[i2]);
  }
  const float ugm = (u[0] * gm[0] + u[1] * gm[1]) + u[2] * gm[2];
  const float ugu = (u[0] * Gu[0] + u[1] * Gu[1]) + u[2] * Gu[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) dm[k] = (a * gm[k] + c * u[k] * ugm) + (Gn * u[k] + (Gu[k] - u[k] * ugu) * inv);
}

}  // namespace nof
