// The interlevel (proposal) loss of mip-NeRF 360 for gfx950 (nof_mipnerf_set_interlevel_loss): a
// coarser level's weight histogram (t^, w^: the proposal, S_c intervals) is pushed to be an upper envelope of the
// last level's (t, w: the target, S_f intervals, a constant here).  Per ray
//   bound_i = sum of w^_j over j in [lo(t_i), hi(t_{i+1})),   c(v) = #{j in 0..S_c : t^_j <= v},
//                                                             lo(v) = max(c(v) - 1, 0), hi(v) = min(c(v), S_c)
//   L_r     = sum_i max(0, w_i - bound_i)^2 / (w_i + eps),    eps = 2^-23
//   dL/dw^_j = c_r sum of g_i over i in [a_j, b_j),           g_i = -2 max(0, w_i - bound_i) / (w_i + eps)
//   a_j = #{k in 1..S_f : t_k < t^_j},  b_j = #{i in 0..S_f-1 : t_i < t^_{j+1}},  c_r = mult lossmult[r] / msum
// (bound is piecewise constant in t^: no gradient there).  One wave64 per ray, the three t / w^ rows and the prefix
// of g in LDS.  bound_i is summed directly over its own range, ascending j: as a difference of prefix sums of w^ a
// 1e-7 prefix error against a 1e-6 weight moves g_i, which is O(1) however small w_i is (2.4e-3 per tensor measured
// in an fp32 emulation); the prefix of g, whose differences only add errors relative to the sum, is harmless.
// No atomics, every sum in a fixed order: two runs give the same bits.
#include "common.h"
#include "launch.h"

namespace nof {

// #{j in [0, n) : row[j] <= v} of a sorted row
__device__ __forceinline__ int count_le(const float* row, int n, float v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// #{j in [0, n) : row[j] < v} of a sorted row
__device__ __forceinline__ int count_lt(const float* row, int n, float v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// PF = S_f / 64 consecutive target intervals per lane.  LDS (2 S_c + 2 S_f + 3 floats): tp[S_c + 1], wp[S_c],
// tf[S_f + 1], G[S_f + 1] with G[i] = sum_{i' < i} h_i', h = -g >= 0 (so a ray without an active hinge stores +0).
template <int PF>
__global__ __launch_bounds__(64) void k_interlevel(InterlevelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int Sf = 64 * PF;
  const int Sc = a.S_prop;
  const int lane = threadIdx.x;
  const int r = blockIdx.x;  // (grid = n)
  float* tp = smem;
  float* wp = tp + (Sc + 1);
  float* tf = wp + Sc;
  float* G = tf + (Sf + 1);
  const float* tpr = a.t_prop + (size_t)r * (Sc + 1);
  const float* wpr = a.w_prop + (size_t)r * Sc;
  const float* tfr = a.t_tgt + (size_t)r * (Sf + 1);
  for (int j = lane; j <= Sc; j += 64) tp[j] = tpr[j];
  for (int j = lane; j < Sc; j += 64) wp[j] = wpr[j];
  for (int k = lane; k <= Sf; k += 64) tf[k] = tfr[k];
  const int i0 = lane * PF;
  float wf[PF];
#pragma unroll
  for (int p = 0; p < PF; ++p) wf[p] = a.w_tgt[(size_t)r * Sf + i0 + p];
  __syncthreads();

  constexpr float eps = 1.1920928955078125e-07f;  // 2^-23
  float h[PF];
  float hs = 0.0f, ls = 0.0f;  // this lane's sums of h_i and of the hinge terms, ascending i
  int c0 = count_le(tp, Sc + 1, tf[i0]);
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    const int c1 = count_le(tp, Sc + 1, tf[i0 + p + 1]);
    const int lo = max(c0 - 1, 0), hi = min(c1, Sc);
    float bound = 0.0f;
    for (int j = lo; j < hi; ++j) bound += wp[j];
    const float m = fmaxf(0.0f, wf[p] - bound);
    const float den = wf[p] + eps;
    h[p] = 2.0f * m / den;
    ls += m * m / den;
    hs += h[p];
    c0 = c1;
  }
  float inc = hs;  // inclusive sum scan over lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  float run = __shfl_up(inc, 1, 64);  // sum over lanes < lane
  if (lane == 0) {
    run = 0.0f;
    G[0] = 0.0f;
  }
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    run += h[p];
    G[i0 + p + 1] = run;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ls += __shfl_xor(ls, o, 64);  // butterfly: the same bits in every lane
  const float c = a.mult * a.lossmult[r] / a.msum;
  if (a.rays && lane == 0) a.rays[r] = c * ls;
  __syncthreads();

  float* q = a.w_grad + (size_t)r * Sc;
  for (int j = lane; j < Sc; j += 64) {
    const int aj = count_lt(tf + 1, Sf, tp[j]);   // (a_j <= b_j: the rows are sorted)
    const int bj = count_lt(tf, Sf, tp[j + 1]);
    const float v = c * (G[aj] - G[bj]);          // = c_r sum of g_i over [a_j, b_j)
    q[j] = a.accumulate ? q[j] + v : v;
  }
}

hipError_t launch_interlevel(const InterlevelArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  const int Sc = a.S_prop;
  if ((Sc != 64 && Sc != 128 && Sc != 256 && Sc != 512) || !a.t_prop || !a.w_prop || !a.t_tgt || !a.w_tgt ||
      !a.lossmult || !a.w_grad || !(a.msum > 0.0f) || !(a.mult >= 0.0f))
    return hipErrorInvalidValue;
  const size_t shm = sizeof(float) * (2 * (size_t)Sc + 2 * (size_t)a.S_tgt + 3);
  const dim3 grid(a.n), block(64);
  switch (a.S_tgt) {
    case 64: hipLaunchKernelGGL(k_interlevel<1>, grid, block, shm, st, a); break;
    case 128: hipLaunchKernelGGL(k_interlevel<2>, grid, block, shm, st, a); break;
    case 256: hipLaunchKernelGGL(k_interlevel<4>, grid, block, shm, st, a); break;
    case 512: hipLaunchKernelGGL(k_interlevel<8>, grid, block, shm, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace nof
