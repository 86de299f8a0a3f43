// Per-view appearance embeddings on the any-shape path (include/nof.h nof_mipnerf_create_ex).
//
// The view layer's per-ray operand grows by G columns read from a [V][G] fp32 table by each ray's view id:
//   * k_appearance_gather writes edx [n][Vd + G] = [enc_dir row | E[id]] once per level's forward (a ray whose id
//     lies outside [0, V) reads zeros: the table is never read out of bounds);
//   * k_appearance_grad sums dApp [n][G] = gray W_view[:, W + Vd :] per view into dE [V][G], k_pose_grad's scheme
//     (dataset.hip): one workgroup per view, thread t keeps the view's rays t, t + 256, ... in ray order, then a
//     fixed tree.  No atomics: bitwise repeatable.  `partial` (optional) is added to the view's sum before it meets
//     the table: a step sums its levels in a buffer of its own and the last level's launch adds that once, so two
//     accumulated steps of one batch give exactly twice its dE.
// Both are a few hundred KB of traffic next to a step's GEMMs: plain coalesced loads and stores, no LDS staging
// but the reduction tree.
#include "common.h"
#include "launch.h"

namespace nof {

constexpr int kAppThreads = 256;

__global__ __launch_bounds__(kAppThreads) void k_appearance_gather(int n, int vd, int dim, int views,
                                                                   const float* __restrict__ enc_dir,
                                                                   const float* __restrict__ table,
                                                                   const int* __restrict__ ids, int const_view,
                                                                   float* __restrict__ out) {
  const int K = vd + dim;
  const int64_t i = (int64_t)blockIdx.x * kAppThreads + threadIdx.x;  // element (r, c) of out, row-major
  if (i >= (int64_t)n * K) return;
  const int r = (int)(i / K), c = (int)(i - (int64_t)r * K);
  float v;
  if (c < vd) {
    v = enc_dir[(int64_t)r * vd + c];
  } else {
    const int id = ids ? ids[r] : const_view;  // (const_view = -1: the neutral, zero appearance)
    const bool ok = id >= 0 && id < views;
    NOF_DCHECK(!ids || ok, kChkGather);
    v = ok ? table[(int64_t)id * dim + (c - vd)] : 0.0f;
  }
  out[i] = v;
}

// accumulators per pass over the view ids: dim > kAppChunk takes ceil(dim / kAppChunk) passes
constexpr int kAppChunk = 8;

__global__ __launch_bounds__(kAppThreads) void k_appearance_grad(int n, int dim, const int* __restrict__ ids,
                                                                 const float* __restrict__ d_app,
                                                                 const float* __restrict__ partial,
                                                                 float* __restrict__ d_table, int accumulate) {
  __shared__ float red[kAppChunk + 1][kAppThreads];
  const int v = blockIdx.x, tid = threadIdx.x;
  for (int g0 = 0; g0 < dim; g0 += kAppChunk) {
    float acc[kAppChunk + 1];
#pragma unroll
    for (int k = 0; k <= kAppChunk; ++k) acc[k] = 0.0f;
    for (int r = tid; r < n; r += kAppThreads) {
      if (ids[r] != v) continue;
      const float* row = d_app + (int64_t)r * dim + g0;
#pragma unroll
      for (int k = 0; k < kAppChunk; ++k)
        if (g0 + k < dim) acc[k] += row[k];
      acc[kAppChunk] += 1.0f;  // (the view's ray count: an empty view leaves an accumulated row as it is)
    }
#pragma unroll
    for (int k = 0; k <= kAppChunk; ++k) red[k][tid] = acc[k];
    __syncthreads();
    for (int o = kAppThreads / 2; o > 0; o >>= 1) {
      if (tid < o)
#pragma unroll
        for (int k = 0; k <= kAppChunk; ++k) red[k][tid] += red[k][tid + o];
      __syncthreads();
    }
    if (tid < kAppChunk && g0 + tid < dim) {
      const int64_t e = (int64_t)v * dim + g0 + tid;
      const float sum = partial ? partial[e] + red[tid][0] : red[tid][0];
      if (!accumulate) d_table[e] = sum;
      else if (red[kAppChunk][0] > 0.0f) d_table[e] = d_table[e] + sum;
    }
    __syncthreads();  // (the next pass rewrites red)
  }
}

hipError_t launch_appearance_gather(int n, int vd, int dim, int views, const float* enc_dir, const float* table,
                                    const int* ids, int const_view, float* out, hipStream_t st) {
  if (n < 0 || vd < 0 || dim < 0 || views < 0 || !out || (vd > 0 && !enc_dir) || (dim > 0 && views > 0 && !table))
    return hipErrorInvalidValue;
  const int64_t total = (int64_t)n * (vd + dim);
  if (total == 0) return hipSuccess;
  const int64_t blocks = (total + kAppThreads - 1) / kAppThreads;
  if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_appearance_gather, dim3((unsigned)blocks), dim3(kAppThreads), 0, st, n, vd, dim, views, enc_dir,
                     table, ids, const_view, out);
  return hipGetLastError();
}

hipError_t launch_appearance_grad(int n, int dim, int views, const int* ids, const float* d_app, const float* partial,
                                  float* d_table, int accumulate, hipStream_t st) {
  if (n < 0 || dim <= 0 || views <= 0 || !d_table || (n > 0 && (!ids || !d_app))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_appearance_grad, dim3(views), dim3(kAppThreads), 0, st, n, dim, ids, d_app, partial,
                     d_table, accumulate);
  return hipGetLastError();
}

NOF_CHECK_UNIT(check_unit_appearance)

}  // namespace nof
