// Ray-batch ingestion on the device (BinDataset.cs:10-53).
//
// The reference seeks into the record file 1024 times per step (BinDataset.LoadBatch), drawing each
// record with System.Random.Next(numSamples) (with replacement).  Here the whole record set is
// resident in HBM and a batch is one gather launch: record index of global ray g at step s =
// (x * count) >> 32 with x = word 0 of Philox4x32-10(ctr = {0, g, stream 4 << 16, s}, key = seed)
// (D2: Philox replaces the unseeded System.Random), so a sharded batch draws the same records as the
// whole batch.  One thread per (ray, 16-B quarter of its 64-B record): coalesced 64-B record reads,
// SoA writes.  The loss-multiplier sum is a fixed-order block reduction (deterministic).
//
// An image-backed scene (include/nof.h nof_dataset_from_images) holds no records: its gather,
// k_gather_rays, draws the same indices and generates each drawn record from its pose and its pixel
// of the image pyramid with raygen.h's per-ray function, one thread per ray.
#include "raygen.h"

namespace nof {

enum : uint32_t { kStreamBatch = 4 };

__device__ inline uint32_t batch_record(uint64_t seed, uint32_t step, uint32_t gray, int64_t count) {
  uint32_t c[4] = {0u, gray, kStreamBatch << 16, step};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (uint32_t)(((uint64_t)c[0] * (uint64_t)count) >> 32);
}

__global__ __launch_bounds__(256) void k_gather_batch(const float4* __restrict__ rec, int64_t count, int n,
                                                      uint64_t seed, uint32_t step, uint32_t ray_base,
                                                      float* __restrict__ o, float* __restrict__ d,
                                                      float* __restrict__ vd, float* __restrict__ radius,
                                                      float* __restrict__ near, float* __restrict__ far,
                                                      float* __restrict__ lm, float* __restrict__ pix,
                                                      int* __restrict__ idx_out, int staged) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = g >> 2, q = g & 3;
  if (r >= n) return;
  const uint32_t idx = batch_record(seed, step, ray_base + (uint32_t)r, count);
  NOF_DCHECK((int64_t)idx < count, kChkGather);
  // staged (streaming datasets): the host already fetched ray r's record into slot r
  const float4 v = rec[(staged ? (size_t)r : (size_t)idx) * 4 + q];  // floats 4q .. 4q+3 (BinDataset.cs:40-49)
  switch (q) {
    case 0:  // origin xyz, direction x
      o[3 * r] = v.x; o[3 * r + 1] = v.y; o[3 * r + 2] = v.z; d[3 * r] = v.w;
      if (idx_out) idx_out[r] = (int)idx;
      break;
    case 1:  // direction yz, viewdir xy
      d[3 * r + 1] = v.x; d[3 * r + 2] = v.y; vd[3 * r] = v.z; vd[3 * r + 1] = v.w;
      break;
    case 2:  // viewdir z, radius, near, far
      vd[3 * r + 2] = v.x; radius[r] = v.y; near[r] = v.z; far[r] = v.w;
      break;
    default:  // lossmult, rgb
      lm[r] = v.x; pix[3 * r] = v.y; pix[3 * r + 1] = v.z; pix[3 * r + 2] = v.w;
      break;
  }
}

// Rays per block of k_gather_rays.  A batch is small (1024 rays) and a ray is a dependent chain of pose
// loads, divides and square roots, so one wave per block spreads the batch over the most CUs
// (DESIGN.md has the measurement against 256).
#ifndef NOF_GATHER_RAYS_BLOCK
#define NOF_GATHER_RAYS_BLOCK 64
#endif
constexpr int kGatherRaysBlock = NOF_GATHER_RAYS_BLOCK;

__global__ __launch_bounds__(kGatherRaysBlock) void k_gather_rays(
    const float* __restrict__ poses, const float* __restrict__ pyr, MultiscaleLayout L, float near_, float far_,
    int ndc, int n, uint64_t seed, uint32_t step, uint32_t ray_base, float* __restrict__ o, float* __restrict__ d,
    float* __restrict__ vd, float* __restrict__ radius, float* __restrict__ near, float* __restrict__ far,
    float* __restrict__ lm, float* __restrict__ pix, int* __restrict__ idx_out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t idx = batch_record(seed, step, ray_base + (uint32_t)r, L.count);
  const RecordPos p = record_pos(L, idx);
  NOF_DCHECK((int64_t)idx < L.count && p.v < L.num_views && p.x < p.w && p.y < p.h, kChkGather);
  const Ray ray = ray_at(poses + 12 * p.v, p.x, p.y, p.w, p.h, p.focal, ndc);
  const float* px = pyr ? pyr + (int64_t)idx * 3 : nullptr;  // the pyramid is stored in record order
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[3 * r + k] = ray.o[k]; d[3 * r + k] = ray.d[k]; vd[3 * r + k] = ray.vd[k];
    pix[3 * r + k] = px ? px[k] : 0.0f;
  }
  radius[r] = ray.radius; near[r] = near_; far[r] = far_; lm[r] = p.lossmult;
  if (idx_out) idx_out[r] = (int)idx;
}

__global__ __launch_bounds__(1024) void k_sum(const float* __restrict__ x, int n, float* __restrict__ out) {
  __shared__ float red[1024];
  float s = 0.0f;
  for (int i = threadIdx.x; i < n; i += 1024) s += x[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}

uint32_t batch_record_host(uint64_t seed, uint32_t step, uint32_t gray, int64_t count) {
  uint32_t c[4] = {0u, gray, kStreamBatch << 16, step};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (uint32_t)(((uint64_t)c[0] * (uint64_t)count) >> 32);
}

hipError_t launch_gather_batch(const float* records, int64_t count, int n, uint64_t seed, uint32_t step,
                               uint32_t ray_base, float* o, float* d, float* vd, float* radius, float* near,
                               float* far, float* lm, float* pix, int* idx_out, float* lm_sum, hipStream_t st,
                               int staged) {
  if (n <= 0) return hipSuccess;
  if (count <= 0 || count > 0xFFFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gather_batch, dim3((4 * n + 255) / 256), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(records), count, n, seed, step, ray_base, o, d, vd, radius,
                     near, far, lm, pix, idx_out, staged);
  if (lm_sum) hipLaunchKernelGGL(k_sum, dim3(1), dim3(1024), 0, st, lm, n, lm_sum);
  return hipGetLastError();
}

hipError_t launch_gather_rays(const float* poses, const float* pyr, const MultiscaleLayout& L, float near, float far,
                              int ndc, int n, uint64_t seed, uint32_t step, uint32_t ray_base, float* o, float* d,
                              float* vd, float* radius, float* nears, float* fars, float* lm, float* pix, int* idx_out,
                              float* lm_sum, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (L.count <= 0 || L.count > 0xFFFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gather_rays, dim3((n + kGatherRaysBlock - 1) / kGatherRaysBlock), dim3(kGatherRaysBlock), 0,
                     st, poses, pyr, L, near, far, ndc, n, seed, step, ray_base, o, d, vd, radius, nears, fars, lm,
                     pix, idx_out);
  if (lm_sum) hipLaunchKernelGGL(k_sum, dim3(1), dim3(1024), 0, st, lm, n, lm_sum);
  return hipGetLastError();
}

// Pose gradients of an image-backed batch (ndc = 0): ray_at gives o = P[9..11], d_i = sum_c P[3 i + c] cam_c with
// cam = pixel_dir's (cx, cy, cz) at the ray's own scale, so dL/dP[9 + i] = sum dL/do_i and dL/dP[3 i + c] =
// sum dL/dd_i cam_c over the view's rays.  One workgroup per view scans the batch's n record indices (O(V n) index
// reads: nothing next to a step); thread t keeps the view's rays t, t + 256, ... in ray order in 12 accumulators,
// then a fixed tree.  No atomics: bitwise repeatable.
constexpr int kPoseGradThreads = 256;
__global__ __launch_bounds__(kPoseGradThreads) void k_pose_grad(MultiscaleLayout L, int n, const int* __restrict__ idx,
                                                                const float* __restrict__ og,
                                                                const float* __restrict__ dg,
                                                                float* __restrict__ pose_grad, int accumulate) {
  __shared__ float red[13][kPoseGradThreads];
  const int v = blockIdx.x, tid = threadIdx.x;
  float acc[13];
#pragma unroll
  for (int k = 0; k < 13; ++k) acc[k] = 0.0f;
  for (int r = tid; r < n; r += kPoseGradThreads) {
    const RecordPos p = record_pos(L, (uint32_t)idx[r]);
    if (p.v != v) continue;
    const float cam[3] = {((float)p.x - (float)p.w * 0.5f + 0.5f) / p.focal,
                          -((float)p.y - (float)p.h * 0.5f + 0.5f) / p.focal, -1.0f};  // pixel_dir's
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float gd = dg[3 * r + i];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[3 * i + c] += gd * cam[c];
      acc[9 + i] += og[3 * r + i];
    }
    acc[12] += 1.0f;  // (the view's ray count: an empty view leaves an accumulated row as it is)
  }
#pragma unroll
  for (int k = 0; k < 13; ++k) red[k][tid] = acc[k];
  __syncthreads();
  for (int o = kPoseGradThreads / 2; o > 0; o >>= 1) {
    if (tid < o)
#pragma unroll
      for (int k = 0; k < 13; ++k) red[k][tid] += red[k][tid + o];
    __syncthreads();
  }
  if (tid < 12) {
    float* dst = pose_grad + 12 * (size_t)v + tid;
    if (!accumulate) *dst = red[tid][0];
    else if (red[12][0] > 0.0f) *dst = *dst + red[tid][0];
  }
}

hipError_t launch_pose_grad(const MultiscaleLayout& L, int n, const int* idx, const float* o_grad, const float* d_grad,
                            float* pose_grad, int accumulate, hipStream_t st) {
  if (L.num_views <= 0 || n < 0 || !idx || !o_grad || !d_grad || !pose_grad) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pose_grad, dim3(L.num_views), dim3(kPoseGradThreads), 0, st, L, n, idx, o_grad, d_grad,
                     pose_grad, accumulate);
  return hipGetLastError();
}

// The view of each ray of a batch (the appearance embeddings' row ids): record_pos of its record index.
__global__ __launch_bounds__(256) void k_batch_views(MultiscaleLayout L, int n, const int* __restrict__ idx,
                                                     int* __restrict__ views) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const RecordPos p = record_pos(L, (uint32_t)idx[r]);
  NOF_DCHECK(p.v >= 0 && p.v < L.num_views, kChkGather);
  views[r] = p.v;
}

hipError_t launch_batch_views(const MultiscaleLayout& L, int n, const int* idx, int* views, hipStream_t st) {
  if (L.num_views <= 0 || n < 0 || !idx || !views) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_batch_views, dim3((n + 255) / 256), dim3(256), 0, st, L, n, idx, views);
  return hipGetLastError();
}

// fails kChkSelfTest on purpose: proves a checked build's plumbing (nof_device_checks_selftest)
__global__ void k_check_selftest(int zero) { NOF_DCHECK(zero != 0, kChkSelfTest); }
hipError_t launch_check_selftest(hipStream_t st) {
  hipLaunchKernelGGL(k_check_selftest, dim3(1), dim3(64), 0, st, 0);
  return hipGetLastError();
}
NOF_CHECK_UNIT(check_unit_dataset)

}  // namespace nof
