// Device ray generation: Dataset.GenerateRays (Dataset.cs:111-176) and the
// LLFF override (Dataset.cs:268-293, ConvertToNdc :295-308), written straight into 64-byte
// BinDataset records (BinDataset.cs:40-49) in HBM, so a scene's whole training set is produced on
// the GPU from poses (+ images) and gathered by dataset.hip.
//
// One thread per pixel; neighbours' directions / NDC origins are recomputed, not exchanged.  Every
// expression keeps the C# evaluation order in fp32 and the file is compiled without FMA contraction
// (raygen.h), so records are bit-identical to the oracle (oracle/raygen.py).
//
// Multiscale scenes (the DatasetType.Multicam loader the reference declares, TrainState.cs:41, and
// never builds, Dataset.cs:203-207): the image pyramid, and the materialiser that writes every
// virtual record of such a scene through the same per-ray function.
#include "raygen.h"

namespace nof {

__device__ inline void store_record(float* __restrict__ rec, const Ray& r, float near, float far, float lossmult,
                                    const float* __restrict__ px) {
  float4* q = reinterpret_cast<float4*>(rec);
  q[0] = make_float4(r.o[0], r.o[1], r.o[2], r.d[0]);
  q[1] = make_float4(r.d[1], r.d[2], r.vd[0], r.vd[1]);
  q[2] = make_float4(r.vd[2], r.radius, near, far);
  q[3] = make_float4(lossmult, px ? px[0] : 0.0f, px ? px[1] : 0.0f, px ? px[2] : 0.0f);
}

__global__ __launch_bounds__(256) void k_generate_rays(const float* __restrict__ poses, int V, int w, int h,
                                                       float focal, float near, float far, int ndc,
                                                       const float* __restrict__ images, float* __restrict__ rec) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)w * h;
  if (g >= per * V) return;
  const int v = (int)(g / per), p = (int)(g - (int64_t)v * per);
  const int y = p / w, x = p - y * w;
  const Ray r = ray_at(poses + 12 * v, x, y, w, h, focal, ndc);
  store_record(rec + g * 16, r, near, far, 1.0f, images ? images + g * 3 : nullptr);  // LossMult = 1
}

hipError_t launch_generate_rays(const float* poses, int V, int w, int h, float focal, float near, float far, int ndc,
                                const float* images, float* records, hipStream_t st) {
  const int64_t n = (int64_t)V * w * h;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_generate_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, poses, V, w, h, focal,
                     near, far, ndc, images, records);
  return hipGetLastError();
}

// One thread per output pixel of level s: V views of w x h from V views of 2w x 2h, all three channels.
__global__ __launch_bounds__(256) void k_pyramid_level(const float* __restrict__ src, float* __restrict__ dst,
                                                       int64_t n, int w, int h) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const int64_t per = (int64_t)w * h;
  const int64_t v = g / per;
  const int p = (int)(g - v * per);
  const int y = p / w, x = p - y * w;
  const float* a = src + ((v * 2 * h + 2 * y) * (2 * (int64_t)w) + 2 * x) * 3;  // (2y, 2x); b follows it
  const float* c = a + 2 * (int64_t)w * 3;                                    // (2y + 1, 2x); d follows it
#pragma unroll
  for (int k = 0; k < 3; ++k) dst[g * 3 + k] = ((a[k] + a[3 + k]) + (c[k] + c[3 + k])) * 0.25f;
}

hipError_t launch_pyramid_level(float* pyr, const MultiscaleLayout& L, int s, hipStream_t st) {
  if (s < 1 || s >= L.num_scales) return hipErrorInvalidValue;
  const int64_t n = (int64_t)L.num_views * L.w[s] * L.h[s];
  hipLaunchKernelGGL(k_pyramid_level, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pyr + L.first[s - 1] * 3,
                     pyr + L.first[s] * 3, n, L.w[s], L.h[s]);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_materialize(const float* __restrict__ poses, const float* __restrict__ pyr,
                                                     MultiscaleLayout L, float near, float far, int ndc,
                                                     float* __restrict__ rec) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= L.count) return;
  const RecordPos p = record_pos(L, (uint32_t)g);
  const Ray r = ray_at(poses + 12 * p.v, p.x, p.y, p.w, p.h, p.focal, ndc);
  store_record(rec + g * 16, r, near, far, p.lossmult, pyr ? pyr + g * 3 : nullptr);
}

hipError_t launch_materialize(const float* poses, const float* pyr, const MultiscaleLayout& L, float near, float far,
                              int ndc, float* records, hipStream_t st) {
  if (L.count <= 0 || L.count > 0xFFFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_materialize, dim3((unsigned)((L.count + 255) / 256)), dim3(256), 0, st, poses, pyr, L, near,
                     far, ndc, records);
  return hipGetLastError();
}

}  // namespace nof
