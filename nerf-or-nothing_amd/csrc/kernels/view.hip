// The test split on the device (include/nof.h nof_dataset_render_view): the reference declares it
// (Split.Test, Dataset.cs:13-17) and leaves it empty (TestInit throws, Dataset.cs:107-110).  A whole
// view of an image-backed scene, at one of its scales, is rendered chunk by chunk with no host round
// trip: per chunk k_view_rays -> the inference forward and the integrator (AcceleratedMipNeRF::Render)
// -> k_view_store; after the last chunk k_view_final.
//
//   k_view_rays   the rays of pixels [p0, p0 + n) of the view, row-major, from its pose (the dataset's
//                 pose table, or 12 floats in the kernel arguments) with raygen.h's per-ray function and
//                 the scale's width, height and focal length: the bits nof_dataset_materialize writes
//                 for that view and scale (raygen.h switches contraction off for this file too).
//   k_view_store  every level's comp_rgb chunk and the last level's distance / acc into the caller's
//                 images at pixel p0 (null images skipped) and, when the view is scored, each level's
//                 squared error against the pyramid slice of (scale, view): per channel d = C - p and
//                 d * d in fp32, added in fp64 in channel order per pixel, then a fixed-order tree over
//                 the block -> one partial per (level, block of the view).
//   k_view_final  one block adds each level's partials in a fixed order.  No atomics anywhere, so a
//                 score is bit-identical from run to run.
#include "raygen.h"

namespace nof {

constexpr int kViewRaysBlock = 64;  // as k_gather_rays (dataset.hip): a chunk is small, a ray a dependent chain

__global__ __launch_bounds__(kViewRaysBlock) void k_view_rays(ViewRayArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  NOF_DCHECK(a.p0 >= 0 && a.n >= 0 && (int64_t)a.p0 + a.n <= (int64_t)a.w * a.h, kChkGather);
  NOF_DCHECK(a.use_pose || (a.view >= 0 && a.view < a.num_views), kChkGather);
  if (r >= a.n) return;
  float P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = a.use_pose ? a.pose[k] : a.poses[12 * (int64_t)a.view + k];
  const int p = a.p0 + r;
  const int y = p / a.w, x = p - y * a.w;
  const Ray ray = ray_at(P, x, y, a.w, a.h, a.focal, a.ndc);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.o[3 * r + k] = ray.o[k];
    a.d[3 * r + k] = ray.d[k];
  }
  a.radius[r] = ray.radius;
  a.nears[r] = a.near;
  a.fars[r] = a.far;
}

hipError_t launch_view_rays(const ViewRayArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (a.w <= 0 || a.h <= 0 || a.p0 < 0 || (int64_t)a.p0 + a.n > (int64_t)a.w * a.h) return hipErrorInvalidValue;
  if (!a.use_pose && (!a.poses || a.view < 0 || a.view >= a.num_views)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_view_rays, dim3((a.n + kViewRaysBlock - 1) / kViewRaysBlock), dim3(kViewRaysBlock), 0, st, a);
  return hipGetLastError();
}

__global__ __launch_bounds__(kViewStoreBlock) void k_view_store(ViewStoreArgs a) {
  __shared__ double red[kViewMaxLevels][kViewStoreBlock];
  const int r = blockIdx.x * kViewStoreBlock + threadIdx.x;
  NOF_DCHECK(a.p0 >= 0 && a.n >= 0 && (int64_t)a.p0 + a.n <= (int64_t)a.npix, kChkGather);
  NOF_DCHECK(a.view >= 0 && a.view < a.num_views, kChkGather);
  NOF_DCHECK(!a.partials || a.block0 + (int)gridDim.x <= a.blocks, kChkGather);
  const bool live = r < a.n;
  const int64_t p = (int64_t)a.p0 + r;
  float g[3] = {0.0f, 0.0f, 0.0f};
  if (live && a.gt) {
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = a.gt[3 * p + k];
  }
#pragma unroll
  for (int l = 0; l < kViewMaxLevels; ++l) {
    double se = 0.0;
    if (l < a.num_levels && live) {
      float c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = a.comp_rgb[l][3 * r + k];
      if (a.rgb[l]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.rgb[l][3 * p + k] = c[k];
      }
      if (a.gt) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float d = c[k] - g[k];
          se += (double)(d * d);
        }
      }
    }
    red[l][threadIdx.x] = se;
  }
  if (live) {
    if (a.distance) a.distance[p] = a.dist_in[r];
    if (a.acc) a.acc[p] = a.acc_in[r];
  }
  if (!a.partials) return;  // uniform: not scored
  __syncthreads();
  for (int o = kViewStoreBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int l = 0; l < kViewMaxLevels; ++l) red[l][threadIdx.x] += red[l][threadIdx.x + o];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < a.num_levels) {  // level l's partials: [l][blocks of the view]
    double v = red[0][0];
#pragma unroll
    for (int l = 1; l < kViewMaxLevels; ++l)
      if ((int)threadIdx.x == l) v = red[l][0];
    a.partials[(int64_t)threadIdx.x * a.blocks + a.block0 + blockIdx.x] = v;
  }
}

hipError_t launch_view_store(const ViewStoreArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  const int grid = view_store_blocks(a.n);
  if (a.num_levels < 1 || a.num_levels > kViewMaxLevels || a.p0 < 0 || (int64_t)a.p0 + a.n > (int64_t)a.npix ||
      a.view < 0 || a.view >= a.num_views)
    return hipErrorInvalidValue;
  if ((a.partials != nullptr) != (a.gt != nullptr)) return hipErrorInvalidValue;
  if (a.partials && (a.block0 < 0 || a.block0 + grid > a.blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_view_store, dim3(grid), dim3(kViewStoreBlock), 0, st, a);
  return hipGetLastError();
}

// sums[l] = partials[l][0 .. blocks) added in a fixed order: a strided pass per thread, then a tree
__global__ __launch_bounds__(256) void k_view_final(const double* __restrict__ partials, int blocks, int num_levels,
                                                    double* __restrict__ sums) {
  __shared__ double red[256];
  for (int l = 0; l < num_levels; ++l) {
    double s = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) s += partials[(int64_t)l * blocks + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) sums[l] = red[0];
    __syncthreads();
  }
}

hipError_t launch_view_final(const double* partials, int blocks, int num_levels, double* sums, hipStream_t st) {
  if (!partials || !sums || blocks <= 0 || num_levels < 1 || num_levels > kViewMaxLevels) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_view_final, dim3(1), dim3(256), 0, st, partials, blocks, num_levels, sums);
  return hipGetLastError();
}
NOF_CHECK_UNIT(check_unit_view)

}  // namespace nof
