// One ray of Dataset.GenerateRays (Dataset.cs:111-176) and its LLFF override (Dataset.cs:268-293,
// ConvertToNdc :295-308) as device functions, shared by the record generator and the materialiser
// (raygen.hip) and by the image-backed batch gather (dataset.hip), plus the multiscale record layout
// both sides index with.  Every expression keeps the C# evaluation order in fp32; contraction is
// switched off here for the rest of the including file, so every kernel built from these functions
// produces the same bits (oracle/raygen.py).
#pragma once
#include "common.h"
#include "launch.h"

#pragma clang fp contract(off)

namespace nof {

// cameraDirs[y, x] then rotation * dir (Dataset.cs:118-141; Matrix3x3 * Vector3, MipHelpers.cs:36-40).
// P = pose: rotation row-major (Matrix3x3 _m11.._m33) then translation.
__device__ inline void pixel_dir(const float* __restrict__ P, int x, int y, int w, int h, float focal, float d[3]) {
  const float cx = ((float)x - (float)w * 0.5f + 0.5f) / focal;
  const float cy = -((float)y - (float)h * 0.5f + 0.5f) / focal;
  const float cz = -1.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = P[3 * i] * cx + P[3 * i + 1] * cy + P[3 * i + 2] * cz;
}

__device__ inline float len3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// ConvertToNdc (Dataset.cs:295-308), near = 1
__device__ inline void to_ndc(const float o_in[3], const float d[3], float focal, float w, float h, float on[3],
                              float dn[3]) {
  const float nearp = 1.0f;
  const float t = -(nearp + o_in[2]) / d[2];
  const float ox = o_in[0] + t * d[0], oy = o_in[1] + t * d[1], oz = o_in[2] + t * d[2];
  on[0] = -(2.0f * focal / w) * (ox / oz);
  on[1] = -(2.0f * focal / h) * (oy / oz);
  on[2] = 1.0f + 2.0f * nearp / oz;
  dn[0] = -(2.0f * focal / w) * (d[0] / d[2] - ox / oz);
  dn[1] = -(2.0f * focal / h) * (d[1] / d[2] - oy / oz);
  dn[2] = -2.0f * nearp / oz;
}

__device__ inline void ndc_origin(const float* __restrict__ P, int x, int y, int w, int h, float focal, float on[3]) {
  float d[3], dn[3];
  pixel_dir(P, x, y, w, h, focal, d);
  to_ndc(P + 9, d, focal, (float)w, (float)h, on, dn);
}

// The ray of pixel (x, y) of a w x h view with pose P: origin, direction, view direction, radius.
struct Ray {
  float o[3], d[3], vd[3], radius;
};
__device__ inline Ray ray_at(const float* __restrict__ P, int x, int y, int w, int h, float focal, int ndc) {
  Ray r;
  float d[3];
  pixel_dir(P, x, y, w, h, focal, d);
  const float dl = len3(d[0], d[1], d[2]);
  r.vd[0] = d[0] / dl; r.vd[1] = d[1] / dl; r.vd[2] = d[2] / dl;  // Vector3.Normalize (pre-NDC direction)
  r.o[0] = P[9]; r.o[1] = P[10]; r.o[2] = P[11];
  r.d[0] = d[0]; r.d[1] = d[1]; r.d[2] = d[2];
  if (!ndc) {  // Dataset.cs:144-152: neighbour to the right, itself in the last column (radius 0)
    const int nx = x < w - 1 ? x + 1 : x;
    float dn[3];
    pixel_dir(P, nx, y, w, h, focal, dn);
    r.radius = len3(d[0] - dn[0], d[1] - dn[1], d[2] - dn[2]) * 2.0f / sqrtf(12.0f);
  } else {  // Dataset.cs:272-289: NDC warp, radius from the NDC origins of the x / y neighbours
    float on[3], dnd[3];
    to_ndc(r.o, d, focal, (float)w, (float)h, on, dnd);
    float a[3], b[3];
    if (x < w - 1) { ndc_origin(P, x + 1, y, w, h, focal, b); a[0] = on[0]; a[1] = on[1]; a[2] = on[2]; }
    else { ndc_origin(P, x - 1, y, w, h, focal, a); b[0] = on[0]; b[1] = on[1]; b[2] = on[2]; }
    const float dx = len3(a[0] - b[0], a[1] - b[1], a[2] - b[2]);
    if (y < h - 1) { ndc_origin(P, x, y + 1, w, h, focal, b); a[0] = on[0]; a[1] = on[1]; a[2] = on[2]; }
    else { ndc_origin(P, x, y - 1, w, h, focal, a); b[0] = on[0]; b[1] = on[1]; b[2] = on[2]; }
    const float dy = len3(a[0] - b[0], a[1] - b[1], a[2] - b[2]);
    r.radius = sqrtf(dx * dx + dy * dy) / sqrtf(12.0f);
    r.o[0] = on[0]; r.o[1] = on[1]; r.o[2] = on[2];
    r.d[0] = dnd[0]; r.d[1] = dnd[1]; r.d[2] = dnd[2];
  }
  return r;
}

// Virtual record idx of a multiscale scene (launch.h MultiscaleLayout: scale-major, view-major, then
// row-major pixels) -> its view and pixel and its scale's row of the table.  The scale is found by
// walking first[]: selects over the (wave-uniform) table entries, no indexed access.
struct RecordPos {
  int v, x, y, w, h;
  float focal, lossmult;
};
__device__ inline RecordPos record_pos(const MultiscaleLayout& L, uint32_t idx) {
  RecordPos p;
  uint32_t first = 0;
  p.w = L.w[0]; p.h = L.h[0]; p.focal = L.focal[0]; p.lossmult = L.lossmult[0];
#pragma unroll
  for (int j = 1; j < kMaxScales; ++j)
    if (j < L.num_scales && (int64_t)idx >= L.first[j]) {
      first = (uint32_t)L.first[j];
      p.w = L.w[j]; p.h = L.h[j]; p.focal = L.focal[j]; p.lossmult = L.lossmult[j];
    }
  const uint32_t local = idx - first;
  const uint32_t w = (uint32_t)p.w, per = w * (uint32_t)p.h;
  const uint32_t v = local / per, pix = local - v * per;
  p.v = (int)v;
  p.y = (int)(pix / w);
  p.x = (int)(pix - (uint32_t)p.y * w);
  return p;
}

}  // namespace nof
