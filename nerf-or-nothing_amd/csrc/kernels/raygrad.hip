// Ray gradients (nof_mipnerf_set_ray_grad): dL/d(origin) and dL/d(direction) of every ray of a step,
// the last link of the chain dL/dEnc -> (dL/dmean, dL/dcov) -> (dL/do, dL/dd) that camera refinement needs.  One
// adjoint kernel for gfx950, k_ray_grad, per level:
//   mean_j = d_j tmean + o_j,  cov_j = tvar d_j^2 + rvar (1 - d_j^2 / D),  D = max(1e-10, |d|^2)   (geometry.h)
//   alpha  = 1 - exp(-sigma delta |d|)                                                              (render.hip)
//   view PE of the unnormalised d                                                                   (dir_feature)
// Constants of the derivative: radius, near, far, every t-value, the Philox uniforms.  (dm, dc) per sample are formed
// exactly as k_encode_grad forms them (crosslevel.hip: the stored encoding and dL/dEnc streamed, no transcendental,
// the stored cos phase's rounding corrected to first order).  No float atomics: every sum runs in a fixed order, two
// runs give the same bits.
#include "common.h"
#include "contract.h"
#include "geometry.h"
#include "launch.h"

namespace nof {

constexpr int kRgChunk = 32;     // samples staged per pass
constexpr int kRgThreads = 256;  // 8 threads per staged sample
constexpr int kRgTerms = 7;      // per sample: dL/do (3), the frustum's share of dL/dd (3), dsigma sigma (1)

// (tmean, tvar, rvar) of one sample: the forward's expressions (geometry.h frustum_gaussian), which keeps them local
__device__ __forceinline__ void frustum_moments(float t0, float t1, float radius, bool cylinder, float* tmean,
                                                float* tvar, float* rvar) {
#pragma clang fp contract(off)
  if (cylinder) {
    *tmean = (t0 + t1) / 2.0f;
    *rvar = radius * radius / 4.0f;
    *tvar = (t1 - t0) * (t1 - t0) / 12.0f;
    return;
  }
  const float mu = (t0 + t1) / 2.0f;
  const float hw = (t1 - t0) / 2.0f;
  const float mu2 = mu * mu;
  const float hw2 = hw * hw;
  const float den = 3.0f * mu2 + hw2;
  *tmean = mu + (2.0f * mu * hw2) / den;
  *tvar = hw2 / 3.0f - (4.0f / 15.0f) * (hw2 * hw2 * (12.0f * mu2 - hw2)) / (den * den);
  *rvar = radius * radius * (mu2 / 4.0f + (5.0f / 12.0f) * hw2 - (4.0f / 15.0f) * (hw2 * hw2) / den);
}

// One workgroup per ray.  Per pass, 32 samples' rows of enc and dEnc go to LDS by 16-byte coalesced loads (the ray's
// S P floats start 16-byte aligned: S is a multiple of 32, P of 6); 8 threads per sample take the degrees q, q + 8,
// ... and a fixed butterfly adds their partial sums; the sample's 7 terms go to LDS.  Then 7 groups of 32 lanes sum
// the S samples' terms (lane l: samples l, l + 32, ... in order, then a fixed butterfly), and three threads add the
// integrator's |d| term and the view encoding's and write the ray's six floats.
template <bool CONTRACT>
__global__ __launch_bounds__(kRgThreads) void k_ray_grad(RayGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float s_sum[8];
  const int S = a.S, P = a.P, ndeg = P / 6;
  float* se = smem;                      // [32][P]
  float* sg = smem + kRgChunk * P;       // [32][P]
  float* sx = smem + 2 * kRgChunk * P;   // [7][S]
  const int r = blockIdx.x, tid = threadIdx.x;
  const float d0 = a.d[3 * r], d1 = a.d[3 * r + 1], d2 = a.d[3 * r + 2];
  const float dms = fmaxf(1e-10f, (d0 * d0 + d1 * d1) + d2 * d2);
  const float dd[3] = {d0 * d0, d1 * d1, d2 * d2};
  const float dv[3] = {d0, d1, d2};
  const float oo[3] = {a.o[3 * r], a.o[3 * r + 1], a.o[3 * r + 2]};
  const float radius = a.radius[r];
  const float* tr = a.t + (size_t)r * (S + 1);
  const int n4 = kRgChunk * P / 4;  // (32 P is a multiple of 4)
  for (int c0 = 0; c0 < S; c0 += kRgChunk) {
    const size_t base = ((size_t)r * S + c0) * P;
    const f32x4* ge = reinterpret_cast<const f32x4*>(a.enc + base);
    const f32x4* gg = reinterpret_cast<const f32x4*>(a.denc + base);
    for (int i = tid; i < n4; i += kRgThreads) {
      reinterpret_cast<f32x4*>(se)[i] = ge[i];
      reinterpret_cast<f32x4*>(sg)[i] = gg[i];
    }
    __syncthreads();
    const int ls = tid >> 3, q = tid & 7;
    const float* e = se + ls * P;
    const float* g = sg + ls * P;
    float dm[3] = {0.0f, 0.0f, 0.0f}, dc[3] = {0.0f, 0.0f, 0.0f};
    // the sample's mean, bit for bit the forward's: kappa, the rounding of the stored cos phase (k_encode_grad)
    float mu[3], cv[3];
    const float t0 = tr[c0 + ls], t1 = tr[c0 + ls + 1];
    frustum_gaussian(t0, t1, oo, dv, radius, mu, cv, a.cylinder != 0);
    // CONTRACT: kappa's y is the contracted mean's; the map's adjoint below is taken at the uncontracted Gaussian
    float m0[3], v0[3];
    if constexpr (CONTRACT) {
#pragma unroll
      for (int j = 0; j < 3; ++j) { m0[j] = mu[j]; v0[j] = cv[j]; }
      contract_gaussian(mu, cv);
    }
    for (int f = q; f < ndeg; f += 8) {
      const float s = (float)(1u << (a.min_deg + f));  // (degrees <= 24)
      const float hs2 = -0.5f * s * s;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        float kappa;
        {
#pragma clang fp contract(off)
          const float y = mu[j] * s;
          const float ph = y + kHalfPi;
          const float bb = ph - y;
          const float err = (y - (ph - bb)) + (kHalfPi - bb);  // (y + kHalfPi) - ph, exactly
          kappa = 4.371139e-8f - err;                          // kHalfPi - pi / 2 = 4.371139e-8
        }
        const float fs = e[6 * f + j], fc = e[6 * f + 3 + j], gs = g[6 * f + j], gc = g[6 * f + 3 + j];
        dm[j] += s * (gs * (fc + kappa * fs) - gc * (fs + kappa * fc));
        dc[j] += hs2 * (gs * fs + gc * fc);
      }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        dm[j] += __shfl_xor(dm[j], o, 64);
        dc[j] += __shfl_xor(dc[j], o, 64);
      }
    }
    if (q == 0) {
      const int k = c0 + ls;
      if constexpr (CONTRACT) contract_adjoint(m0, v0, dm, dc);
      float tmean, tvar, rvar;
      frustum_moments(t0, t1, radius, a.cylinder != 0, &tmean, &tvar, &rvar);
      // d mean_j / d d_j = tmean;  d cov_j / d d_j = 2 d_j (tvar - rvar / D);  d cov_i / d d_j (through D) =
      // 2 d_j rvar d_i^2 / D^2
      const float through_d = (2.0f * rvar / (dms * dms)) * ((dd[0] * dc[0] + dd[1] * dc[1]) + dd[2] * dc[2]);
      const float own = 2.0f * (tvar - rvar / dms);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        sx[j * S + k] = dm[j];
        sx[(3 + j) * S + k] = (tmean * dm[j] + dv[j] * (own * dc[j])) + dv[j] * through_d;
      }
      const size_t m = (size_t)r * S + k;
      sx[6 * S + k] = a.dsigma[m] * a.sigma[m];
    }
    __syncthreads();
  }
  {
    const int grp = tid >> 5, l = tid & 31;  // (a 32-lane group is half a wave: the butterfly stays inside it)
    float v = 0.0f;
    if (grp < kRgTerms)
      for (int k = l; k < S; k += 32) v += sx[grp * S + k];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (l == 0) s_sum[grp] = v;
  }
  __syncthreads();
  if (tid < 3) {
    const int j = tid;
    // alpha = 1 - exp(-sigma delta |d|): dL/d|d| = sum_k dsigma_k sigma_k / |d|, d|d| / dd_j = d_j / |d|
    float gd = s_sum[3 + j] + (dv[j] / dms) * s_sum[6];
    if (a.ddir) {  // identity rows, then per degree (sin rows, cos rows): a (sin, cos) pair is its own derivative
      const float* pe = a.enc_dir + (size_t)r * a.Vd;
      const float* gp = a.ddir + (size_t)r * a.Vd;
      float v = gp[j];
      const int nv = (a.Vd - 3) / 6;
      for (int f = 0; f < nv; ++f) {
        const float s = (float)(1u << f);
        const int is = 3 + 6 * f + j, ic = is + 3;
        v += s * (gp[is] * pe[ic] - gp[ic] * pe[is]);
      }
      gd += v;
    }
    const float go = s_sum[j];
    const size_t i = (size_t)3 * r + j;
    a.o_grad[i] = a.accumulate ? a.o_grad[i] + go : go;
    a.d_grad[i] = a.accumulate ? a.d_grad[i] + gd : gd;
  }
}

hipError_t launch_ray_grad(const RayGradArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (a.S < kRgChunk || a.S % kRgChunk != 0 || a.S > 512 || a.P < 6 || a.P % 6 != 0 || a.min_deg < 0 ||
      a.min_deg + a.P / 6 > 24 || !a.t || !a.o || !a.d || !a.radius || !a.enc || !a.denc || !a.sigma || !a.dsigma ||
      !a.o_grad || !a.d_grad || ((uintptr_t)a.enc & 15) || ((uintptr_t)a.denc & 15))
    return hipErrorInvalidValue;
  if (a.ddir && (!a.enc_dir || a.Vd < 3 || (a.Vd - 3) % 6 != 0 || (a.Vd - 3) / 6 > 24)) return hipErrorInvalidValue;
  const size_t shm = sizeof(float) * (2 * (size_t)kRgChunk * a.P + (size_t)kRgTerms * a.S);
  if (shm > 64 * 1024) return hipErrorInvalidValue;
  if (a.contract)
    hipLaunchKernelGGL(k_ray_grad<true>, dim3(a.n), dim3(kRgThreads), shm, st, a);
  else
    hipLaunchKernelGGL(k_ray_grad<false>, dim3(a.n), dim3(kRgThreads), shm, st, a);
  return hipGetLastError();
}

}  // namespace nof
