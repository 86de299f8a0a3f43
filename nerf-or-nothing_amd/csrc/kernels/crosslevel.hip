// Cross-level gradients (nof_config.stop_level_grad = 0): with t^l = resample(t^{l-1}, w^{l-1}; u)
// differentiable, level l's loss reaches level l - 1's weights.  Three adjoint kernels for gfx950:
//   * k_encode_grad: cast + IPE with respect to t.  A (sin, cos) feature pair is its own derivative, so the
//     kernel streams the stored encoding and dL/dEnc and evaluates no transcendental (the rounding of the stored
//     cos phase is corrected to first order from the sample's mean);
//   * k_sample_pdf_grad: the resampler, with respect to the input weights and the input t row (the bin edges).
//     The forward's discrete decisions are recomputed by the forward's own code (resample.h);
//   * (the integrator's dL/dt lives with the integrator: render.hip k_render_bwd_x).
// No float atomics: every sum runs in a fixed order, the results are bit-identical run to run.
#include "common.h"
#include "contract.h"
#include "geometry.h"
#include "launch.h"
#include "resample.h"

namespace nof {

// ---- cast + IPE adjoint ---------------------------------------------------------------------------------
// d(tmean, tvar, rvar) -> d(t0, t1) of one sample (ConicalFrustumToGaussian MH:391-402 / CylinderToGaussian
// MH:403-409 differentiated; geometry.h frustum_gaussian is the forward)
__device__ __forceinline__ void cast_adjoint(float t0, float t1, float radius, bool cylinder, float dtmean, float dtvar,
                                             float drvar, float* dt0, float* dt1) {
  if (cylinder) {  // tmean = (t0 + t1) / 2, tvar = (t1 - t0)^2 / 12, rvar constant
    const float x = dtvar * (t1 - t0) * (1.0f / 6.0f);
    *dt0 = 0.5f * dtmean - x;
    *dt1 = 0.5f * dtmean + x;
    return;
  }
  const float mu = (t0 + t1) * 0.5f, hw = (t1 - t0) * 0.5f;
  const float mu2 = mu * mu, h = hw * hw;
  const float den = 3.0f * mu2 + h;
  const float iden = 1.0f / den, iden2 = iden * iden;
  // tmean = mu + 2 mu h / den
  const float tm_mu = 1.0f + 2.0f * h * iden - 12.0f * mu2 * h * iden2;
  const float tm_h = 2.0f * mu * iden - 2.0f * mu * h * iden2;
  // tvar = h / 3 - (4/15) N / den^2, N = h^2 (12 mu^2 - h)
  const float N = h * h * (12.0f * mu2 - h);
  const float N_mu = 24.0f * mu * h * h, N_h = 24.0f * mu2 * h - 3.0f * h * h;
  const float c415 = 4.0f / 15.0f;
  const float tv_mu = -c415 * (N_mu * iden2 - 12.0f * mu * N * iden2 * iden);
  const float tv_h = 1.0f / 3.0f - c415 * (N_h * iden2 - 2.0f * N * iden2 * iden);
  // rvar = r^2 (mu^2 / 4 + (5/12) h - (4/15) h^2 / den)
  const float r2 = radius * radius;
  const float rv_mu = r2 * (0.5f * mu + c415 * 6.0f * mu * h * h * iden2);
  const float rv_h = r2 * (5.0f / 12.0f - c415 * (2.0f * h * iden - h * h * iden2));
  const float dmu = (dtmean * tm_mu + dtvar * tv_mu) + drvar * rv_mu;
  const float dh = (dtmean * tm_h + dtvar * tv_h) + drvar * rv_h;
  const float dhw = dh * 2.0f * hw;
  *dt0 = 0.5f * (dmu - dhw);
  *dt1 = 0.5f * (dmu + dhw);
}

constexpr int kEgChunk = 32;    // samples staged per pass
constexpr int kEgThreads = 256; // 8 threads per staged sample

// One workgroup per ray.  Per pass, 32 samples' rows of enc and dEnc (32 P contiguous floats each: the ray's
// S P floats start 16-byte aligned, S being a multiple of 64) go to LDS by 16-byte coalesced loads; 8 threads
// per sample then take the degrees q, q + 8, ... and a fixed butterfly adds their partial sums.  Feature order:
// the any-shape encoder's (generic.hip k_encode_g): 6 f + j = sin, 6 f + 3 + j = "cos" at degree min_deg + f.
template <bool CONTRACT>
__global__ __launch_bounds__(kEgThreads) void k_encode_grad(EncodeGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = a.S, P = a.P, ndeg = P / 6;
  float* se = smem;                       // [32][P]
  float* sg = smem + kEgChunk * P;        // [32][P]
  float* sd0 = smem + 2 * kEgChunk * P;   // [S] dL/dt0 of each sample
  float* sd1 = sd0 + S;                   // [S] dL/dt1
  const int r = blockIdx.x, tid = threadIdx.x;
  const float d0 = a.d[3 * r], d1 = a.d[3 * r + 1], d2 = a.d[3 * r + 2];
  const float dms = fmaxf(1e-10f, (d0 * d0 + d1 * d1) + d2 * d2);
  const float dd[3] = {d0 * d0, d1 * d1, d2 * d2};
  const float dv[3] = {d0, d1, d2};
  const float oo[3] = {a.o[3 * r], a.o[3 * r + 1], a.o[3 * r + 2]};
  const float radius = a.radius[r];
  const float* tr = a.t + (size_t)r * (S + 1);
  const int n4 = kEgChunk * P / 4;  // (32 P is a multiple of 4)
  for (int c0 = 0; c0 < S; c0 += kEgChunk) {
    const size_t base = ((size_t)r * S + c0) * P;
    const f32x4* ge = reinterpret_cast<const f32x4*>(a.enc + base);
    const f32x4* gg = reinterpret_cast<const f32x4*>(a.denc + base);
    for (int i = tid; i < n4; i += kEgThreads) {
      reinterpret_cast<f32x4*>(se)[i] = ge[i];
      reinterpret_cast<f32x4*>(sg)[i] = gg[i];
    }
    __syncthreads();
    const int ls = tid >> 3, q = tid & 7;
    const float* e = se + ls * P;
    const float* g = sg + ls * P;
    float dm[3] = {0.0f, 0.0f, 0.0f}, dc[3] = {0.0f, 0.0f, 0.0f};
    // the sample's mean, bit for bit the forward's (geometry.h): the phase of a stored "cos" feature is
    // fl32(y + fl32(pi / 2)) = y + pi / 2 + kappa, and kappa (up to half an ulp of y: 5e-4 at y = 1e4) is exact in
    // fp32 (the addition's rounding error by TwoSum, plus fl32(pi / 2) - pi / 2).  To first order in kappa
    //   d(damp sin y) / dy = f_c + kappa f_s,   d(damp sin(y + pi / 2 + kappa)) / dy = -f_s - kappa f_c
    float mu[3], cv[3];
    frustum_gaussian(tr[c0 + ls], tr[c0 + ls + 1], oo, dv, radius, mu, cv, a.cylinder != 0);
    // CONTRACT: the stored features were evaluated at the contracted mean (kappa's y); the map's adjoint below is
    // taken at the uncontracted Gaussian
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
      // mean_j = d_j tmean + o_j ; cov_j = tvar d_j^2 + rvar (1 - d_j^2 / |d|^2)
      const float dtmean = (dv[0] * dm[0] + dv[1] * dm[1]) + dv[2] * dm[2];
      const float dtvar = (dd[0] * dc[0] + dd[1] * dc[1]) + dd[2] * dc[2];
      const float drvar = ((1.0f - dd[0] / dms) * dc[0] + (1.0f - dd[1] / dms) * dc[1]) + (1.0f - dd[2] / dms) * dc[2];
      float x0, x1;
      cast_adjoint(tr[k], tr[k + 1], radius, a.cylinder != 0, dtmean, dtvar, drvar, &x0, &x1);
      sd0[k] = x0;
      sd1[k] = x1;
    }
    __syncthreads();
  }
  // t_k bounds sample k - 1 above and sample k below; then the other two terms of dL/dt^l in a fixed order
  for (int k = tid; k <= S; k += kEgThreads) {
    float v = (k > 0 ? sd1[k - 1] : 0.0f) + (k < S ? sd0[k] : 0.0f);
    const size_t i = (size_t)r * (S + 1) + k;
    if (a.add0) v = a.add0[i] + v;
    if (a.add1) v = v + a.add1[i];
    a.t_grad[i] = v;
  }
}

hipError_t launch_encode_grad(const EncodeGradArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (a.S < 64 || a.S % 64 != 0 || a.P < 6 || a.P % 6 != 0 || a.min_deg < 0 || a.min_deg + a.P / 6 > 24 || !a.t || !a.o || !a.d ||
      !a.radius || !a.enc || !a.denc || !a.t_grad || ((uintptr_t)a.enc & 15) || ((uintptr_t)a.denc & 15))
    return hipErrorInvalidValue;
  const size_t shm = sizeof(float) * (2 * (size_t)kEgChunk * a.P + 2 * (size_t)a.S);
  if (shm > 64 * 1024) return hipErrorInvalidValue;
  if (a.contract)
    hipLaunchKernelGGL(k_encode_grad<true>, dim3(a.n), dim3(kEgThreads), shm, st, a);
  else
    hipLaunchKernelGGL(k_encode_grad<false>, dim3(a.n), dim3(kEgThreads), shm, st, a);
  return hipGetLastError();
}

// ---- resampler adjoint ----------------------------------------------------------------------------------
// One 64-lane workgroup per ray, as the forward.  LDS: the forward's 3 B + 2 floats (resample.h), then
//   sw[B] the input weights, sidx[ns], sa[4][ns] each output sample's terms, sb[4][B] their per-bin sums,
//   sDc[B + 1] dL/dcdf, sdp[B] dL/dpdf then dL/dwb
// Held at their forward values (the forward's code recomputes them): the bin index, tt clamped, den > 0,
// min(1, run) saturated, the pad branch, the blur-pool's max picks (a tie splits the gradient equally).
__global__ __launch_bounds__(64) void k_sample_pdf_grad(SamplePdfGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float s_wsum, s_pad, s_dot, s_sum;
  const int B = a.S_in, ns = a.S_out + 1;
  float* wb = smem;               // pdf after resample_cdf
  float* cdf = smem + B;
  float* trs = smem + 2 * B + 1;
  float* sw = smem + 3 * B + 2;
  int* sidx = reinterpret_cast<int*>(sw + B);
  float* sa = reinterpret_cast<float*>(sidx + ns);  // [4][ns]: db0, db1, dc0, dc1
  float* sb = sa + 4 * ns;                            // [4][B]
  float* sDc = sb + 4 * B;                            // [B + 1]
  float* sdp = sDc + B + 1;                           // [B]
  const int r = blockIdx.x, lane = threadIdx.x;
  const float* wr = a.w + (size_t)r * B;
  const float* tr = a.t_in + (size_t)r * (B + 1);
  for (int i = lane; i <= B; i += 64) {
    if (i < B) {
      const float v = wr[i];
      cdf[i] = v;
      sw[i] = v;
    }
    trs[i] = tr[i];
  }
  __syncthreads();
  resample_cdf(lane, B, smem, &s_wsum, a.padding, &s_pad);
  const float s1 = 1.0f / (float)ns;
  const float* g0 = a.t_out_grad + (size_t)r * ns;
  for (int s = lane; s < ns; s += 64) {
    const float u = resample_u(r, s, ns, s1, a.randomized, a.seed, a.step, a.level, a.ray_base);
    const int lo = resample_bin(cdf, B, u);
    const float b0 = trs[lo], b1 = trs[lo + 1], c0 = cdf[lo], c1 = cdf[lo + 1];
    float tt, raw;
    {
#pragma clang fp contract(off)
      const float denom = c1 - c0;
      raw = denom > 0.0f ? (u - c0) / denom : 0.0f;
      tt = fminf(fmaxf(raw, 0.0f), 1.0f);
    }
    const float denom = c1 - c0;
    const float g = g0[s];
    sidx[s] = lo;
    sa[s] = g * (1.0f - tt);
    sa[ns + s] = g * tt;
    float e0 = 0.0f, e1 = 0.0f;
    if (denom > 0.0f && raw >= 0.0f && raw <= 1.0f) {  // tt = (u - c0) / (c1 - c0), not clamped
      const float dtt = g * (b1 - b0) / denom;
      e0 = dtt * (tt - 1.0f);
      e1 = -dtt * tt;
    }
    sa[2 * ns + s] = e0;
    sa[3 * ns + s] = e1;
  }
  __syncthreads();
  // u is monotone in s, so a bin's samples are a contiguous range: gathered in s order, no scatter
  for (int i = lane; i < B; i += 64) {
    int lo = 0, hi = ns;  // first s with sidx[s] >= i
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sidx[mid] < i) lo = mid + 1; else hi = mid;
    }
    float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, x3 = 0.0f;
    for (int s = lo; s < ns && sidx[s] == i; ++s) {
      x0 += sa[s]; x1 += sa[ns + s]; x2 += sa[2 * ns + s]; x3 += sa[3 * ns + s];
    }
    sb[i] = x0; sb[B + i] = x1; sb[2 * B + i] = x2; sb[3 * B + i] = x3;
  }
  __syncthreads();
  for (int i = lane; i <= B; i += 64) {  // edge i = lower edge of bin i, upper edge of bin i - 1
    const float db = (i < B ? sb[i] : 0.0f) + (i > 0 ? sb[B + i - 1] : 0.0f);
    if (a.t_in_grad) a.t_in_grad[(size_t)r * (B + 1) + i] = db;
    sDc[i] = (i < B ? sb[2 * B + i] : 0.0f) + (i > 0 ? sb[3 * B + i - 1] : 0.0f);
  }
  __syncthreads();
  if (lane == 0) {  // cdf[k + 1] = min(1, run_k), run_k = run_{k-1} + pdf_k (k < B - 1); cdf[0], cdf[B] constants
    float acc = 0.0f, dot = 0.0f, sum = 0.0f;
    sdp[B - 1] = 0.0f;
    for (int k = B - 2; k >= 0; --k) {
      if (cdf[k + 1] < 1.0f) acc += sDc[k + 1];
      sdp[k] = acc;
      dot += acc * wb[k];
      sum += acc;
    }
    s_dot = dot;
    s_sum = sum;
  }
  __syncthreads();
  {
    const float wsum = s_wsum;
    // pdf = wb' / wsum.  No pad: wsum = sum wb.  Pad branch: wb' = wb + (1e-5 - sum wb) / B, wsum = 1e-5
    const bool padded = s_pad > 0.0f;
    const float sub = padded ? (s_sum / wsum) / (float)B : s_dot / wsum;
    for (int i = lane; i < B; i += 64) sdp[i] = sdp[i] / wsum - sub;
  }
  __syncthreads();
  float* wg = a.w_grad + (size_t)r * B;
  for (int j = lane; j < B; j += 64) {  // wb_i = .5 (max(w_{i-1}, w_i) + max(w_i, w_{i+1})) + padding, edges repeated
    const float wj = sw[j];
    float v = 0.0f;
    if (j == 0) v += 0.5f * sdp[0];
    if (j == B - 1) v += 0.5f * sdp[B - 1];
    if (j > 0) {
      const float o = sw[j - 1];
      const float share = wj > o ? 1.0f : (wj == o ? 0.5f : 0.0f);
      v += share * (0.5f * (sdp[j - 1] + sdp[j]));
    }
    if (j < B - 1) {
      const float o = sw[j + 1];
      const float share = wj > o ? 1.0f : (wj == o ? 0.5f : 0.0f);
      v += share * (0.5f * (sdp[j] + sdp[j + 1]));
    }
    wg[j] = v;
  }
}

hipError_t launch_sample_pdf_grad(const SamplePdfGradArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (a.S_in < 2 || a.S_out < 1 || !a.t_in || !a.w || !a.t_out_grad || !a.w_grad) return hipErrorInvalidValue;
  const size_t B = a.S_in, ns = (size_t)a.S_out + 1;
  const size_t shm = sizeof(float) * ((3 * B + 2) + B + ns + 4 * ns + 4 * B + (B + 1) + B);
  if (shm > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sample_pdf_grad, dim3(a.n), dim3(64), shm, st, a);
  return hipGetLastError();
}

}  // namespace nof
