// Fused MLP backward (input-gradient chain), fp32 precision, on v_mfma_f32_16x16x4_f32 at two
// waves per SIMD (mlp16.h): heads -> layer 9 -> layers 7..1.
//
// Replaces the 11 backpropagate_neuron* launches of AcceleratedMLP::get_gradient
// (MLPcpp:256-321; AF:91-182), whose ~17 G global atomicAdds per 256x256 layer (AF:101-110)
// are the reference's dominant cost.  The chain dh_{l-1} = W_l^T delta_l runs with delta resident
// in registers (the forward's register-layout trick, on the transposed slices), ReLU masks come
// from the forward's packed bits, and every delta_l is written once in the block-swizzled [F][32]
// layout for the deterministic weight-gradient GEMMs (wgrad.hip).
// Gradient routing per D11: dh7 = W8^T dz_s + W9[:, :256]^T delta9 ; dh3 = W4[:, :256]^T delta4.
// Heads per MNcs:23-28,184-189 with the sigmoid' written as s(1-s) (overflow-safe, D28).
#include "common.h"
#include "launch.h"
#include "mlp16.h"

namespace nof {


// delta = mask ? acc (+ w8 * dz_s) : 0 -> B operand + delta block, one tile per call inside the
// next layer's MFMA stream; w8 values loaded one tile ahead.  kSplit (f16x2): the B operand is kept
// pre-split (put_tile, mlp16.h).
template <bool kDensity, class ST, bool kSplit = false>
struct BwdEpi16 {
  static constexpr int kVmPerPart = 4;
  const f32x4 (&acc)[16];
  float (&bin)[16][4];
  const ST& bst;
  const int g;
  const float* w8;  // LDS, + 4g
  float dzs;
  __amdgpu_buffer_rsrc_t dst_blk;
  uint2 mk;
  f32x4 wnext;

  __device__ __forceinline__ BwdEpi16(const f32x4 (&acc_)[16], float (&bin_)[16][4], const ST& bst_, int lane)
      : acc(acc_), bin(bin_), bst(bst_), g(lane >> 4) {}
  template <class E>
  __device__ __forceinline__ void begin(const uint2* mask, E* dst_blk_, const float* w8_ = nullptr, float dzs_ = 0.0f) {
    mk = *mask;
    dst_blk = blk_rsrc_t(dst_blk_);
    if constexpr (kDensity) {
      w8 = w8_ + 4 * g;
      dzs = dzs_;
      wnext = *reinterpret_cast<const f32x4*>(w8);
    }
  }
  __device__ __forceinline__ void operator()(int t) {
    f32x4 w4;
    if constexpr (kDensity) {
      w4 = wnext;
      if (t + 1 < 16) wnext = *reinterpret_cast<const f32x4*>(w8 + 16 * (t + 1));
    }
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = acc[t][r];
      if constexpr (kDensity) v[r] = __builtin_fmaf(w4[r], dzs, v[r]);  // explicit: every variant rounds alike
      v[r] = mask16_apply(mk, t, r, v[r]);
    }
    put_tile<kSplit, true>(bin, t, v, bst, dst_blk);
  }
  __device__ __forceinline__ void tile01() {
    (*this)(0);
    (*this)(1);
  }
};

// P: 0 = fp32, 2 = f16x2 (16x16x32 f16, power-of-2 scaled deltas stored as fp16 blocks),
// 3 = F32_F16SPLIT (16x16x32 f16, the scaled deltas stored as fp32 blocks)
//
// A launch may carry a second level (BwdArgs::M1 > 0): its workgroups follow the first level's on the
// grid.  A workgroup belongs to one level, picked from blockIdx.x before anything else: every wave of it runs the
// single-level code on that level's fields, with the tail-wave clamp and the delta scale of that level alone.
template <int P>
__global__ __launch_bounds__(kMlp16Threads, 1) void k_mlp_bwd16(BwdArgs a0) {
  typedef typename Store16<P, true>::T ST;
  typedef typename Store16<P, true>::E AE;
  __shared__ __attribute__((aligned(16))) float lds[ring16_floats<P>() + 256];
  float* w8_lds = lds + ring16_floats<P>();
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, j = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform: block pointers stay in SGPRs
  const int half = wave & 1;
  const ST bst(lane, half);
  const int wg0 = (a0.M / kBlk + 3) / 4;  // the first level's workgroups
  const bool second = a0.M1 > 0 && (int)blockIdx.x >= wg0;  // workgroup-uniform: scalar selects, no divergence
  struct {
    int M;
    const float *dsigma, *drgb, *zhead;
    const uint32_t *amax, *masks;
    const float* wimg_b;
    float dbias, rgb_scale;
    float *delta, *delta9x;
  } a;
  a.M = second ? a0.M1 : a0.M;
  a.dsigma = second ? a0.dsigma1 : a0.dsigma;
  a.drgb = second ? a0.drgb1 : a0.drgb;
  a.zhead = second ? a0.zhead1 : a0.zhead;
  a.amax = second ? a0.amax1 : a0.amax;
  a.masks = second ? a0.masks1 : a0.masks;
  a.delta = second ? a0.delta1 : a0.delta;
  a.delta9x = second ? a0.delta9x1 : a0.delta9x;
  a.wimg_b = a0.wimg_b; a.dbias = a0.dbias; a.rgb_scale = a0.rgb_scale;
  const int wg = second ? (int)blockIdx.x - wg0 : (int)blockIdx.x;
  const int nblk = a.M / kBlk;
  const int blk_raw = wg * 4 + (wave >> 1);
  const int blk = blk_raw < nblk ? blk_raw : nblk - 1;  // tail waves duplicate the last block of their level
  const int m = blk * kBlk + 16 * half + j;
  NOF_DCHECK(a.M % kBlk == 0 && blk >= 0 && blk < nblk, kChkMlpBlock);
  const float* tail = a.wimg_b + (size_t)kBwdSlices * kSliceFloats;
  const size_t layer_stride = (size_t)nblk * kWidth * kBlk;
  uint32_t* masks = const_cast<uint32_t*>(a.masks);

  // ---- prologue.  vmcnt retires in issue order: a wait for a value loaded after the ring DMA would wait for the
  // DMA's 64 KB, a wait for a W10 row loaded after a delta9x store for that store's HBM acknowledgement, and
  // __syncthreads() (vmcnt(0)) for all the stores, which nothing here reads.  So every load goes first, into
  // registers (the heads' inputs, the view layer's mask words, all of W10, w8), then the ring DMA of slices 0 and
  // 1, then the arithmetic with its delta9x stores, then a counted wait and the barrier.
  const f32x4 zh = reinterpret_cast<const f32x4*>(a.zhead)[m];
  const float dsig = a.dsigma[m];
  const float drgb3[3] = {a.drgb[(size_t)m * 3], a.drgb[(size_t)m * 3 + 1], a.drgb[(size_t)m * 3 + 2]};
  float sc = 1.0f;
  if constexpr (P >= 2) sc = delta_scale(a.amax, false);  // f16 pieces: deltas enter them scaled by a power of two
  const uint2 mk9 = *mask16_ptr(masks, blk, 8, half, lane);
  f32x4 w10r[8][3];  // W10[c][16t + 4g .. + 3]
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      w10r[t][c] = *reinterpret_cast<const f32x4*>(tail + kBwdTailW10 + 128 * c + 16 * t + 4 * g);
  // (every wave loads the 1-KB w8 row, wave 0 writes it: a load inside a branch would be waited for at its end)
  const f32x4 w8r = reinterpret_cast<const f32x4*>(tail + kBwdTailW8)[lane];
  __builtin_amdgcn_sched_barrier(0);
  ring16_prologue(a.wimg_b, lds, tid);
  __builtin_amdgcn_sched_barrier(0);

  // ---- heads (MNcs:23-28,184-189) ------------------------------------------------------------
  float dzs = dsig * sigmoid_f(zh[0] + a.dbias);
  float dzc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s = sigmoid_f(zh[1 + c]);
    dzc[c] = drgb3[c] * (s * (1.0f - s)) * a.rgb_scale;
  }
  if constexpr (P >= 2) {
    dzs *= sc;
#pragma unroll
    for (int c = 0; c < 3; ++c) dzc[c] *= sc;
  }
  if (wave == 0) reinterpret_cast<f32x4*>(w8_lds)[lane] = w8r;
  const __amdgpu_buffer_rsrc_t d9 = blk_rsrc_t(reinterpret_cast<AE*>(a.delta9x) + (size_t)blk * kD9F * kBlk);
  // rows 128..143 = tile 8: dz_sigma, dz_rgb in lane group 0, zeros above
#pragma unroll
  for (int r = 0; r < 4; ++r) bst.store(d9, 8, r, g == 0 ? (r == 0 ? dzs : dzc[r - 1]) : 0.0f);
  // ---- delta9 = (W10^T dz_rgb) * relu'(layer 9) ------------------------------------------
  float bin[16][4];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)  // explicit FMAs: every precision variant rounds alike
      v[r] = mask16_apply(mk9, t, r, __builtin_fmaf(w10r[t][2][r], dzc[2],
                                                   __builtin_fmaf(w10r[t][1][r], dzc[1], w10r[t][0][r] * dzc[0])));
    put_tile<P >= 2, true>(bin, t, v, bst, d9);
  }
  // The barrier that publishes the ring's slots 0 and 1 and w8.  Issue order of this wave's vector-memory
  // operations: the loads above, the 8 ring DMA steps, then the kD9Stores delta9x stores (tile 8's 4, then per tile
  // of delta9 4 dword stores, or 2 packed fp16 stores in f16x2 mode) and nothing else.  vmcnt retires in issue
  // order, so vmcnt(kD9Stores) leaves at most those stores in flight and has retired every load and DMA step;
  // lgkmcnt(0) retires wave 0's w8 write.  No ring slot and no w8 word is read before this barrier: the first such
  // reads are layer 9's, below.  36 and 20 fit the 6-bit vmcnt field (max 63).
  constexpr int kD9Stores = 4 + 8 * (P == 2 ? 2 : 4);
  static_assert(kD9Stores == (P == 2 ? 20 : 36), "the literals in the waits below");
  if constexpr (P == 2) asm volatile("s_waitcnt vmcnt(20)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(36)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  int cur = 0;
  const float* wsrc = a.wimg_b;
  f32x4 accA[16], accB[16];  // ping-pong, as in the forward
  AE* delta_blk = reinterpret_cast<AE*>(a.delta) + (size_t)blk * kWidth * kBlk;
  // ---- dh7 = W9[:, :256]^T delta9 + w8 dz_s ; delta7 ---------------------------------------
  BwdEpi16<true, ST, P >= 2> e7(accA, bin, bst, lane);
  e7.begin(mask16_ptr(masks, blk, 7, half, lane), delta_blk + 7 * layer_stride, w8_lds, dzs);
  layer16<P, 4, 0, 16>(bin, nullptr, accA, lds, cur, wsrc, false, tid, lane);
  e7.tile01();
  // ---- dh_{l-1} = W_l[:, :256]^T delta_l ; delta_{l-1}, l = 7..1 (l odd: A -> B) ------------
  BwdEpi16<false, ST, P >= 2> ea(accA, bin, bst, lane), eb(accB, bin, bst, lane);
  eb.begin(mask16_ptr(masks, blk, 6, half, lane), delta_blk + 6 * layer_stride);
  layer16<P, 8, 0, 16>(bin, nullptr, accB, lds, cur, wsrc, false, tid, lane, e7);
  eb.tile01();
  static_assert(kDepth == 8, "bwd pairing assumes 8 trunk layers");
  for (int l = kDepth - 2; l >= 2; l -= 2) {
    ea.begin(mask16_ptr(masks, blk, l - 1, half, lane), delta_blk + (l - 1) * layer_stride);
    layer16<P, 8, 0, 16>(bin, nullptr, accA, lds, cur, wsrc, false, tid, lane, eb);
    ea.tile01();
    eb.begin(mask16_ptr(masks, blk, l - 2, half, lane), delta_blk + (l - 2) * layer_stride);
    layer16<P, 8, 0, 16>(bin, nullptr, accB, lds, cur, wsrc, l == 2, tid, lane, ea);
    eb.tile01();
  }
  // delta0: nothing left to hide it under
#pragma unroll
  for (int t = 2; t < 16; ++t) eb(t);
}

hipError_t launch_mlp_bwd16(const BwdArgs& a, hipStream_t st) {
  // one workgroup per 4 blocks of a level; the second level's (M1 > 0) after the first's
  const dim3 grid((a.M / kBlk + 3) / 4 + (a.M1 > 0 ? (a.M1 / kBlk + 3) / 4 : 0));
  if (a.split == 2) hipLaunchKernelGGL(k_mlp_bwd16<2>, grid, dim3(kMlp16Threads), 0, st, a);
  else if (a.split == 3) hipLaunchKernelGGL(k_mlp_bwd16<3>, grid, dim3(kMlp16Threads), 0, st, a);
  else hipLaunchKernelGGL(k_mlp_bwd16<0>, grid, dim3(kMlp16Threads), 0, st, a);
  return hipGetLastError();
}

NOF_CHECK_UNIT(check_unit_mlp_bwd16)

}  // namespace nof
