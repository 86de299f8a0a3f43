// Any-shape MLP, fp16 products (NOF_PRECISION_F16_PRODUCTS): k_gemm's product (generic.hip; launch.h
// GemmArgs: two strided sources per operand along k, per-ray rows, bias / ReLU / G > 0 epilogues, split-K
// chunks, row sums) on v_mfma_f32_16x16x32_f16 instead of v_mfma_f32_16x16x4_f32:
//   C(i, j) = epilogue(inv_s * sum_k f16(s X(i, k)) f16(Y(j, k)))
// Both operands stay fp32 in HBM and are rounded to fp16 (RNE, v_cvt_pk_f16_f32) when they are staged in
// LDS; the products are exact in fp32 and summed in fp32 in a fixed k order.  s = delta_scale(scale_amax)
// (mlp_common.h: a power of two read on the device, 1 without scale_amax) multiplies the operand scale_src
// names (1: A, 2: B) before the rounding, and the sums are multiplied by its exact inverse before the
// epilogue: the backward's deltas (1e-9 and below at the heads) keep their significands in fp16 and nothing
// scaled is ever stored.  rowsum[z M + i] = inv_s * sum_k f16(s A(i, k)), from the staged tile in k order.
//
// LDS tile [row][32 halves]: 64-byte rows, no padding; the 16-byte chunk c (k = 8c .. 8c + 7) of row r
// is stored at chunk position c ^ ((r >> 1) & 3).  Bank argument (banks of 4 bytes):
//   * operand reads, one ds_read_b128 per 16 x 32 fragment (lane l: row l & 15, chunk l >> 4), 64 banks,
//     lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: a group reads rows 0-3 and
//     12-15 at one chunk c and rows 4-11 at c ^ 1 (or the reverse).  Rows with equal r & 3 share a 256-byte
//     phase (4 rows x 64 bytes); of such a quadruple t, 4 + t, 8 + t, 12 + t the group reads positions
//     c ^ x, c ^ 1 ^ 2 ^ x, c ^ 1 ^ x, c ^ 2 ^ x (x = t >> 1): all four chunks of the 64-byte segment, so the
//     16 lanes cover the 16 slots of the 256 bytes once.  Unswizzled, rows t and 12 + t collide (2-way);
//   * row-fast staging (a thread holds 8 consecutive k of a row: one ds_write_b128), 32 banks, groups of 8
//     consecutive lanes = 8 consecutive rows from a multiple of 8 at one chunk: rows of equal parity share a
//     128-byte phase and (r >> 1) & 3 takes its four values over them: 8 slots, each once;
//   * k-fast staging (a thread holds 2 consecutive k: one ds_write_b32), 32 banks, groups of 32 lanes = two
//     whole rows = 128 consecutive bytes, whatever the chunk order inside a row.
// Only the row sums (wave 0 of the first column tile, one row per lane) read with 2-way conflicts.
#include "common.h"
#include "gemm_tile.h"
#include "launch.h"
#include "mlp_common.h"

namespace nof {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kHK = 32;    // k-step: one 16x16x32 MFMA deep
constexpr int kHD = 2;     // k-steps of global loads in flight

__device__ __forceinline__ int h_chunk(int r, int c) { return c ^ ((r >> 1) & 3); }

// Per-thread load plan of one operand tile (T rows x 32 k per k-step, E = T / 8 elements per thread), as
// generic.hip's GPlan: threads run along the source's unit-stride index.  k-fast (sk == 1): a thread holds
// E / 2 pairs of consecutive k, pair p in row 16 p + tid / 16 at k = 2 (tid & 15) (16 lanes along a row's
// 32 k); row-fast: lanes along the rows, a thread holds the E consecutive k from (tid / T) E of row tid % T.
// A pair whose source is 8-byte aligned at every even k is one 8-byte load, else two dwords (measured, the
// 8 x 512 network's step: dword pairs 51.3 ms, 8-byte pairs 44.0 ms; quads of 4 k on 16-byte loads and
// ds_write_b64, 8 lanes along a row: 48.5 ms, not kept).
// Either way elements (e, e + 1), e even, are neighbours along k: one packed conversion.  One pointer per
// pair (k-fast) or per thread (row-fast) at k-step 0, with the per-ray row divisions, is computed once (a
// pointer per element, k_gemm's plan, costs 2 E registers per source: two waves per SIMD did not hold the
// 64 x 128 tile's).  A step inside one source and the chunk adds wave-uniform offsets to it; other steps
// (a source boundary or the chunk's tail inside the step) compute and mask each element.
template <int T>
struct HPlan {
  static constexpr int E = T * kHK / kTileThreads;
  static constexpr int P = E / 2;
  const float* b1[P];  // row-fast: [0] alone
  const float* b2[P];
  bool kfast;
  bool al1, al2;  // k-fast: the source's pairs are 8-byte aligned at every even k (one 8-byte load per pair)
};
__device__ __forceinline__ bool h_aligned2(const GemmSrc& s, int k_origin) {
  return s.sk == 1 && (s.si & 1) == 0 && (reinterpret_cast<uintptr_t>(s.p) & 7) == 0 && (k_origin & 1) == 0;
}
template <int T> __device__ __forceinline__ int h_row(bool kfast, int e, int tid) {
  return kfast ? 16 * (e >> 1) + (tid >> 4) : tid % T;
}
template <int T> __device__ __forceinline__ int h_kbase(bool kfast, int tid) {  // the pointer's k within a step
  return kfast ? 2 * (tid & 15) : (tid / T) * HPlan<T>::E;
}

template <bool TWO, int T>
__device__ __forceinline__ void h_plan(HPlan<T>& pl, const GemmSrc& s1, const GemmSrc& s2, int rows, int r0, int tid,
                                       int K1, int kb) {
  static_assert(HPlan<T>::E % 8 == 0, "row-fast plans store 8 k per ds_write_b128");
  const bool kfast = s1.sk == 1;
  pl.kfast = kfast;
  pl.al1 = h_aligned2(s1, kb);  // (a chunk's steps start at kb + a multiple of 32)
  pl.al2 = TWO && h_aligned2(s2, kb - K1);
  const int64_t kl = h_kbase<T>(kfast, tid);
#pragma unroll
  for (int p = 0; p < HPlan<T>::P; ++p) {
    const int i = r0 + h_row<T>(kfast, 2 * p, tid);
    const int ic = i < rows ? i : 0;  // a row outside the operand re-reads row 0 (never stored)
    const int i1 = s1.idiv == 1 ? ic : ic / s1.idiv;
    pl.b1[p] = s1.p + (int64_t)i1 * s1.si + kl * s1.sk;
    if (TWO) {
      const int i2 = s2.idiv == 1 ? ic : ic / s2.idiv;
      pl.b2[p] = s2.p + (int64_t)i2 * s2.si + kl * s2.sk;
    }
  }
}

// a step with a source boundary or the chunk's tail inside: every element's address and mask
template <bool TWO, int T, bool KF>
__device__ __forceinline__ uint32_t h_fetch_masked(float (&v)[HPlan<T>::E], const HPlan<T>& pl, const GemmSrc& s1,
                                                   const GemmSrc& s2, int K1, int ke, int k0, int rows, int r0, int tid) {
  constexpr int E = HPlan<T>::E;
  const float* ptr[E];
  const int kb = h_kbase<T>(KF, tid);
  uint32_t m = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int k = k0 + kb + (KF ? (e & 1) : e);
    const bool ok = r0 + h_row<T>(KF, e, tid) < rows && k < ke;
    const bool one = !TWO || k < K1;
    const int kk = (one ? k : k - K1) - kb;  // from the pointer's k
    const float* p1 = pl.b1[KF ? e >> 1 : 0] + (int64_t)kk * s1.sk;
    if (TWO) {
      const float* p2 = pl.b2[KF ? e >> 1 : 0] + (int64_t)kk * s2.sk;
      ptr[e] = ok ? (one ? p1 : p2) : s1.p;
    } else {
      ptr[e] = ok ? p1 : s1.p;
    }
    m |= ok ? 1u << e : 0u;
  }
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = *ptr[e];
  return m;
}

// the loads only (the masks are applied at the LDS store: a select here would wait for the loads).
// Returns whether the step took the uniform-offset path; else bit e of okm = element e is inside.
template <bool TWO, int T>
__device__ __forceinline__ bool h_fetch(float (&v)[HPlan<T>::E], uint32_t& okm, const HPlan<T>& pl, const GemmSrc& s1,
                                        const GemmSrc& s2, int K1, int ke, int k0, int rows, int r0, int tid) {
  constexpr int E = HPlan<T>::E;
  if (k0 + kHK <= ke && (k0 + kHK <= K1 || k0 >= K1)) {
    const bool one = !TWO || k0 < K1;
    if (pl.kfast) {
      if (one && pl.al1) {
#pragma unroll
        for (int e = 0; e < E; e += 2) {
          const f32x2 t = *reinterpret_cast<const f32x2*>(pl.b1[e >> 1] + k0);
          v[e] = t[0]; v[e + 1] = t[1];
        }
      } else if (one) {  // sk == 1: the pair's second element is an immediate offset
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = pl.b1[e >> 1][(int64_t)k0 + (e & 1)];
      } else if (pl.al2) {
#pragma unroll
        for (int e = 0; e < E; e += 2) {
          const f32x2 t = *reinterpret_cast<const f32x2*>(pl.b2[e >> 1] + (k0 - K1));
          v[e] = t[0]; v[e + 1] = t[1];
        }
      } else {
        const int64_t koff = (int64_t)(k0 - K1) * s2.sk;
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = pl.b2[e >> 1][koff + (e & 1) * s2.sk];
      }
    } else {
      if (one) {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = pl.b1[0][(int64_t)(k0 + e) * s1.sk];
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = pl.b2[0][(int64_t)(k0 - K1 + e) * s2.sk];
      }
    }
    return true;
  }
  // (static pointer indices under a wave-uniform branch: a runtime index would put the arrays in scratch)
  if (pl.kfast) okm = h_fetch_masked<TWO, T, true>(v, pl, s1, s2, K1, ke, k0, rows, r0, tid);
  else okm = h_fetch_masked<TWO, T, false>(v, pl, s1, s2, K1, ke, k0, rows, r0, tid);
  return false;
}

// RNE fp32 pair -> packed fp16 (v_cvt_pk_f16_f32)
__device__ __forceinline__ uint32_t h_pk(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2{a, b}), f16x2));
}

// scale, zero what the masks exclude (the k tail, rows outside the operand, the other source's k), round
// and store: dst = the tile as 16-byte chunks, 4 per row
template <int T>
__device__ __forceinline__ void h_store(uint32_t* dst, const HPlan<T>& pl, const float (&v)[HPlan<T>::E], uint32_t okm,
                                        bool nomask, float s, int tid) {
  constexpr int E = HPlan<T>::E;
  uint32_t w[E / 2];
#pragma unroll
  for (int e = 0; e < E; e += 2) {
    const float x = nomask || (okm >> e & 1u) ? v[e] * s : 0.0f;
    const float y = nomask || (okm >> (e + 1) & 1u) ? v[e + 1] * s : 0.0f;
    w[e / 2] = h_pk(x, y);
  }
  const int kb = h_kbase<T>(pl.kfast, tid);
  if (pl.kfast) {
#pragma unroll
    for (int e = 0; e < E; e += 2) {
      const int r = h_row<T>(true, e, tid);
      dst[r * 16 + 4 * h_chunk(r, kb >> 3) + ((kb & 7) >> 1)] = w[e / 2];
    }
  } else {
    const int r = h_row<T>(false, 0, tid);
#pragma unroll
    for (int e = 0; e < E; e += 8) {
      const u32x4 q = {w[e / 2], w[e / 2 + 1], w[e / 2 + 2], w[e / 2 + 3]};
      *reinterpret_cast<u32x4*>(dst + r * 16 + 4 * h_chunk(r, (kb + e) >> 3)) = q;
    }
  }
}

// gemm_tile.h's tile and epilogue (k_gemm's) around the fp16 load pipeline above
template <int TN, bool TWO, bool MASK>
__global__ __launch_bounds__(kTileThreads, 2) void k_gemm_h(GemmArgs a) {
  static_assert(!MASK || TN == 64, "the mask epilogue is the 64-column tiles'");
  constexpr int NQ = TN / 32;
  __shared__ __attribute__((aligned(16))) uint32_t As[kTileM * 16], Bs[TN * 16];
  const int tid = threadIdx.x, lane = tid & 63;
  const GemmTile t = gemm_tile<TN>(a);
  const int i0 = t.i0, j0 = t.j0, wi = t.wi, wj = t.wj, kb = t.kb, ke = t.ke;
  // the power-of-two scale of one operand and its exact inverse (wave-uniform: one scalar load)
  const float s = a.scale_src && a.scale_amax ? delta_scale(a.scale_amax, false) : 1.0f;
  const float inv_s = a.scale_src && a.scale_amax ? delta_scale(a.scale_amax, true) : 1.0f;
  const float sa = a.scale_src == 1 ? s : 1.0f, sb = a.scale_src == 2 ? s : 1.0f;
  HPlan<kTileM> pa;
  HPlan<TN> pb;
  h_plan<TWO>(pa, a.A1, a.A2, a.M, i0, tid, a.K1, kb);
  h_plan<TWO>(pb, a.B1, a.B2, a.N, j0, tid, a.K1, kb);
  f32x4 acc[2][NQ];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[p][q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float rs = 0.0f;
  float va[kHD][HPlan<kTileM>::E], vb[kHD][HPlan<TN>::E];
  uint32_t oa[kHD], ob[kHD];  // a masked step's element masks
  bool fa[kHD], fb[kHD];      // the set's step took the uniform-offset path (wave-uniform)
#pragma unroll
  for (int d = 0; d < kHD; ++d) oa[d] = ob[d] = 0u;
#pragma unroll
  for (int d = 0; d < kHD; ++d) {
    fa[d] = h_fetch<TWO>(va[d], oa[d], pa, a.A1, a.A2, a.K1, ke, kb + d * kHK, a.M, i0, tid);
    fb[d] = h_fetch<TWO>(vb[d], ob[d], pb, a.B1, a.B2, a.K1, ke, kb + d * kHK, a.N, j0, tid);
  }
  // the lane's fragment chunk: row (l & 15) of a 16-row block (a multiple of 16: the swizzle sees l alone)
  const int frag = (lane & 15) * 16 + 4 * h_chunk(lane & 15, lane >> 4);
  auto step = [&](int k0, int d) {
    h_store(As, pa, va[d], oa[d], fa[d], sa, tid);
    h_store(Bs, pb, vb[d], ob[d], fb[d], sb, tid);
    __syncthreads();
    if (k0 + kHD * kHK < ke) {
      fa[d] = h_fetch<TWO>(va[d], oa[d], pa, a.A1, a.A2, a.K1, ke, k0 + kHD * kHK, a.M, i0, tid);
      fb[d] = h_fetch<TWO>(vb[d], ob[d], pb, a.B1, a.B2, a.K1, ke, k0 + kHD * kHK, a.N, j0, tid);
    }
    if (t.rowsum)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f16x8 w = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(As + lane * 16 + 4 * h_chunk(lane, c)));
#pragma unroll
        for (int u = 0; u < 8; ++u) rs += (float)w[u];
      }
    f16x8 av[2], bv[NQ];
#pragma unroll
    for (int p = 0; p < 2; ++p)
      av[p] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(As + (wi + 16 * p) * 16 + frag));
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      bv[q] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(Bs + (wj + 16 * q) * 16 + frag));
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[p], bv[q], acc[p][q], 0, 0, 0);
    __syncthreads();
  };
  for (int k0 = kb; k0 < ke; k0 += kHD * kHK)
#pragma unroll
    for (int d = 0; d < kHD; ++d)
      if (k0 + d * kHK < ke) step(k0 + d * kHK, d);
  gemm_epilogue<NQ, MASK, true>(a, t, acc, rs, inv_s);
}

const char* gen_h_variant_name(int v) {
  static const char* const kNames[kGhCount] = {
      "k_gemm_h<64,false,false>.unsplit", "k_gemm_h<64,true,false>.unsplit", "k_gemm_h<64,false,true>.unsplit",
      "k_gemm_h<64,true,true>.unsplit", "k_gemm_h<64,false,false>.splitk", "k_gemm_h<128,false,false>.splitk"};
  return v >= 0 && v < kGhCount ? kNames[v] : nullptr;
}

hipError_t launch_gemm_h(const GemmArgs& a, int ksplit, hipStream_t st, int* variant) {
  if (variant) *variant = -1;
  if (a.M <= 0 || a.N <= 0) return hipSuccess;
  if (a.scale_src < 0 || a.scale_src > 2) return hipErrorInvalidValue;
  static constexpr void (*kKern[])(GemmArgs) = {k_gemm_h<64, false, false>, k_gemm_h<64, true, false>,
                                                k_gemm_h<64, false, true>,  k_gemm_h<64, true, true>,
                                                k_gemm_h<64, false, false>, k_gemm_h<128, false, false>};
  int pick;
  dim3 grid;
  const hipError_t e = gemm_tile_grid(a, ksplit, &pick, &grid);
  if (e != hipSuccess) return e;
  if (variant) *variant = kGhGemm64 + pick;
  hipLaunchKernelGGL(kKern[pick], grid, dim3(kTileThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace nof
