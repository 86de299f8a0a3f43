// What the two tiled any-shape GEMMs, k_gemm (generic.hip, fp32 products) and k_gemm_h (gemm_h.hip, fp16
// products), share: the tile 64 (i) x TN (j), TN = 64 or 128, of 4 waves in a 2 x 2 grid of 32 x TN / 2 wave
// tiles, a split-K chunk's k bounds, the epilogue and the launchers' checks.  The load pipelines are their own.
#pragma once
#include "common.h"
#include "launch.h"

namespace nof {

constexpr int kTileM = 64;  // tile rows (i)
constexpr int kTileThreads = 256;

struct GemmTile {
  int tcol, i0, j0;  // column tile, the tile's first row and column
  int wi, wj;        // the wave's tile inside it
  int ib, jb;        // lane rows i = ib + 16 p + r, columns j = jb + 16 q (the epilogue's)
  int kb, ke;        // the chunk's k range: the chunk end bounds k as well (a split-K chunk reads only its own k)
  // row sums of A over this chunk's k (the bias gradient beside a weight gradient): the first column tile's
  // wave 0, one row per lane, from the LDS tile, in k order
  bool rowsum;
};

template <int TN>
__device__ __forceinline__ GemmTile gemm_tile(const GemmArgs& a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  GemmTile t;
  // output tiles linear in blockIdx.x, columns fastest (a grid's y is capped at 65535 row tiles)
  const int ntc = (a.N + TN - 1) / TN;
  t.tcol = blockIdx.x % ntc;
  t.i0 = (blockIdx.x / ntc) * kTileM;
  t.j0 = t.tcol * TN;
  t.wi = (wave >> 1) * 32;
  t.wj = (wave & 1) * (TN / 2);
  t.ib = t.i0 + t.wi + 4 * (lane >> 4);
  t.jb = t.j0 + t.wj + (lane & 15);
  t.kb = blockIdx.z * a.kchunk;
  t.ke = min(a.K1 + a.K2, t.kb + a.kchunk);
  t.rowsum = a.rowsum && t.tcol == 0 && wave == 0;
  return t;
}

// the dX GEMMs' ReLU mask (G > 0: the forward activation): all 8 NQ loads issued together before the
// epilogue uses any (per element, beside its use, they were dependent loads one after another: the dX
// GEMMs 200 us against 136 us for forward GEMMs of the same shape; configs[0] step 5.16 -> 4.72 ms).
// Issued before the k loop instead they held 16 more registers through it: a wave per SIMD less, 10 % slower
template <int NQ>
__device__ __forceinline__ void gemm_mask_fetch(float (&gv)[NQ][2][4], const GemmArgs& a, const GemmTile& t) {
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = min(t.ib + 16 * p + r, a.M - 1), j = min(t.jb + 16 * q, a.N - 1);
        gv[q][p][r] = a.G[i * a.gi + j * a.gj];
      }
}

// after the k loop: the row sum rs and the lane's sums acc, each times inv_s if SCALED (k_gemm_h's operand
// scale), to rowsum and to the chunk's slab of C: + bias, ReLU, the mask (MASK: a.G), inside M x N only
template <int NQ, bool MASK, bool SCALED>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& a, const GemmTile& t, const f32x4 (&acc)[2][NQ], float rs,
                                              float inv_s = 1.0f) {
  const int lane = threadIdx.x & 63;
  float gv[MASK ? NQ : 1][2][4];
  if constexpr (MASK) gemm_mask_fetch(gv, a, t);
  if constexpr (SCALED) rs *= inv_s;
  if (t.rowsum && t.i0 + lane < a.M) a.rowsum[(int64_t)blockIdx.z * a.M + t.i0 + lane] = rs;
  float* C = a.C + (int64_t)blockIdx.z * a.slab_stride;
  // one 64-bit row offset per lane, wave-uniform steps
  const int64_t crow = (int64_t)t.ib * a.ci;
  float bj[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) bj[q] = a.bias && t.jb + 16 * q < a.N ? a.bias[t.jb + 16 * q] : 0.0f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int j = t.jb + 16 * q;
    if (j >= a.N) continue;
    const int64_t cj = (int64_t)j * a.cj;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (t.ib + 16 * p + r >= a.M) continue;
        float v = acc[p][q][r];
        if constexpr (SCALED) v *= inv_s;
        if (a.bias) v += bj[q];
        if (a.relu) v = fmaxf(v, 0.0f);
        if constexpr (MASK)
          if (!(gv[q][p][r] > 0.0f)) v = 0.0f;
        C[crow + (int64_t)(16 * p + r) * a.ci + cj] = v;
      }
  }
}

// Host side: what launch_gemm and launch_gemm_h check alike, their grid and their pick of an instantiation, in
// the order of both variant lists (launch.h): <64, TWO, MASK> with one k chunk at TWO + 2 MASK, then split-K
// (ksplit > 1) <64> and <128>.  Split-K is the weight gradients': one k source, no mask; it takes 64 x 128
// tiles for products wider than 64 columns (A read once for up to 128 columns).
inline hipError_t gemm_tile_grid(const GemmArgs& a, int ksplit, int* pick, dim3* grid) {
  const bool two = a.K2 > 0, mask = a.G != nullptr;
  if (ksplit < 1 || a.kchunk <= 0 || !a.A1.p || !a.B1.p || (two && (!a.A2.p || !a.B2.p)) || a.A1.idiv < 1 ||
      a.A2.idiv < 1 || a.B1.idiv < 1 || a.B2.idiv < 1 || !a.C || (ksplit > 1 && (two || mask)))
    return hipErrorInvalidValue;
  *pick = ksplit > 1 ? (a.N > 64 ? 5 : 4) : two + 2 * mask;
  const int TN = *pick == 5 ? 128 : 64;
  const int64_t tiles = (int64_t)((a.N + TN - 1) / TN) * ((a.M + kTileM - 1) / kTileM);
  if (tiles > 0x7fffffff || ksplit > 65535) return hipErrorInvalidValue;
  *grid = dim3((unsigned)tiles, 1, ksplit);
  return hipSuccess;
}

}  // namespace nof
