// Host-side launchers of the gfx950 kernels (one definition per .hip file).
// All launches are asynchronous on the given stream; none allocates or synchronises,
// so a caller may capture any sequence of them into a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nof {

// ---- device checks (common.h NOF_DCHECK; compiled in only with -DNOF_DEVICE_CHECKS) -------------
// per translation unit: its failed-check bits, optionally cleared; ~0u if the copy failed
uint32_t check_unit_sampling(bool clear);
uint32_t check_unit_mlp_fwd16(bool clear);
uint32_t check_unit_mlp_bwd16(bool clear);
uint32_t check_unit_wgrad(bool clear);
uint32_t check_unit_dataset(bool clear);
uint32_t check_unit_view(bool clear);
uint32_t check_unit_appearance(bool clear);
hipError_t launch_check_selftest(hipStream_t st);  // fails kChkSelfTest on purpose

// ---- sampling.hip (get_sample_t_vals AF:222-242, get_resampled_t_vals AF:246-291) ----------
// lindisp: t linear in disparity (SampleAlongRay MH:618-620) instead of depth
hipError_t launch_sample_stratified(int n, int S, const float* nears, const float* fars, int randomized,
                                    uint64_t seed, uint32_t step, uint32_t level, uint32_t ray_base, float* t,
                                    hipStream_t st, int lindisp = 0);
hipError_t launch_sample_pdf(int n, int S_in, const float* t_in, const float* w, int S_out, float padding,
                             int randomized, uint64_t seed, uint32_t step, uint32_t level, uint32_t ray_base,
                             float* t_out, int32_t* idx_out, hipStream_t st);
// ray_shape 1: cylinders (CylinderToGaussian MH:403-409) instead of conical frustums; contraction != 0: the scene
// contraction (contract.h) applied to every Gaussian before it is stored (k_cast_contract; 0: k_cast, as it was)
hipError_t launch_cast(int n, int S, const float* t, const float* o, const float* d, const float* radius,
                       float* mean, float* cov, hipStream_t st, int ray_shape = 0, int contraction = 0);
hipError_t launch_encode(int n, int S, const float* mean, const float* cov, const float* d, float* enc_pos,
                         float* enc_dir, hipStream_t st);

// ---- render.hip (volumetric_rendering AF:318-344, get_output_gradient AF:347-361,
//      volumetric_rendering_gradient AF:362-402) -------------------------------------------------
// acc / dist (optional): accumulated opacity and the clamped weighted-midpoint distance (MH:472-492);
// nonfinite (optional): word 0 set to 1 when a ray's composite colour is not finite
hipError_t launch_render_fwd(int n, int S, const float* sigma, const float* rgb, const float* t, const float* d,
                             int white, float* C, float* w, hipStream_t st, float* acc = nullptr,
                             float* dist = nullptr, uint32_t* nonfinite = nullptr);
// the training forward's integrator of a level (as launch_render_fwd, no acc / dist) and the resampler of
// the next level (as launch_sample_pdf, no idx) in one launch, one ray per workgroup
struct RenderPdfArgs {
  int n, S;  // rays, samples of this level (the resampler's input bins)
  const float *sigma, *rgb, *t, *d;
  int white;
  float *C, *w;
  uint32_t* nonfinite;
  int S_out;  // the next level's samples
  float padding;
  int randomized;
  uint64_t seed;
  uint32_t step, level, ray_base;  // level: the next level's index (its Philox stream)
  float* t_out;
};
hipError_t launch_render_fwd_pdf(const RenderPdfArgs& a, hipStream_t st);
// g_ext != null: dL/dC supplied by the caller (callback path); else fused loss gradient from pix.
hipError_t launch_render_bwd(int n, int S, const float* sigma, const float* rgb, const float* t, const float* d,
                             int white, const float* C, const float* g_ext, const float* pix,
                             const float* lossmult, float loss_mult_sum, float lam, float* dsigma, float* drgb,
                             float* loss_rays, hipStream_t st);
// Several levels of S samples per ray in one launch (the fused step's loss gradient + adjoint of every
// level): lv[l] the level's inputs / outputs; lv[l].amax (optional, zero on entry) receives the bits of
// max(|dsigma|, |drgb|) over the level (launch_delta_amax's value), a.nonfinite word 1 its non-finite flag.
constexpr int kRenderMaxLevels = 4;
struct RenderBwdLevel {
  const float *sigma, *rgb, *t, *C, *g_ext;
  float lam;
  float *dsigma, *drgb, *loss_rays;
  uint32_t* amax;
  // the distortion loss (the last level only: 0 for every other one, a block-uniform skip):
  // dL/dw_k of dist_mult lossmult[r] / msum L_r joins e_k; dist_rays ([n], optional) receives that per-ray term
  float dist_mult = 0.0f;
  float* dist_rays = nullptr;
};
struct RenderBwdArgs {
  int n, S, white;
  const float *d, *pix, *lossmult;
  float msum;
  uint32_t* nonfinite;
  RenderBwdLevel lv[kRenderMaxLevels];
  // 1: the last entry's level has not been composited yet: its blocks run the integrator forward first
  // (as launch_render_fwd with C = fwd_C, w = fwd_w; no acc / dist), g_ext must be null
  int fwd_last = 0;
  float *fwd_C = nullptr, *fwd_w = nullptr;
  // the rays' near / far ([n]) and the sampling's lindisp, the normalised distance of the distortion loss (needed
  // where a dist_mult != 0).  The trailing levels with dist_mult != 0 run k_render_bwd<PER, true>, the others the
  // instantiation without the term in a launch of their own: with every dist_mult 0, exactly the launch it was
  const float *nears = nullptr, *fars = nullptr;
  int lindisp = 0;
};
hipError_t launch_render_bwd(const RenderBwdArgs& a, int nlev, hipStream_t st);
hipError_t launch_output_gradient(int n, const float* C, const float* pix, const float* lossmult,
                                  float loss_mult_sum, float lam, float* g, hipStream_t st);

// One level's loss gradient + adjoint with the cross-level terms (nof_config.stop_level_grad = 0): q (optional,
// [n][S]) = dL/dw_k from the next level's resampler, folded into e_k = g.c_k - G + q_k; t_grad (optional,
// [n][S + 1], overwritten) = dL/dt through delta_k = t_{k+1} - t_k: dt_k = ddelta_{k-1} - ddelta_k with
// ddelta_k = X_k sigma_k |d|.  Otherwise launch_render_bwd's single-level form (its own kernel: the
// instantiations above are untouched); fwd: the level's integrator forward first, as RenderBwdArgs::fwd_last.
struct RenderBwdXArgs {
  int n, S, white;
  const float *d, *pix, *lossmult;
  float msum;
  uint32_t* nonfinite;
  const float *sigma, *rgb, *t, *C, *g_ext;
  float lam;
  float *dsigma, *drgb, *loss_rays;
  const float* q;
  float* t_grad;
  int fwd;
  float *fwd_C, *fwd_w;
  // the distortion loss, as RenderBwdLevel / RenderBwdArgs (dist_mult != 0: k_render_bwd_x<PER, true>); with
  // t_grad, its dL/dt_k = dL/ds_k s'(t_k) is added to the row before it is stored
  float dist_mult;
  float* dist_rays;
  const float *nears, *fars;
  int lindisp;
};
hipError_t launch_render_bwd_x(const RenderBwdXArgs& a, hipStream_t st);

// ---- crosslevel.hip: the adjoints of cast + IPE and of the resampler (stop_level_grad = 0) ------------
// t_grad [n][S + 1] (overwritten) = (add0 +) d/dt of sum_{m, F} denc[m][F] enc[m][F](t) (+ add1): enc / denc
// [n S][P], P = 6 degrees from min_deg in the any-shape encoder's feature order, enc the stored forward
// encoding; add0 / add1 (optional, [n][S + 1]) are added before / after in that order.  S a multiple of 64.
// contract != 0: enc is the encoding of the contracted Gaussians (contract.h; k_encode_grad<true>).
struct EncodeGradArgs {
  int n, S, P, min_deg, cylinder;
  const float *t, *o, *d, *radius, *enc, *denc;
  const float *add0, *add1;
  float* t_grad;
  int contract;
};
hipError_t launch_encode_grad(const EncodeGradArgs& a, hipStream_t st);
// The adjoint of launch_sample_pdf (same sampling arguments): t_out_grad [n][S_out + 1] -> w_grad [n][S_in]
// and, optional, t_in_grad [n][S_in + 1] (the input t row as the bin edges)
struct SamplePdfGradArgs {
  int n, S_in, S_out;
  const float *t_in, *w;
  float padding;
  int randomized;
  uint64_t seed;
  uint32_t step, level, ray_base;
  const float* t_out_grad;
  float *w_grad, *t_in_grad;
};
hipError_t launch_sample_pdf_grad(const SamplePdfGradArgs& a, hipStream_t st);

// ---- interlevel.hip: the interlevel (proposal) loss of one coarser level (nof_mipnerf_set_interlevel_loss) ----
// w_grad [n][S_prop] (accumulate: added to, else overwritten) = dL/dw^ of mult lossmult[r] / msum L_r, L_r the
// envelope loss of the proposal (t_prop [n][S_prop + 1], w_prop [n][S_prop]) against the target (t_tgt
// [n][S_tgt + 1], w_tgt [n][S_tgt], a constant); rays ([n], optional) receives the per-ray term.  S_prop, S_tgt in
// {64, 128, 256, 512} independently.
struct InterlevelArgs {
  int n, S_prop, S_tgt, accumulate;
  const float *t_prop, *w_prop, *t_tgt, *w_tgt, *lossmult;
  float msum, mult;
  float *w_grad, *rays;
};
hipError_t launch_interlevel(const InterlevelArgs& a, hipStream_t st);

// ---- raygrad.hip: one level's share of dL/d(origin), dL/d(direction) per ray (nof_mipnerf_set_ray_grad) ------
// o_grad / d_grad [n][3] (accumulate: added to, else overwritten) from enc / denc [n S][P] (as EncodeGradArgs), the
// level's sigma / dsigma [n S] (the integrator's |d|) and, ddir != null, the view encoding enc_dir / ddir [n][Vd]
// (Vd = 3 + 6 deg_view, dir_feature's order).  S a multiple of 32, at most 512.  contract != 0: as EncodeGradArgs
// (k_ray_grad<true>).
struct RayGradArgs {
  int n, S, P, min_deg, cylinder, Vd, accumulate;
  const float *t, *o, *d, *radius, *enc, *denc, *sigma, *dsigma;
  const float *enc_dir, *ddir;
  float *o_grad, *d_grad;
  int contract;
};
hipError_t launch_ray_grad(const RayGradArgs& a, hipStream_t st);

// ---- mlp_fwd.hip / mlp_bwd.hip -----------------------------------------------------------------
struct FwdArgs {
  int M, S, encoded;
  int no_store;                            // 1: inference only, skip the backward's side outputs
  int split;                               // MLP precision: 0 fp32, 1 bf16x3 split, 2 f16x2 (mlp_common.h)
  int cylinder;                            // fused encoding: cylinders (MH:403-409) instead of conical frustums
  // heads (MNcs:19-22,151-152): sigma = softplus(z_s + dbias), rgb = sigmoid(z_c) rgb_scale - rgb_pad with
  // rgb_scale = fp32(1 + 2 rgb_pad); MipNerfModel.DensityBias / RgbPadding, the reference values by default
  float dbias = -1.0f, rgb_scale = 1.002f, rgb_pad = 0.001f;
  const float *t, *origins, *dirs, *radii;  // fused-encoding inputs
  const float *enc_pos, *enc_dir;          // encoded inputs (API path): [M][96], [n][27]
  // k_mlp_fwd16, fused encoding only (optional, both or neither): the step's per-ray view tables (ViewTabArgs,
  // written by the pack launch) — the view-PE rows [n][32] and the view layer's per-ray bias [n][128]; null: every
  // wave computes its ray's from dirs and the image's tail (the same bits)
  const float *view_pe, *view_bias;
  const float* wimg;                       // packed forward image (slices + tail)
  float* act_in;   // [M/32][128][32]
  float* act_h;    // [8][M/32][256][32]
  float* act_h9;   // [M/32][128][32]
  uint32_t* masks; // [M/32][9][64][4]
  float* zhead;    // [M][4]
  float* sigma;    // [M]
  float* rgb;      // [M][3]
};
hipError_t launch_mlp_fwd(const FwdArgs& a, hipStream_t st);

struct BwdArgs {
  int M;
  int split;                               // as FwdArgs::split
  const float *dsigma, *drgb, *zhead;
  const uint32_t* amax;                    // split == 2: max |dsigma|, |drgb| bits (launch_delta_amax)
  float dbias = -1.0f, rgb_scale = 1.002f; // the heads' derivatives (MNcs:23-28,184-189), as FwdArgs
  const uint32_t* masks;
  const float* wimg_b;                     // packed backward image (slices + tail)
  float* delta;    // [8][M/32][256][32]
  float* delta9x;  // [M/32][160][32]
  // F16 (k_mlp_bwd_h32) only: a second level's dX chain in the same launch (M1 > 0), its 256-sample groups
  // after the first level's — one persistent launch per step instead of one per level
  int M1;
  const float *dsigma1, *drgb1, *zhead1;
  const uint32_t *amax1, *masks1;
  float *delta1, *delta9x1;
};
hipError_t launch_mlp_bwd(const BwdArgs& a, hipStream_t st);
// f16x2 mode: *amax = bits of max(|dsigma|, |drgb|) over M samples (clears *amax first); nonfinite
// (optional): word 1 set to 1 when an input is not finite
hipError_t launch_delta_amax(const float* dsigma, const float* drgb, int M, uint32_t* amax, hipStream_t st,
                             uint32_t* nonfinite = nullptr, bool cleared = false);  // cleared: *amax is 0 already
// fp32-precision kernels (v_mfma_f32_16x16x4_f32, two waves per SIMD): mlp_fwd16.hip / mlp_bwd16.hip
hipError_t launch_mlp_fwd16(const FwdArgs& a, hipStream_t st);
hipError_t launch_mlp_bwd16(const BwdArgs& a, hipStream_t st);
// F16 mode (mlp_h32.h, mlp_f16.hip): 32 samples per wave on 32x32x16 f16, row-chunk-outer layers;
// activations / deltas as row-major [M][F] fp16, wimg / wimg_b the h32 images
hipError_t launch_mlp_fwd_h32(const FwdArgs& a, hipStream_t st);
int device_cus();  // compute units of the current device (persistent grids)
hipError_t launch_mlp_bwd_h32(const BwdArgs& a, hipStream_t st);

// ---- wgrad.hip: weight/bias gradients as one scheduled split-K launch + ordered reduce ------
struct WgProblem {
  const float* A; const float* B;
  int FA, a_row0, ntr;   // A rows [a_row0, a_row0 + 32*ntr) of an [FA][32]-block buffer
  int FB, b_col0, ntc;   // B rows (= output columns) [b_col0, b_col0 + 32*ntc)
  int shape;             // fp32 k_wgrad wave-grid shape (wgrad_shape); unused by k_wgrad_x3
  // F16 (k_wgrad_s) only: output columns past the first ntc1 tiles come from up to two more operands
  // (B2 rows [b2_col0, +32 ntc2), then B3), so the problems that share an A operand read it once
  int ntc1;              // tiles of B (ntc = ntc1 + ntc2 + ntc3)
  const float* B2; int FB2, b2_col0, ntc2;
  const float* B3; int FB3, b3_col0, ntc3;
  int level;             // the MLP level whose operands these are (the reduce's per-level delta scale)
};
struct WgItem { int prob, kb0, kb1; int slab; };  // slab = index into slab_off[]
// k_wgrad_reduce threads an output needs (max_elems of launch_wgrad_reduce = the max over outputs)
int wgrad_reduce_threads(int nrows, int ncols, int col_off);
constexpr int kWgMaxLevels = 4;
struct WgOut {
  int item0, nitems;        // contiguous items of the problem (item i writes slab i)
  int lev_items[kWgMaxLevels];  // of which level 0's come first, then level 1's, ... (the reduce's grouping)
  int nlev;
  int row_off, nrows, col_off, ncols;
  float* dst; int ld, dst_col;
  float* bias_dst;          // null: no bias
  int prob;
};
hipError_t launch_wgrad(const WgProblem* probs, const WgItem* items, const int* item_ptr, int num_wg,
                        const int64_t* slab_off, float* slabs, float* bias_slabs, hipStream_t st);
// fp32 k_wgrad: the cheapest wave-grid shape for an ntr x ntc tile problem; *cost2 = MFMA tiles of
// its busiest SIMD per 16 k-steps (2 per 32x32 tile-k-block at two waves per SIMD)
int wgrad_shape(int ntr, int ntc, int* cost2);
// fp32 k_wgrad: calibrated time of one k-block of an ntr x ntc tile problem (1600 = an (8,8) block);
// *shape = the wave-grid shape it runs with
int wgrad_block_cost(int ntr, int ntc, int* shape);
int wgrad_x3_grid_cols();  // columns of k_wgrad_x3's 2 x C wave grid (schedule cost model)
// split-precision weight gradients: precision 1 (bf16x3) or 2 (f16x2)
hipError_t launch_wgrad_x3(const WgProblem* probs, const WgItem* items, const int* item_ptr, int num_wg,
                           const int64_t* slab_off, float* slabs, float* bias_slabs, int precision, hipStream_t st);
hipError_t launch_wgrad_reduce(const WgOut* outs, int nouts, int max_elems, const WgItem* items,
                               const WgProblem* probs, const int64_t* slab_off, const float* slabs,
                               const float* bias_slabs, int accumulate, const uint32_t* amax, hipStream_t st);
// (amax != null: sums are multiplied by the inverse f16x2 delta scale, mlp_common.h)

// ---- generic.hip: the any-shape fp32 MLP, one MFMA GEMM launch per layer ----------------------
// element (i, k) of a source = p[(i / idiv) si + k sk] (idiv: 1 or a per-ray divisor, the view encodings
// read per sample without a per-sample copy)
struct GemmSrc {
  const float* p = nullptr;
  int64_t si = 0, sk = 0;
  int idiv = 1;
};
// C(i, j) = epilogue(sum_{k < K1 + K2} A(i, k) B(j, k)), i < M, j < N; A(i, k) = A1(i, k) for k < K1, else
// A2(i, k - K1) (B alike).  Epilogue: + bias[j], ReLU, then 0 where !(G(i, j) > 0) — each optional.
// Split-K (one k source, no G): blockIdx.z = chunk of kchunk (a multiple of 16) k values, its raw sums at C + z
// slab_stride.
struct GemmArgs {
  int M = 0, N = 0, K1 = 0, K2 = 0;
  GemmSrc A1, A2, B1, B2;
  const float* bias = nullptr;
  int relu = 0;
  const float* G = nullptr; int64_t gi = 0, gj = 0;
  float* C = nullptr; int64_t ci = 0, cj = 0;
  int kchunk = 0; int64_t slab_stride = 0;
  float* rowsum = nullptr;  // optional: rowsum[z M + i] = sum_{k in chunk z} A(i, k) (bias gradients)
  // gemm_ws.hip only: the ReLU mask as bits, 4 words per row (word (i, g) bit 4t + r = column 16t + 4g + r):
  // written by a ReLU product (mask_out), applied by a dX product (mask_in) in place of G
  const uint32_t* mask_in = nullptr;
  uint32_t* mask_out = nullptr;
  // gemm_h.hip only: the power-of-two scale s = delta_scale(scale_amax) (mlp_common.h; read on the device) of
  // one operand inside each fp16 product, its inverse applied to the sums: 0 none, 1 the A operand, 2 B
  const uint32_t* scale_amax = nullptr;
  int scale_src = 0;
};
// Every kernel variant the any-shape launchers can select (AcceleratedMLP's dispatch tally: tests and
// tooling see which instantiation a product ran on).  A launcher reports its pick through its optional
// `variant` out-parameter, set where the template is chosen (-1: nothing launched).
enum GenVariant : int {
  kGvGemm64 = 0,       // k_gemm<64, TWO, MASK>, one k chunk: + TWO + 2 MASK
  kGvGemm64Split = 4,  // k_gemm<64, false, false>, split-K (ksplit > 1)
  kGvGemm128Split,     // k_gemm<128, false, false>, split-K, N > 64
  kGvWs_8_6_0,         // k_gemm_ws's static chunk shapes <NT, SC1, SC2, SV2[, T1]>
  kGvWs_8_8_0,
  kGvWs_1_8_0,
  kGvWs_8_8_2,
  kGvWs_8_8_1,
  kGvWs_8_1_0_T1,
  kGvWsRuntime,                  // k_gemm_ws<NT>, runtime chunk shape: + NT - 1 (NT = 1 .. 8)
  kGvEncode = kGvWsRuntime + 8,  // k_encode_g
  kGvEncode4,                    // k_encode_g4
  kGvSlabSums,                   // k_slab_sums (one count per batch launched)
  kGvRaySum,                     // k_ray_sum
  kGvCount
};
const char* gen_variant_name(int v);  // null outside [0, kGvCount)
hipError_t launch_gemm(const GemmArgs& a, int ksplit, hipStream_t st, int* variant = nullptr);
// gemm_h.hip (NOF_PRECISION_F16_PRODUCTS): launch_gemm's product with one fp16 product per term on
// v_mfma_f32_16x16x32_f16: C(i, j) = epilogue(inv_s sum_k f16(s X(i, k)) f16(Y(j, k))), X the operand
// a.scale_src names, fp32 sums in a fixed k order; rowsum[z M + i] = inv_s sum_k f16(s A(i, k)).  kchunk: any
// positive count; split-K (ksplit > 1) takes one k source and no mask.  Its own variant list (a tally of its
// own: AcceleratedMLP::gen_dispatch_h):
enum GenHVariant : int {
  kGhGemm64 = 0,       // k_gemm_h<64, TWO, MASK>, one k chunk: + TWO + 2 MASK
  kGhGemm64Split = 4,  // k_gemm_h<64, false, false>, split-K
  kGhGemm128Split,     // k_gemm_h<128, false, false>, split-K, N > 64
  kGhCount
};
const char* gen_h_variant_name(int v);  // null outside [0, kGhCount)
hipError_t launch_gemm_h(const GemmArgs& a, int ksplit, hipStream_t st, int* variant = nullptr);
// gemm_ws.hip: the weight-stationary form for N <= 128, 16-padded K1 + K2 <= 160, no split, no G / rowsum
constexpr int kWsMaxN = 128, kWsMaxK = 160;
bool gemm_ws_fits(const GemmArgs& a);
hipError_t launch_gemm_ws(const GemmArgs& a, hipStream_t st, int* variant = nullptr);
// dst[r ld + c] (+)= sum_{z < nz} slabs[z stride + r pitch + c] (a fixed order), r < rows, c < cols
hipError_t launch_slab_sum(int rows, int cols, int pitch, int nz, const float* slabs, int64_t stride, float* dst,
                           int64_t ld, int accumulate, hipStream_t st);
// many slab sums (disjoint destinations) in ceil(n / kSlabJobsMax) launches: the table travels in the
// kernel arguments
struct SlabJob {
  const float* slabs;
  float* dst;
  int64_t stride, ld;
  int rows, cols, pitch, nz, accumulate;
};
constexpr int kSlabJobsMax = 24;
struct SlabBatch {
  SlabJob job[kSlabJobsMax];
  int first[kSlabJobsMax + 1];
  int n;
};
hipError_t launch_slab_sums(const SlabJob* jobs, int n, hipStream_t st, int* launches = nullptr);  // (batches launched)
// IPE at degrees [min_deg, min_deg + P / 6) per sample, view PE (Vd = 3 + 6 deg_view features) per ray
// out[r][c] = sum over a ray's S sample rows of in (the per-ray operand's weight gradient over rays)
hipError_t launch_ray_sum(int R, int S, int cols, const float* in, int64_t ld, float* out, hipStream_t st);
hipError_t launch_encode_g(int n, int S, const float* mean, const float* cov, const float* d, int min_deg, int P,
                           int Vd, float* enc_pos, float* enc_dir, hipStream_t st, int* variant = nullptr);
// z [M][4] (density, rgb pre-activations) -> sigma [M], rgb [M][3]; backward: dz [M][4]
hipError_t launch_heads_fwd(int M, const float* z, float* sigma, float* rgb, float dbias, float rgb_scale,
                            float rgb_pad, hipStream_t st);
hipError_t launch_heads_bwd(int M, const float* dsigma, const float* drgb, const float* z, float* dz, float dbias,
                            float rgb_scale, hipStream_t st);

// ---- adam.hip ----------------------------------------------------------------------------------
// ---- dataset.hip: device-resident record set -> SoA batch gather (+ optional loss-mult sum) ----
hipError_t launch_gather_batch(const float* records, int64_t count, int n, uint64_t seed, uint32_t step,
                               uint32_t ray_base, float* o, float* d, float* vd, float* radius, float* near,
                               float* far, float* lm, float* pix, int* idx_out, float* lm_sum, hipStream_t st,
                               int staged = 0);
// the record index the gather draws for global ray `gray` (host copy of dataset.hip batch_record)
uint32_t batch_record_host(uint64_t seed, uint32_t step, uint32_t gray, int64_t count);

// ---- raygen.hip: poses (V x [R row-major | t]) (+ images [V][H][W][3]) -> 64-byte records ----
hipError_t launch_generate_rays(const float* poses, int V, int w, int h, float focal, float near, float far, int ndc,
                                const float* images, float* records, hipStream_t st);

// ---- multiscale scenes (include/nof.h nof_multiscale_layout): images at num_scales resolutions ----
// Scale s halves width, height and focal length s times and weighs its rays by lossmult[s].  The
// virtual records are scale-major, then view-major, then row-major pixels: first[s] is scale s's first
// record, and, the image pyramid being stored in the same order, also its first pixel.  Passed to the
// kernels by value.
constexpr int kMaxScales = 4;
struct MultiscaleLayout {
  int num_scales, num_views;
  int w[kMaxScales], h[kMaxScales];
  float focal[kMaxScales], lossmult[kMaxScales];
  int64_t first[kMaxScales];
  int64_t count;
};
// raygen.hip: pyramid level s from level s - 1 of the same allocation (pyr: count x 3 floats, level 0
// filled by the caller): p = ((a + b) + (c + d)) * 0.25f over each 2 x 2 block, per channel
hipError_t launch_pyramid_level(float* pyr, const MultiscaleLayout& L, int s, hipStream_t st);
// raygen.hip: every virtual record in order (count x 16 floats); pyr == nullptr: rgb = 0
hipError_t launch_materialize(const float* poses, const float* pyr, const MultiscaleLayout& L, float near, float far,
                              int ndc, float* records, hipStream_t st);
// dataset.hip: launch_gather_batch for an image-backed scene: each drawn record is generated in the
// gather from its pose and pyramid pixel instead of being read
hipError_t launch_gather_rays(const float* poses, const float* pyr, const MultiscaleLayout& L, float near, float far,
                              int ndc, int n, uint64_t seed, uint32_t step, uint32_t ray_base, float* o, float* d,
                              float* vd, float* radius, float* nears, float* fars, float* lm, float* pix, int* idx_out,
                              float* lm_sum, hipStream_t st);
// dataset.hip: the rays' gradients o_grad / d_grad [n][3] of a batch of an image-backed scene (ndc = 0) summed per
// view into pose_grad [V][12] (rotation row-major, then translation: d = R cam(x, y, scale), o = t); idx: the
// batch's record indices.  A view without a ray: 0, or unchanged when accumulating.
hipError_t launch_pose_grad(const MultiscaleLayout& L, int n, const int* idx, const float* o_grad, const float* d_grad,
                            float* pose_grad, int accumulate, hipStream_t st);
// dataset.hip: the view of every record index of a batch of an image-backed scene (record_pos), views [n]
hipError_t launch_batch_views(const MultiscaleLayout& L, int n, const int* idx, int* views, hipStream_t st);

// ---- appearance.hip: per-view appearance embeddings (include/nof.h nof_mipnerf_create_ex) ----
// out [n][vd + dim] = [enc_dir row | table[id] row]; id = ids[r], or const_view for every ray when ids == null; an
// id outside [0, views) reads zeros (with per-ray ids a checked build also sets NOF_CHECK_GATHER)
hipError_t launch_appearance_gather(int n, int vd, int dim, int views, const float* enc_dir, const float* table,
                                    const int* ids, int const_view, float* out, hipStream_t st);
// d_table [views][dim] (+)= the rows of d_app [n][dim] summed per view id in a fixed order (an id outside
// [0, views) joins no row), plus partial [views][dim] when given (distinct from d_table).  A view without a ray:
// 0 (+ partial), or unchanged when accumulating.
hipError_t launch_appearance_grad(int n, int dim, int views, const int* ids, const float* d_app, const float* partial,
                                  float* d_table, int accumulate, hipStream_t st);

// ---- view.hip: a whole view of an image-backed scene, chunk by chunk (include/nof.h nof_dataset_render_view) ----
// The rays of pixels [p0, p0 + n) of a w x h view (one scale's row of the MultiscaleLayout), row-major, into a
// device SoA; the pose is row `view` of the device table `poses`, or `pose` when use_pose.  Bit-identical to
// launch_materialize's records of that view and scale.
struct ViewRayArgs {
  const float* poses;
  float pose[12];
  int use_pose, view, num_views;
  int w, h;
  float focal, near, far;
  int ndc, p0, n;
  float *o, *d, *radius, *nears, *fars;
};
hipError_t launch_view_rays(const ViewRayArgs& a, hipStream_t st);
// A rendered chunk (comp_rgb per level, the last level's distance and acc: n rays) into image buffers at pixel
// p0 (null ones skipped) and, gt != nullptr, each level's squared error against gt (the view's [npix][3]
// pixels): block b of this launch writes partials[l * blocks + block0 + b], a view's launches covering
// [0, blocks) between them.  launch_view_final then adds each level's partials in a fixed order.
constexpr int kViewMaxLevels = 4;  // NOF_MAX_LEVELS
constexpr int kViewStoreBlock = 256;
inline int view_store_blocks(int n) { return (n + kViewStoreBlock - 1) / kViewStoreBlock; }
struct ViewStoreArgs {
  int num_levels;
  const float* comp_rgb[kViewMaxLevels];
  const float *dist_in, *acc_in;
  float* rgb[kViewMaxLevels];
  float *distance, *acc;
  const float* gt;
  double* partials;
  int block0, blocks;
  int p0, n, npix;
  int view, num_views;
};
hipError_t launch_view_store(const ViewStoreArgs& a, hipStream_t st);
hipError_t launch_view_final(const double* partials, int blocks, int num_levels, double* sums, hipStream_t st);

// ---- metrics.hip: PSNR / SSIM of device images [H][W][3] (synchronises st) ----
hipError_t image_metrics(const float* a, const float* b, int W, int H, float max_val, float* psnr, float* ssim,
                         hipStream_t st);

// loopback all-reduce: bufs[0..k) (k <= kLoopMax, one device) <- their element-wise sum in member order
constexpr int kLoopMax = 8;
hipError_t launch_loopback_sum(int k, float* const* bufs, int64_t n, hipStream_t st);
hipError_t launch_adam(int64_t n, float* p, const float* g, float* m, float* v, float lr, float inv1, float inv2,
                       hipStream_t st);
// Adam's options (Config.GradMaxNorm / GradMaxVal / WeightDecayMult, TrainState.cs:58-59,70) and the step
// statistics (StatsUtil.cs:13,16-18).  The parameter / gradient tensors as segments of one virtual arena:
// tensor s holds elements [off[s], off[s + 1]); n = 1 for the flat arenas.  The moments are always flat.
constexpr int kAdamStatBlocks = 256;  // most blocks of the statistics pass = most partials per sum
constexpr int kAdamMaxSegs = 64;
struct AdamSegs {
  int n = 0;
  int64_t off[kAdamMaxSegs + 1] = {};
  float* p[kAdamMaxSegs] = {};
  const float* g[kAdamMaxSegs] = {};
};
struct AdamOpts {
  float grad_max_norm = 0.0f, grad_max_val = 0.0f;
  float wdc = 0.0f;  // (2 weight_decay_mult) / P, 0 = no decay
};
struct AdamStepStats {  // = nof_step_stats (include/nof.h)
  float weight_l2, grad_norm, grad_abs_max, grad_norm_clipped, clip_scale;
  int32_t iteration;
};
// partials [4][kAdamStatBlocks] doubles: per-block sums of g1^2, g2^2, p^2 and the per-block max |g1|
hipError_t launch_adam_stats(int64_t total, const AdamSegs& s, const AdamOpts& o, double* partials, hipStream_t st);
// the update after launch_adam_stats(total, ...) on the same stream: one block writes *record; modify = apply
// the decay and the clips (else k_adam's update on the gradient as it is)
hipError_t launch_adam_opt(int64_t total, const AdamSegs& s, float* m, float* v, float lr, float inv1, float inv2,
                           const AdamOpts& o, bool modify, const double* partials, AdamStepStats* record,
                           int32_t iteration, hipStream_t st);
// level 0's stratified t-values (k_sample_stratified's arguments), computable by the pack launch's extra blocks
struct StratArgs {
  int n = 0, S = 0;  // rays, samples (n = 0: none)
  const float* nears = nullptr;
  const float* fars = nullptr;
  int randomized = 0, lindisp = 0;
  uint64_t seed = 0;
  uint32_t step = 0, ray_base = 0;
  float* t = nullptr;
};
// the step's per-ray view tables (k_mlp_fwd16's FwdArgs::view_pe / view_bias), computable by the pack launch's
// extra blocks from the canonical parameter arena (not from the image the same launch is writing):
//   pe[r][k]   = dir_feature(k, dirs[r]) for k < 27, 0 for k = 27..31  (act_in rows 96..127 of the ray's samples)
//   bias[r][o] = fma chain s = b9[o]; s = fmaf(W9[o][256 + k], pe[r][k], s), k = 0..26 ascending
// — the values and the rounding order of k_mlp_fwd16's own prologue, which every wave of every level repeats
struct ViewTabArgs {
  int n = 0;  // rays (0: none)
  const float* dirs = nullptr;
  float *pe = nullptr, *bias = nullptr;
};
struct PackArgs {
  int woff[11]; int boff[11];
  uint32_t* zero = nullptr; int nzero = 0;  // words the pack launch also clears (the f16 modes' delta-scale maxima)
  // the training step's level-0 sampling rides the pack launch (blocks past the pack's own: one launch fewer
  // per step; the launch wrappers set pack_blocks), and so do the view tables (launch_pack_weights and
  // launch_pack_weights_x3 only: blocks past the sampling's, the wrappers set strat_blocks)
  StratArgs strat;
  ViewTabArgs view;
  int pack_blocks = 0, strat_blocks = 0;
};
hipError_t launch_pack_weights(const float* params, const PackArgs& pa, float* wimg_f, float* wimg_b, hipStream_t st);
// split images: precision 1 (bf16 hi/mid/lo) or 2 (f16 hi/lo)
hipError_t launch_pack_weights_h32(const float* params, const PackArgs& pa, float* wimg_f, float* wimg_b,
                                   hipStream_t st);
hipError_t launch_pack_weights_x3(const float* params, const PackArgs& pa, float* wimg_f, float* wimg_b,
                                  int precision, hipStream_t st);

}  // namespace nof
