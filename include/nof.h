/*
 * nof.h — C ABI of the MI355X-native ScratchNerf hot path ("nerf-or-nothing_amd").
 *
 * This is the drop-in boundary for the reference's C++/CLI host API
 * (namespace AcceleratedNeRFUtils, the headers in /root/reference/ScratchNerf/AcceleratedNeRFUtils/),
 * consumed by ScratchNerf/Program.cs:24-26,42,51-60.  Each entry point below names the
 * reference member it replaces.  Conventions:
 *   - every call returns nof_status; nof_last_error() gives a thread-local message;
 *     nothing aborts the process;
 *   - device pointers returned by the library are BORROWED: valid until the next call
 *     on the same object or its destruction (MLPcpp:254,315-320);
 *   - host inputs are only read during the call; host outputs are caller-provided;
 *   - all device work is enqueued on cfg->stream (NULL = default stream), asynchronously,
 *     except where a host result is returned (layer sizes, retrieve_output, loss);
 *   - float3 / System.Numerics.Vector3 arrays are packed float[n][3] (12 B per element).
 * No torch / HIP types appear in these signatures.
 */
#ifndef NOF_H
#define NOF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum nof_status {
  NOF_OK = 0,
  NOF_ERR_INVALID_ARG = 1,
  NOF_ERR_HIP = 2,
  NOF_ERR_RCCL = 3,
  NOF_ERR_OOM = 4,
  NOF_ERR_UNSUPPORTED = 5
} nof_status;

#define NOF_MAX_LEVELS 4

/* One POD replacing the reference's compile-time constants (helpers.h:16-20,
 * AcceleratedMLP.h:10-19, AF:15-16,183-184,243-245,345-346) and static C# Config
 * (TrainState.cs:45-72).  nof_config_default() fills the reference values. */
typedef struct nof_config {
  int32_t device;                         /* HIP device ordinal (reference: cudaSetDevice(0), MNcpp:10) */
  int32_t max_rays;                       /* capacity in rays per call (reference: 1024, helpers.h:18) */
  int32_t num_levels;                     /* 2 (helpers.h:16) */
  int32_t num_samples[NOF_MAX_LEVELS];    /* per level; 128, 128 (helpers.h:17); GPU: 64, 128, 256 or 512 */
  int32_t net_depth, net_width;           /* 8, 256.  Any network (MLP.cs:64-86; net_depth + net_depth_condition
                                             <= 14, widths <= 4096, 0 <= min_deg < max_deg <= 24, deg_view <= 24)
                                             runs; shapes other than the reference's 8x256 / 1x128 / skip 4 / PE
                                             (0, 16), 4 run on the any-shape path: NOF_PRECISION_F32 or
                                             NOF_PRECISION_F16_PRODUCTS only */
  int32_t net_depth_condition, net_width_condition; /* 1, 128 */
  int32_t skip_layer;                     /* 4 */
  int32_t min_deg_point, max_deg_point;   /* 0, 16 */
  int32_t deg_view;                       /* 4 */
  int32_t randomized;                     /* 1 (TrainState.cs:66) */
  int32_t white_bkgd;                     /* 1 (TrainState.cs:71) */
  float resample_padding;                 /* 0.01 (MNcs:12, AF:243) */
  float coarse_loss_mult;                 /* 0.1 (TrainState.cs:69, AF:345) */
  uint64_t seed;                          /* Philox key (reference: time(nullptr), MNcpp:44) */
  void* stream;                           /* hipStream_t, NULL = default stream */
  int32_t precision;                      /* NOF_PRECISION_*: MLP contraction arithmetic (build extension) */
  int32_t grad_buckets;                   /* 0: the weight-gradient split-K items are cut for the whole launch;
                                             1: cut per all-reduce bucket (layers 5..10 | 0..4), the cut the
                                             bucketed (attached, overlapped) launches use, so an unbucketed and
                                             a bucketed step sum every gradient element in the same order and a
                                             data-parallel run is bitwise the same attached or not.  Installing
                                             a gradient-bucket hook (nof_dp_attach) selects 1 (build extension) */
  int32_t lindisp;                        /* 0: t linear in depth; 1: linear in disparity (MipNerfModel.LinDisp,
                                             MNcs:14, SampleAlongRay MH:618-620); default 0 */
  int32_t ray_shape;                      /* NOF_RAY_CONICAL (MNcs:15, MH:391-402) or NOF_RAY_CYLINDRICAL
                                             (CylinderToGaussian MH:403-409); default conical */
  float density_bias;                     /* MipNerfModel.DensityBias (MNcs:20): sigma = softplus(z + bias); -1 */
  float rgb_padding;                      /* MipNerfModel.RgbPadding (MNcs:22): rgb = sigmoid(z) (1 + 2 p) - p;
                                             0.001, in [0, 0.5).  The activations themselves are the
                                             reference's fixed softplus / sigmoid (MNcs:19,21) */
  int32_t stop_level_grad;                /* MipNerfModel.StopLevelGrad (MNcs:13, declared and read by nothing): 1
                                             (default): level l + 1's t-values are constants of the backward; 0:
                                             t^{l+1} = resample(t^l, w^l; u) is differentiated in w^l and t^l, so
                                             a finer level's loss trains the coarser pass as a proposal (the
                                             discrete decisions of the resampler held at their forward values).
                                             0 runs on the any-shape path: NOF_PRECISION_F32 (the reference 8x256
                                             network is routed there) or NOF_PRECISION_F16_PRODUCTS; the fused
                                             8x256 modes produce no input gradient: NOF_ERR_UNSUPPORTED.  The
                                             forward is unchanged by the option; num_levels == 1: a no-op */
  float distortion_loss_mult;             /* lambda_d >= 0, default 0 = off (no counterpart in the reference): the
                                             distortion loss of mip-NeRF 360 on the LAST level's weights, added to
                                             the objective as lambda_d sum_r mu_r L_r / sum mu with
                                               L_r = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i
                                             over the midpoints m and widths delta of the normalised distance
                                             s(t) = (t - near) / (far - near), or with lindisp = 1
                                             (1/near - 1/t) / (1/near - 1/far).  Its gradient joins the integrator
                                             adjoint: every precision mode and network; with
                                             stop_level_grad = 0 its dL/dt also trains the coarser levels.  A ray
                                             whose far - near (lindisp: near, 1/near - 1/far) is not a positive
                                             finite number contributes nothing.  Negative or non-finite:
                                             NOF_ERR_INVALID_ARG.  nof_mipnerf_loss stays the photometric loss;
                                             the term is read with nof_mipnerf_distortion_loss */
} nof_config;
/* The struct grows at its end only (grad_buckets, then lindisp / ray_shape, then density_bias / rgb_padding, then
 * stop_level_grad, then distortion_loss_mult, which fills the 4 bytes of tail padding the 8-byte aligned struct had:
 * sizeof(nof_config) did not change with it, and an older binding's zeroed struct reads as 0 = off): a binding
 * compiled against an older header passes a shorter struct.  nof_config_size() is sizeof(nof_config) of
 * this library; a binding checks it against its own struct size before passing one. */
size_t nof_config_size(void);

enum { NOF_RAY_CONICAL = 0, NOF_RAY_CYLINDRICAL = 1 };

/* MLP contraction arithmetic.  Every mode holds operands and accumulators in fp32 between the
 * MFMAs; they differ in how the MFMAs form products.
 *   F32       : v_mfma_f32_16x16x4_f32 (exact fp32 fmaf chains).  Parity: 1e-5.
 *   F32_SPLIT : each fp32 operand as three bf16 pieces (24 significand bits), six
 *               v_mfma_f32_32x32x16_bf16 per product, fp32 accumulation.  Same 1e-5 parity.
 *   F16X2     : perf mode (BASELINE config 5 "fp16 on MFMA"): fp16 hi + lo pieces,
 *               three v_mfma_f32_32x32x16_f16 per product, backward deltas power-of-2 scaled.
 *               Parity: per-tensor relative L2 <= 2e-3 (the weight gradients take ONE fp16 product of the
 *               stored fp16 activation and delta: that product is the mode's error).
 *   F32_F16SPLIT : fp16 hi + lo pieces in EVERY contraction: the F16X2 forward and dX chain (three
 *               v_mfma_f32_16x16x32_f16 per product), activations and scaled deltas stored as fp32,
 *               the weight gradients split into hi + lo again (three v_mfma_f32_32x32x16_f16 per
 *               product).  22 significand bits per operand: the same 1e-5 parity as F32, within fp16's
 *               exponent range (activations below 65504; deltas power-of-2 scaled per level).
 *   F16       : plain fp16 mixed precision (BASELINE config 5's "fp16 activations on MFMA"): ONE
 *               v_mfma_f32_32x32x16_f16 per product, fp16(weight) x fp16(activation or scaled delta),
 *               fp32 accumulation; fp16 blocks and single-product weight gradients.  Parity: outputs
 *               and the integrator adjoint relative L2 <= 2e-3; gradients per tensor against fp64
 *               <= 2e-3, layer 0's W0 / b0 <= 6e-3 (fp16 pre-activations may gate a ReLU the other
 *               way; measured <= 4.9e-3, W0), all <= 2e-3 with the ReLU decisions fixed.
 *   F16_PRODUCTS : the any-shape path's perf mode, for every network (the reference's 8x256 runs on the
 *               any-shape path in this mode): every MLP contraction takes ONE fp16 product per term on
 *               v_mfma_f32_16x16x32_f16.  Both operands are rounded to fp16 (RNE) when they are staged for the
 *               MFMA, the products accumulate in fp32 in a fixed k order; activations, deltas, parameters and
 *               gradients stay fp32 in memory (F16 stores fp16 blocks: the two differ in storage as F16X2 and
 *               F32_F16SPLIT do).  The backward's delta operand is multiplied by a per-level power of two
 *               inside each product (from max |dsigma|, |drgb|, read on the device) and the sums by its exact
 *               inverse: nothing scaled is stored.  The view encoding's weight gradient over rays stays fp32.
 *               Heads, encodings, integrator, resampler and Adam are every mode's.  Parity: outputs and the
 *               integrator adjoint relative L2 <= 2e-3 against the fp64 oracle, gradients per tensor <= 2e-3
 *               with the GPU's ReLU decisions adopted.  Activations above 65504 become inf and surface
 *               through nof_mipnerf_numeric_status, as in the other fp16 modes. */
enum {
  NOF_PRECISION_F32 = 0,
  NOF_PRECISION_F32_SPLIT = 1,
  NOF_PRECISION_F16X2 = 2,
  NOF_PRECISION_F32_F16SPLIT = 3,
  NOF_PRECISION_F16 = 4,
  NOF_PRECISION_F16_PRODUCTS = 5
};

void nof_config_default(nof_config* cfg);
const char* nof_last_error(void);
const char* nof_version(void);

typedef struct nof_mipnerf nof_mipnerf;
typedef struct nof_mlp nof_mlp;
typedef struct nof_adam nof_adam;
typedef struct nof_gradcalc nof_gradcalc;

/* Func<uint64_t, int, float, uint64_t, uint64_t> getOutputGradient (AcceleratedMipNeRF.h:14-16):
 * (device compRgb [n][3], level, lossMultSum, device lossMults [n]) -> device dL/dCompRgb [n][3].
 * Invoked synchronously on the calling thread once per level in order 0..L-1 (MNcpp:125-127);
 * it may re-enter the library and must enqueue its work on the same stream. */
typedef uint64_t (*nof_output_grad_fn)(void* user, uint64_t dev_comp_rgb, int32_t level, float loss_mult_sum,
                                       uint64_t dev_loss_mults);

/* ---- AcceleratedMipNeRF (AcceleratedMipNeRF.h:10-41) --------------------------------------- */
/* ctor MNcpp:7-50 (which also builds AcceleratedMLP(16, 4), AcceleratedMipNeRF.h:18) */
nof_status nof_mipnerf_create(const nof_config* cfg, nof_mipnerf** out);
/* dtor MNcpp:151-176 */
nof_status nof_mipnerf_destroy(nof_mipnerf* h);
/* GetGradient MNcpp:52-144: host ray SoA (origins/dirs [n][3]; radii, nears, fars, loss_mults [n])
 * + loss-gradient callback -> 2L borrowed device gradient pointers [W0..W(L-1), b0..b(L-1)] (L = net_depth +
 * net_depth_condition + 2: 22 pointers [W0..W10, b0..b10] for the reference network). */
nof_status nof_mipnerf_get_gradient(nof_mipnerf* h, int32_t n, const float* origins, const float* directions,
                                    const float* radii, const float* nears, const float* fars,
                                    const float* loss_mults, nof_output_grad_fn cb, void* cb_user,
                                    float* const** out_dev_grads);
/* Same step with every input already resident in device memory and the loss gradient
 * (AF:347-361 / Program.LossFn, D14-D15 fixed) fused into the integrator adjoint:
 * dev_pixels [n][3]; loss_mult_sum = the GLOBAL sum over all data-parallel shards. */
nof_status nof_mipnerf_get_gradient_device(nof_mipnerf* h, int32_t n, const float* dev_origins,
                                           const float* dev_directions, const float* dev_radii,
                                           const float* dev_nears, const float* dev_fars,
                                           const float* dev_loss_mults, const float* dev_pixels,
                                           float loss_mult_sum, float* const** out_dev_grads);
/* Gradient flags (build extension; the reference overwrites per call, MLPcpp:101-129):
 *   NOF_GRAD_ACCUMULATE: add this call's gradient onto the arena (level 0 included) instead of
 *                        overwriting it -- micro-batching a large batch into several calls;
 *   NOF_GRAD_PUBLISH:    this call completes the step's gradient: with a bucket hook set
 *                        (nof_mipnerf_set_grad_buckets), its last level's weight gradients run as
 *                        NOF_GRAD_BUCKETS launches in reverse layer order and the hook fires after each
 *                        bucket's final values are enqueued, so its all-reduce overlaps the rest.
 * nof_mipnerf_get_gradient_device == _ex with flags = NOF_GRAD_PUBLISH. */
enum { NOF_GRAD_ACCUMULATE = 1, NOF_GRAD_PUBLISH = 2 };
#define NOF_GRAD_BUCKETS 2
nof_status nof_mipnerf_get_gradient_device_ex(nof_mipnerf* h, int32_t n, const float* dev_origins,
                                              const float* dev_directions, const float* dev_radii,
                                              const float* dev_nears, const float* dev_fars,
                                              const float* dev_loss_mults, const float* dev_pixels,
                                              float loss_mult_sum, uint32_t flags, float* const** out_dev_grads);
/* Bucket hook: invoked synchronously on the calling thread, in bucket order 0..NOF_GRAD_BUCKETS-1,
 * once the work producing the bucket's final gradient values has been enqueued on the model's
 * stream.  spans: (offset, count) in floats into the flat gradient arena; bucket 0 = W5..W10,
 * bucket 1 = W0..W4 and all biases.  Typical use: make a communication stream wait on the model
 * stream and enqueue the spans' all-reduce there.  fn = NULL removes the hook. */
typedef void (*nof_grad_bucket_fn)(void* user, int32_t bucket, int32_t nspans, const int64_t* span_offsets,
                                   const int64_t* span_counts);
nof_status nof_mipnerf_set_grad_buckets(nof_mipnerf* h, nof_grad_bucket_fn fn, void* user);
/* The spans the hook receives, from the 2L layer sizes of get_layer_sizes (host only; offsets and
 * counts hold at least 2 entries each). */
nof_status nof_grad_bucket_spans(int32_t bucket, const int32_t* layer_sizes, int32_t count, int64_t* offsets,
                                 int64_t* counts, int32_t* nspans);
/* GetLayerSizes MNcpp:146-149 -> get_layer_sizes MLPcpp:131-154 */
nof_status nof_mipnerf_layer_sizes(nof_mipnerf* h, int32_t* out, int32_t cap, int32_t* count);
/* public field `mlp` (AcceleratedMipNeRF.h:18), borrowed */
nof_status nof_mipnerf_mlp(nof_mipnerf* h, nof_mlp** out);
/* Philox stream position: key = seed, counter = (step, level, global ray id, k); ray_base = global
 * id of this shard's first ray.  `step` auto-increments after every get_gradient call. */
nof_status nof_mipnerf_set_rng(nof_mipnerf* h, uint64_t seed, uint32_t step, uint32_t ray_base);
nof_status nof_mipnerf_get_rng(nof_mipnerf* h, uint64_t* seed, uint32_t* step, uint32_t* ray_base);

/* Device views of one level's buffers from the last call (borrowed; for tests / tooling). */
typedef struct nof_level_view {
  int32_t n, samples;
  const float* t;          /* [n][S+1] */
  const float* weights;    /* [n][S] */
  const float* comp_rgb;   /* [n][3] */
  const float* density;    /* [n][S]   (post softplus) */
  const float* rgb;        /* [n][S][3] (post sigmoid/padding) */
  const float* density_grad; /* [n][S] */
  const float* rgb_grad;   /* [n][S][3] */
} nof_level_view;
nof_status nof_mipnerf_level_view(nof_mipnerf* h, int32_t level, nof_level_view* out);
/* stop_level_grad = 0: borrowed device views of the last step's cross-level terms (tests and tooling):
 * *w_grad = q^level [n][S] = dL/dw^level from level + 1's resampler (NULL for the last level), *t_grad =
 * dL/dt^level [n][S + 1] = integrator + encoding + bin-edge terms (NULL for level 0, whose t is a constant).
 * Both NULL with stop_level_grad = 1, unless the interlevel loss is on (nof_mipnerf_set_interlevel_loss): then
 * *w_grad = q^level holds that loss's dL/dw^level (at stop_level_grad = 0 added to the resampler's) for every
 * level but the last, and *t_grad stays NULL at stop_level_grad = 1. */
nof_status nof_mipnerf_cross_view(nof_mipnerf* h, int32_t level, const float** w_grad, const float** t_grad);
/* Ray gradients, for camera refinement: with the option on, every step also leaves dL/d origins and
 * dL/d directions of its own rays (radius, near, far, the t-values and the Philox uniforms held constant).
 * Any-shape objects only (any network in F32 / F16_PRODUCTS; the reference 8x256 in F16_PRODUCTS, or in F32 with
 * stop_level_grad = 0); a fused 8x256 object: NOF_ERR_UNSUPPORTED, the object staying usable.  Allocates; call
 * before the step.  enable = 0 frees nothing and launches nothing more.  The parameter gradients are bitwise the
 * same with the option on or off. */
nof_status nof_mipnerf_set_ray_grad(nof_mipnerf* h, int32_t enable);
/* the last step's dL/d origins, dL/d directions [n][3], borrowed device pointers (overwritten by the next step;
 * with NOF_GRAD_ACCUMULATE too: they belong to the call's own rays); NOF_ERR_INVALID_ARG before a step with the
 * option on */
nof_status nof_mipnerf_ray_grad(nof_mipnerf* h, const float** dev_o_grad, const float** dev_d_grad);
/* sum over rays and levels of lambda_l * m_r |C - p|^2 / sum m (fused path only; synchronises) */
nof_status nof_mipnerf_loss(nof_mipnerf* h, float* out);
/* nof_config.distortion_loss_mult's term of the last gradient step, lambda_d sum_r mu_r L_r / sum mu (either
 * gradient entry; the per-ray terms summed on the host in ray order; synchronises).  0 with the option off;
 * NOF_ERR_INVALID_ARG before a step. */
nof_status nof_mipnerf_distortion_loss(nof_mipnerf* h, float* out);
/* The interlevel (proposal) loss of mip-NeRF 360 (no counterpart in the reference).  mult = lambda_p
 * >= 0, 0 = off (the default: every launch as without the option).  For every level l < num_levels - 1 the
 * objective gains lambda_p sum_r mu_r L_r^l / sum mu with
 *   L_r^l = sum_i max(0, w_i - bound_i)^2 / (w_i + 2^-23),
 * (t, w) the LAST level's intervals and weights, a constant of the backward (also at stop_level_grad = 0), and
 * bound_i the sum of level l's weights over its intervals that touch [t_i, t_{i+1}] (the published lossfun_outer):
 * level l's weight histogram is pushed to be an upper envelope of the last level's.  The term has a gradient in
 * level l's weights only; it joins that level's integrator adjoint as q^l.  Every precision mode, network and both
 * gradient entries; with stop_level_grad = 0 it is added to the q^l of the resampler adjoint.  The levels share one
 * MLP (mip-NeRF): this is 360's loss, not its separate proposal network.  nof_config is not extended (its tail
 * padding is used up): the option is this setter.  num_levels == 1: a no-op.  Negative or non-finite:
 * NOF_ERR_INVALID_ARG (interlevel_loss_mult).  The first mult > 0 allocates q^l and the per-ray terms. */
nof_status nof_mipnerf_set_interlevel_loss(nof_mipnerf* h, float mult);
/* its term of the last gradient step, summed on the host in level order, then ray order (synchronises); 0 with the
 * option off; NOF_ERR_INVALID_ARG before a step.  nof_mipnerf_loss stays the photometric loss. */
nof_status nof_mipnerf_interlevel_loss(nof_mipnerf* h, float* out);
/* Scene contraction for unbounded scenes (mip-NeRF 360's; no counterpart in the reference).  With
 * NOF_CONTRACT_SPHERE every sample's Gaussian (mean m, diagonal covariance v, as the cast makes them in world
 * coordinates) is mapped into the ball of radius 2 before it is encoded: |m| <= 1 (and NaN) untouched, else
 *   m' = (2 - 1 / n) m / n,  v' = diag(J diag(v) J^T),  J = a (I - u u^T) + b u u^T,
 * n = |m|, u = m / n, a = (2 n - 1) / n^2, b = 1 / n^2 (the linearised covariance, kept diagonal as the IPE is).
 * It applies wherever the object casts rays itself: the training step through both gradient entries,
 * nof_mipnerf_render_device and nof_dataset_render_view, and to the adjoints of stop_level_grad = 0 and
 * nof_mipnerf_set_ray_grad.  nof_mlp_get_output takes caller-encoded inputs and is unaffected.  Cameras are expected
 * inside the unit ball; lindisp = 1 with a large far plane goes with it.  A hyper-parameter, not state: checkpoints
 * do not hold it; it takes effect from the next call and allocates nothing (nof_config is not extended: the option
 * is this setter).  Any-shape objects only (as nof_mipnerf_set_ray_grad); a fused 8x256 object: NOF_ERR_UNSUPPORTED,
 * the object staying usable (NOF_CONTRACT_NONE is accepted there).  An unknown mode: NOF_ERR_INVALID_ARG. */
enum { NOF_CONTRACT_NONE = 0, NOF_CONTRACT_SPHERE = 1 };
nof_status nof_mipnerf_set_contraction(nof_mipnerf* h, int32_t mode);
nof_status nof_mipnerf_get_contraction(nof_mipnerf* h, int32_t* mode);
/* Diagnostic: which of the fused 8x256 training step's launch fusions are in force.  Bit flags, all
 * on by default; clearing one runs that part the unfused way.  It never changes a result: gradients, parameters,
 * colours and the loss are bit for bit the same at every setting, which is what the A/B measurements and
 * tests/test_gpu_step_fusion.py rely on.
 *   NOF_STEP_FUSION_BWD_PAIR   fp32 / f16x2 / f16split: the dX chains of a pair of levels in ONE k_mlp_bwd16 launch
 *                              (both gradient entries; nof_mlp_get_gradient, one level per call, always launches
 *                              per level); cleared: one launch per level.
 *   NOF_STEP_FUSION_VIEW_TABLES  the same modes: the step's pack launch writes every ray's view-PE row and
 *                              view-layer bias b9 + W9[:, 256:283] PE(d) once, and k_mlp_fwd16 reads them; cleared:
 *                              every wave of every level computes its ray's in the kernel's prologue, as
 *                              nof_mlp_get_output and nof_mipnerf_render_device always do.
 * Takes effect from the next call, allocates nothing, is not held by checkpoints.  Unknown bits:
 * NOF_ERR_INVALID_ARG.  Any-shape objects and the F16 / split modes accept it and ignore it. */
enum { NOF_STEP_FUSION_BWD_PAIR = 1, NOF_STEP_FUSION_VIEW_TABLES = 2, NOF_STEP_FUSION_ALL = 3 };
nof_status nof_mipnerf_set_step_fusion(nof_mipnerf* h, uint32_t flags);
/* Per-view appearance embeddings (NeRF-W / mip-NeRF 360's GLO vectors; no counterpart in the reference; DESIGN.md
 * 6j).  With appearance_views = V and appearance_dim = G > 0 the model owns a zero-initialised fp32 table E [V][G]
 * outside the parameter arena, and the view layer (layer net_depth + 1) has in = W + Vd + G: its input for every
 * sample of ray r is [h | viewPE(d_r) | E[view(r)]].  The parameter layout, the Glorot initialisation (fan-in = the
 * widened in), nof_mipnerf_layer_sizes, Adam, checkpoints and the data-parallel arena see only a wider layer; the
 * table is not in checkpoints.  Any-shape objects only: a fused 8x256 object (precision modes 0-4 with the reference
 * shape and stop_level_grad = 1) with G > 0 is NOF_ERR_UNSUPPORTED.  ext == NULL or appearance_dim == 0 is exactly
 * nof_mipnerf_create.  size = sizeof the caller's struct (the struct grows at its end).  NOF_ERR_INVALID_ARG, before
 * any device call: dim < 0, dim > 256, dim > 0 with views <= 0, views * dim >= 2^31, size too small. */
typedef struct nof_model_ext {
  uint32_t size;
  int32_t appearance_views, appearance_dim;
} nof_model_ext;
nof_status nof_mipnerf_create_ex(const nof_config* cfg, const nof_model_ext* ext, nof_mipnerf** out);
/* Borrowed device pointers to E and to its gradient dE, each views x dim floats.  The caller owns the update: a
 * second nof_adam created with layer_sizes = {views * dim} steps the table (and a data-parallel caller all-reduces
 * dE itself, as the pose buffer).  dE[v][g] = sum over levels, then over the rays r of view v, of
 * sum_o gray^l[r][o] W_view[o][W + Vd + g] (gray^l: the view layer's deltas summed over the ray's samples), formed
 * by every step through either gradient entry in a fixed order (bitwise repeatable): overwritten, or added to with
 * NOF_GRAD_ACCUMULATE; a view without a ray gets 0 (accumulating: stays as it is).  A model without appearance:
 * NOF_ERR_INVALID_ARG. */
nof_status nof_mipnerf_appearance(nof_mipnerf* h, float** dev_table, float** dev_grad, int32_t* views, int32_t* dim);
/* The view ids [n] (device ints) of the rays of the NEXT single call that casts rays: either gradient entry, or
 * nof_mipnerf_render_device.  They are read in that call's stream work; the call then resets the pointer to NULL.
 * A ray whose id lies outside [0, views) reads the zero vector and contributes to no table row (lib/libnof_check.so
 * sets NOF_CHECK_GATHER for it).  A gradient step on an appearance model with no ids set: NOF_ERR_INVALID_ARG ("ray
 * views"), the object staying usable. */
nof_status nof_mipnerf_set_ray_views(nof_mipnerf* h, const int32_t* dev_view_ids);
/* The constant view of calls that have no per-ray ids: nof_mipnerf_render_device without ids,
 * nof_dataset_render_view and nof_mlp_get_output.  -1 (the default): the zero vector.  Out of range:
 * NOF_ERR_INVALID_ARG.  (nof_mlp_get_gradient leaves dE alone.) */
nof_status nof_mipnerf_set_render_appearance(nof_mipnerf* h, int32_t view);
/* Non-finite detection, every precision mode (the f16x2 perf mode's fp16 activation range is its
 * stated limit: an overflow surfaces here instead of silently): NOF_NUMERIC_FORWARD = a training
 * forward produced a non-finite composite colour; NOF_NUMERIC_DELTA = the f16x2 delta scaling saw a
 * non-finite output gradient.  Bits accumulate until cleared (clear != 0).  Synchronises. */
#define NOF_NUMERIC_FORWARD 1u
#define NOF_NUMERIC_DELTA 2u
nof_status nof_mipnerf_numeric_status(nof_mipnerf* h, uint32_t* flags, int32_t clear);
/* Device-side bounds checks (no reference counterpart; its CUDA path has real out-of-bounds writes,
 * SURVEY.md Appendix A): a library built with `make check` (lib/libnof_check.so, -DNOF_DEVICE_CHECKS)
 * checks launch geometry, sample bins, weight-gradient problem geometry and record indices inside
 * the kernels; a failed check sets its bit (NOF_CHECK_*) instead of trapping.  Synchronises the
 * current device and returns the bits seen on it since the last clear.  The product build returns
 * NOF_ERR_UNSUPPORTED.  nof_device_checks_selftest fails NOF_CHECK_SELFTEST on purpose. */
#define NOF_CHECK_MLP_BLOCK (1u << 0)
#define NOF_CHECK_SAMPLE_IDX (1u << 1)
#define NOF_CHECK_WGRAD_GEOM (1u << 2)
#define NOF_CHECK_GATHER (1u << 3)
#define NOF_CHECK_SELFTEST (1u << 31)
nof_status nof_device_checks(uint32_t* bits, int32_t clear);
nof_status nof_device_checks_selftest(void);

/* ---- evaluation ------------------------------------------------------------
 * Forward-only two-level render: replaces MipNerfModel.Call(rays, randomized, whiteBackground)
 * (MipNerfModel.cs:36-97, whose level-1 resampling reads an empty array: D22).  Per level the
 * composite rgb, the clamped weighted-midpoint distance and the accumulated opacity
 * (VolumetricRendering, MipHelpers.cs:472-492).  Inputs device-resident; outputs device, borrowed
 * until the next call on h.  randomized != 0 draws jitter from the model's Philox state (set_rng)
 * without advancing it. */
typedef struct nof_render_out {
  int32_t num_levels;
  const float* comp_rgb[NOF_MAX_LEVELS];  /* [n][3] */
  const float* distance[NOF_MAX_LEVELS];  /* [n] */
  const float* acc[NOF_MAX_LEVELS];       /* [n] */
} nof_render_out;
nof_status nof_mipnerf_render_device(nof_mipnerf* h, int32_t n, const float* dev_origins, const float* dev_dirs,
                                     const float* dev_radii, const float* dev_nears, const float* dev_fars,
                                     int32_t randomized, int32_t white_bkgd, nof_render_out* out);

/* ---- ray-batch ingestion ---------------------------------------------------
 * Replaces BinDataset (BinDataset.cs:10-53): 64-byte little-endian records {origin[3], direction[3],
 * viewdir[3], radius, near, far, lossmult, rgb[3]} (BinDataset.cs:40-49) held in HBM; a batch is a
 * device gather of records drawn with replacement (BinDataset.cs:34: _rng.Next(numSamples)) by a
 * Philox counter of (seed, step, global ray id), so shards of one batch draw what the whole batch
 * would.  Batch buffers are device SoA owned by the dataset, valid until its next call. */
typedef struct nof_dataset nof_dataset;
typedef struct nof_batch {
  int32_t n;
  float *origins, *directions, *viewdirs; /* [n][3] */
  float *radii, *nears, *fars, *loss_mults; /* [n] */
  float* pixels;                          /* [n][3] */
  int32_t* record_index;                  /* [n] record drawn for each ray */
} nof_batch;
/* The whole record file is copied into HBM, unless it exceeds half the device's free memory: then it
 * is streamed as by nof_dataset_open_streaming. */
nof_status nof_dataset_open(const char* path, int32_t device, nof_dataset** out);
/* A record file resident in HBM iff it holds at most max_resident_records records; otherwise STREAMED
 * (files larger than HBM): each nof_dataset_next reads the batch's records from the file, as
 * BinDataset.LoadBatch does (BinDataset.cs:31-38), into pinned host memory, copies them to the device
 * and unpacks them with the same gather — batches bit-identical to the resident dataset's — while the
 * records of the next step of the same request (step + 1) are prefetched on a host thread. */
nof_status nof_dataset_open_streaming(const char* path, int32_t device, int64_t max_resident_records,
                                      nof_dataset** out);
nof_status nof_dataset_is_streaming(nof_dataset* ds, int32_t* streaming);
nof_status nof_dataset_from_host(const float* records /* count x 16 */, int64_t count, int32_t device,
                                 nof_dataset** out);
nof_status nof_dataset_count(nof_dataset* ds, int64_t* count);
/* loss_mult_sum != NULL: also returns the batch's loss-multiplier sum (synchronises the stream) */
nof_status nof_dataset_next(nof_dataset* ds, int32_t n, uint64_t seed, uint32_t step, uint32_t ray_base,
                            void* stream, nof_batch* out, float* loss_mult_sum);
nof_status nof_dataset_destroy(nof_dataset* ds);

/* ---- device ray generation ---------------------------------------------------
 * Dataset.GenerateRays (Dataset.cs:111-176): pinhole directions d = R ((x - w/2 + .5)/f,
 * -(y - h/2 + .5)/f, -1) (unnormalised), origin = pose translation, viewdir = normalize(d),
 * radius = |d(x,y) - d(x+1,y)| 2/sqrt(12) (0 in the last column, as the reference), lossmult 1;
 * ndc != 0: the LLFF override (Dataset.cs:268-293): ConvertToNdc (near 1, :295-308) and the radius
 * from the NDC origins of the x and y neighbours.  poses: host, V x 12 floats (rotation row-major,
 * then translation).  images: device [V][H][W][3] or NULL (rgb = 0).  Output: BinDataset records
 * (V*H*W x 16 floats, view-major then row-major pixels) on the device. */
nof_status nof_generate_rays(const float* host_poses, int32_t num_views, int32_t width, int32_t height, float focal,
                             float near_, float far_, int32_t ndc, const float* dev_images, float* dev_records,
                             void* stream);
/* The same, straight into a device-resident dataset (then nof_dataset_next). */
nof_status nof_dataset_generate(const float* host_poses, int32_t num_views, int32_t width, int32_t height, float focal,
                                float near_, float far_, int32_t ndc, const float* dev_images, int32_t device,
                                nof_dataset** out);

/* ---- multiscale, image-backed scenes ------------------------------------------------------------
 * mip-NeRF trains on every image at several resolutions at once.  The reference declares the loader
 * (DatasetType.Multicam, TrainState.cs:41,48) and never builds it (Multicam.LoadRenderings throws,
 * Dataset.cs:203-207).  Here scale s of num_scales (1..4) is the image set halved s times: width >> s,
 * height >> s, focal / 2^s (so a pixel's radius doubles per scale), the scene's near and far, and the
 * loss multiplier 4^s.  nof_multiscale_layout fills the per-scale table (arrays of 4; entries past
 * num_scales are 0) and the virtual record order: scale-major, then view-major, then row-major pixels,
 * firsts[s] = num_views * sum_{j<s} w_j h_j, count = num_views * sum_s w_s h_s.  A batch's record_index maps
 * back to (scale, view, y, x) through it.  Host only, no device.  NOF_ERR_INVALID_ARG: num_scales
 * outside 1..4, width or height not divisible by 2^(num_scales-1), a last scale under 2 x 2,
 * focal <= 0, count > 0xFFFFFFFF.
 * disable_multiscale_loss != 0 is Config.DisableMultiscaleLoss (TrainState.cs:65): every scale's
 * multiplier is 1. */
nof_status nof_multiscale_layout(int32_t width, int32_t height, float focal, int32_t num_scales,
                                 int32_t disable_multiscale_loss, int32_t num_views, int32_t* w /* [4] */,
                                 int32_t* h /* [4] */, float* focals /* [4] */, float* lossmults /* [4] */,
                                 int64_t* firsts /* [4] */, int64_t* count);
/* The loader the reference leaves unbuilt (Dataset.cs:203-207), image-backed: the dataset keeps the
 * poses and an image pyramid in HBM (12 bytes per ray in place of a 64-byte record) and
 * nof_dataset_next generates each drawn record inside its gather launch, with the arithmetic of
 * nof_generate_rays (bit-identical records).  dev_images: device [V][H][W][3] fp32, read only during
 * the call (NULL: rgb = 0); pyramid level s is the 2 x 2 mean of level s-1,
 * ((a + b) + (c + d)) * 0.25f over (2y,2x), (2y,2x+1), (2y+1,2x), (2y+1,2x+1) per channel in fp32.
 * Arguments are refused as by nof_multiscale_layout (and null poses) before any device call.
 * nof_dataset_count / _next / _is_streaming (0) / _destroy and nof_dp_train_step take the result. */
nof_status nof_dataset_from_images(const float* host_poses, int32_t num_views, int32_t width, int32_t height,
                                   float focal, float near_, float far_, int32_t ndc, const float* dev_images,
                                   int32_t num_scales, int32_t disable_multiscale_loss, int32_t device,
                                   nof_dataset** out);
/* Every record of the dataset, in order, into dev_records (count x 16 floats, device), asynchronously
 * on stream: what the Multicam loader of Dataset.cs:203-207 would have handed to BinDataset
 * (BinDataset.cs:40-49), e.g. to write a multiscale record file.  Image-backed: generated; records
 * resident in HBM: copied; streaming: NOF_ERR_UNSUPPORTED (the file is the record list). */
nof_status nof_dataset_materialize(nof_dataset* ds, float* dev_records, void* stream);
/* LLFFDataset.RecenterPoses (Dataset.cs:309-319) in place on host poses (V x 12). */
nof_status nof_recenter_poses(float* host_poses, int32_t num_views);

/* ---- training state ----------------------------------------------------------
 * Config.SaveEvery (TrainState.cs:59) is declared but never implemented by the reference.  A
 * checkpoint holds the parameters, Adam's moments and step, and the Philox state, so a resumed run
 * continues bit-identically.  Files are checksummed and written atomically (tmp + rename). */
nof_status nof_checkpoint_save(const char* path, nof_mipnerf* h, nof_adam* adam);
nof_status nof_checkpoint_load(const char* path, nof_mipnerf* h, nof_adam* adam);

/* ---- data parallelism over RCCL (SURVEY.md 8b "(new) DP", 8e) --------------------------------------
 * Rays shard across GPUs (global ray ids via nof_mipnerf_set_rng; the global loss-mult sum passed
 * to get_gradient_device); the only exchange is an in-place all-reduce (sum) of the flat gradient
 * arena, after which every rank runs the same Adam step on identical bits.  For hosts without
 * torch.distributed (the reference's C# driver):
 *   one process per GPU: rank 0 calls nof_dp_unique_id and shares the 128 bytes (any channel);
 *                        every rank calls nof_dp_init_rank;
 *   one process, n GPUs: nof_dp_init_all fills n handles; nof_dp_allreduce_grads_all groups the
 *                        n all-reduces. */
typedef struct nof_dp nof_dp;
nof_status nof_dp_unique_id(uint8_t id[128]);
/* Communicators are non-blocking: initialisation waits at most timeout_ms for every rank to join
 * (0 = NOF_DP_TIMEOUT_MS from the environment, else 300 s), then aborts and returns NOF_ERR_RCCL. */
nof_status nof_dp_init_rank(const uint8_t id[128], int32_t world, int32_t rank, int32_t device, nof_dp** out);
nof_status nof_dp_init_rank_timeout(const uint8_t id[128], int32_t world, int32_t rank, int32_t device,
                                    int32_t timeout_ms, nof_dp** out);
nof_status nof_dp_init_all(int32_t ndev, const int32_t* devices, nof_dp** out /* ndev handles */);
nof_status nof_dp_allreduce(nof_dp* dp, float* dev_buf, int64_t count, void* stream);
/* all-reduce of the model's gradient arena on its stream (or streams[i]) */
nof_status nof_dp_allreduce_grads(nof_dp* dp, nof_mipnerf* h, void* stream);
nof_status nof_dp_allreduce_grads_all(int32_t n, nof_dp* const* dps, nof_mipnerf* const* hs, void* const* streams);
/* Overlapped mode: installs the model's bucket hook (nof_mipnerf_set_grad_buckets) so that every
 * NOF_GRAD_PUBLISH call all-reduces each bucket on comm_stream (NULL = an internal stream) as soon
 * as it is final, and the model's stream waits for the last one (work enqueued after the call, e.g.
 * Adam, sees the reduced gradient).  h = NULL detaches. */
nof_status nof_dp_attach(nof_dp* dp, nof_mipnerf* h, void* comm_stream);
/* Failure detection: waits until the last all-reduce enqueued through dp has completed, polling
 * ncclCommGetAsyncError; on an asynchronous RCCL error or after timeout_ms (0 = the init timeout)
 * the communicator is aborted and NOF_ERR_RCCL returned.  Every later call on an aborted dp
 * returns NOF_ERR_RCCL (never hangs). */
nof_status nof_dp_wait(nof_dp* dp, int32_t timeout_ms);
/* End of a training step, one step behind: the same bounded wait for the all-reduces of the PREVIOUS
 * call's step (this step's become the next call's), so the host can enqueue the next step while this
 * one's exchange runs.  A final nof_dp_wait covers the last step. */
nof_status nof_dp_step_end(nof_dp* dp, int32_t timeout_ms);
nof_status nof_dp_abort(nof_dp* dp);
nof_status nof_dp_destroy(nof_dp* dp);
/* Loopback group (SURVEY.md §4 "T0 DP logic"): k <= 8 communicators of this process on ONE device
 * whose all-reduce sums the k members' buffers on the device in member order.  Every nof_dp_* call
 * above works on them unchanged (grouped, attached / bucketed, nof_dp_train_step), so the
 * data-parallel choreography runs with k models on one GPU.  A loopback collective completes when
 * its last member arrives; the members' streams then wait for it. */
nof_status nof_dp_init_loopback(int32_t k, int32_t device, nof_dp** out /* k handles */);
/* One data-parallel TrainStep (Program.cs:48-62) — what a C# driver calls once per step.
 * n replicas: one per device (nof_dp_init_all), a loopback group (n = k), or this process's one rank
 * (n = 1, nof_dp_init_rank: the shard is its rank's); dps = NULL: one replica, no exchange.
 * Replica r (rank r) takes the contiguous shard [r s, (r + 1) s) of the global batch (s =
 * global_batch / world; global ray ids: the same rays and Philox samples whatever the sharding),
 * gathered from datasets[r] for (seed, step); every shard normalises by the GLOBAL loss-multiplier
 * sum; a shard runs as shard / micro_batch micro-batches (0 = one), the later ones accumulating;
 * the gradient arenas are all-reduced (bucket by bucket when the communicators are attached, else one
 * grouped all-reduce); every replica applies Adam(lr); then a bounded nof_dp_wait.  Replica
 * parameters stay bitwise identical.  *loss_mult_sum (optional) = the global sum.  A model with appearance
 * embeddings (nof_mipnerf_create_ex) is refused, NOF_ERR_UNSUPPORTED: the table's all-reduce and its Adam are the
 * caller's, as the pose buffer's are. */
nof_status nof_dp_train_step(int32_t n, nof_dp* const* dps, nof_mipnerf* const* models, nof_adam* const* adams,
                             nof_dataset* const* datasets, int32_t global_batch, int32_t micro_batch, uint64_t seed,
                             int32_t step, float lr, float* loss_mult_sum);

/* Image metrics on device images [H][W][3] (float, any range; max_val as MathHelpers' maxVal):
 * psnr = MseToPsnr(mean squared error) (MipHelpers.cs:672); ssim = ComputeSsimAverage with the
 * reference defaults (11x11 Gaussian, sigma 1.5, k1 0.01, k2 0.03, zero-padded 'same' convolution,
 * variances and covariance clipped at 0; MipHelpers.cs:685-736,903-927).  Synchronises the stream. */
nof_status nof_image_metrics(const float* dev_img0, const float* dev_img1, int32_t width, int32_t height,
                             float max_val, float* psnr, float* ssim, void* stream);

/* ---- the test split: whole views rendered and scored on the device ------------------------------
 * The reference declares the test side and leaves it empty: Split.Test (Dataset.cs:13-17) whose
 * TestInit throws (Dataset.cs:107-110), and Config.LlffHold, Config.RenderPath, Config.GcEvery ("the
 * number of steps to render an image") and Config.TestRenderInterval (TrainState.cs:52-53,63-64), read
 * by nothing.  Here a whole view of an image-backed dataset (nof_dataset_from_images), at one of its
 * scales, is rendered in one call: per chunk of the model's max_rays pixels (row-major from pixel 0, the
 * last chunk ragged) the rays are generated from the pose — the bits nof_dataset_materialize writes for
 * that view and scale, no record is stored —, go through the inference forward of
 * nof_mipnerf_render_device (MipNerfModel.Call, MipNerfModel.cs:36-97; randomized 0, the model's
 * white_bkgd: the images are those of nof_mipnerf_render_device on the materialised records in the same
 * chunks, bitwise) and are written into the caller's image-shaped device buffers.  Everything is
 * enqueued on the model's stream, with no host round trip between chunks; the chunk ray buffers are
 * the dataset's own (a batch of nof_dataset_next stays valid and unchanged) and the model's Philox
 * state is not advanced.  Nothing is allocated after the first call with a given max_rays.
 *
 * metrics != NULL (a scene built with images; view, not host_pose): level l's rgb is scored against the
 * pyramid level the dataset keeps for (scale, view): per channel d = C - p and d * d in fp32, summed
 * over channels, pixels and chunks in fp64 in a fixed order (no atomics: bit-identical run to run),
 * mse[l] = sum / (3 w h), psnr[l] = MseToPsnr(mse[l]) (MipHelpers.cs:672).  flags & NOF_VIEW_SSIM: ssim =
 * nof_image_metrics' SSIM of the last level against the same pixels (the dataset keeps the image itself
 * when out->rgb[last] is NULL); otherwise NaN.  The call then synchronises the model's stream once, at
 * the end; with metrics == NULL it does not synchronise.
 *
 * host_pose != NULL: 12 host floats (rotation row-major, then translation), a novel pose rendered with
 * the scene's intrinsics at `scale` (what Config.RenderPath needs; the reference's own test poses,
 * Dataset.cs:320-321, are not implemented and not built here); view is ignored, metrics must be NULL.
 *
 * Refused before any launch, the objects staying usable: NOF_ERR_UNSUPPORTED for a dataset that is not
 * image-backed (resident records or streaming); NOF_ERR_INVALID_ARG for view or scale out of range,
 * dataset and model on different devices, metrics on a scene built without images, metrics together
 * with host_pose, unknown flag bits, and null ds, model or out. */
typedef struct nof_view_out {            /* caller-provided device buffers, any may be NULL */
  float* rgb[NOF_MAX_LEVELS];            /* [h_s][w_s][3] per level */
  float* distance;                       /* [h_s][w_s], last level */
  float* acc;                            /* [h_s][w_s], last level */
} nof_view_out;
typedef struct nof_view_metrics {
  int32_t width, height, num_levels;
  double mse[NOF_MAX_LEVELS];
  float psnr[NOF_MAX_LEVELS];
  float ssim;                            /* last level; NaN unless NOF_VIEW_SSIM */
} nof_view_metrics;
#define NOF_VIEW_SSIM 1u
/* image-backed datasets: views, scales and the per-scale sizes (arrays of 4, 0 past num_scales);
 * NOF_ERR_UNSUPPORTED for any other dataset */
nof_status nof_dataset_scene_info(nof_dataset* ds, int32_t* num_views, int32_t* num_scales,
                                  int32_t* w, int32_t* h, int32_t* has_images);
nof_status nof_dataset_render_view(nof_dataset* ds, nof_mipnerf* model, int32_t view, const float* host_pose,
                                   int32_t scale, uint32_t flags, const nof_view_out* out,
                                   nof_view_metrics* metrics);
/* Camera refinement.  Image-backed, ndc = 0: the gradients [n][3] of the rays of the dataset's LAST
 * nof_dataset_next batch (its record_index; n at most that batch's) summed per view -> dev_pose_grad [V][12]
 * (rotation row-major, then translation; d = R cam, o = t, the radius held constant).  accumulate = 0 overwrites
 * (a view that drew no ray: 0), else adds (such a view's row is left as it is).  Bitwise repeatable.
 * NOF_ERR_UNSUPPORTED: not image-backed, or an NDC scene (ConvertToNdc is not differentiated here). */
nof_status nof_dataset_pose_grad(nof_dataset* ds, int32_t n, const float* dev_o_grad, const float* dev_d_grad,
                                 float* dev_pose_grad, int32_t accumulate, void* stream);
/* The view of every ray of the dataset's LAST nof_dataset_next batch (its record_index decoded as
 * nof_multiscale_layout orders the records) -> dev_view_ids [n], the ids nof_mipnerf_set_ray_views takes.
 * Image-backed datasets only (else NOF_ERR_UNSUPPORTED); n larger than that batch: NOF_ERR_INVALID_ARG. */
nof_status nof_dataset_batch_views(nof_dataset* ds, int32_t n, int32_t* dev_view_ids, void* stream);
/* the image-backed dataset's pose table, V x 12 host floats.  set: ordered with the dataset's next gather and with
 * nof_dataset_render_view (it waits for the device, then copies); rays are made from the table inside the
 * gather, so nothing is regenerated. */
nof_status nof_dataset_get_poses(nof_dataset* ds, float* host_poses);
nof_status nof_dataset_set_poses(nof_dataset* ds, const float* host_poses);

/* ---- AcceleratedMLP (AcceleratedMLP.h:7-45) -------------------------------------------------- */
/* get_output MLPcpp:214-255: encoded inputs in device memory (enc_pos [n*S][96] in the reference's
 * feature order, enc_dir [n][27] per ray, D5; any-shape networks: [n*S][6 (max_deg - min_deg)] and
 * [n][3 + 6 deg_view]) -> (density [n*S], rgb [n*S][3]) borrowed.  The inputs are read during the
 * call's stream work only (the library keeps its own copy for get_gradient).  The reference returns
 * (density, rgb) but its caller binds them swapped (D9): here they are named. */
nof_status nof_mlp_get_output(nof_mlp* m, const float* dev_enc_pos, const float* dev_enc_dir, int32_t level,
                              int32_t n_rays, int32_t samples, uint64_t* dev_density, uint64_t* dev_rgb);
/* get_gradient MLPcpp:256-321: dL/d rgb [n*S][3] and dL/d density [n*S] of `level`'s last forward.
 * level 0 overwrites the gradient arena, level > 0 accumulates (sum over levels, D10). */
nof_status nof_mlp_get_gradient(nof_mlp* m, const float* dev_color_grad, const float* dev_density_grad,
                                int32_t level, float* const** out_dev_grads);
/* ... with NOF_GRAD_* flags (ACCUMULATE: level 0 accumulates too; PUBLISH: see above) */
nof_status nof_mlp_get_gradient_ex(nof_mlp* m, const float* dev_color_grad, const float* dev_density_grad,
                                   int32_t level, uint32_t flags, float* const** out_dev_grads);
/* allParams / allGradients (AcceleratedMLP.h:24-25): 2L views into one flat arena (22 for 8x256) */
nof_status nof_mlp_params(nof_mlp* m, float* const** out);
nof_status nof_mlp_grads(nof_mlp* m, float* const** out);
nof_status nof_mlp_flat_params(nof_mlp* m, float** out, int64_t* count);
nof_status nof_mlp_flat_grads(nof_mlp* m, float** out, int64_t* count);
nof_status nof_mlp_layer_sizes(nof_mlp* m, int32_t* out, int32_t cap, int32_t* count);
/* Internal per-level buffers of the last forward/backward (borrowed; tests and tooling).  Block
 * layout: element (feature f, sample m) of an [F]-feature tensor lives at
 * (m/32)*F*32 + f*32 + ((m%32) ^ (f%32)).  masks: [M/32][9][64][4] uint32 ReLU bits. */
typedef struct nof_mlp_debug {
  int32_t M;              /* samples of this level's last forward */
  const float* act_in;    /* [128]-feature blocks: IPE 0..95 | view PE 96..122 | 0 */
  const float* act_h;     /* 8 consecutive [256]-feature tensors h0..h7 (stride M*256) */
  const float* act_h9;    /* [128]-feature blocks */
  const uint32_t* masks;
  const float* zhead;     /* [M][4]: z_density, z_rgb[3] (pre-activation heads) */
  const float* delta;     /* 8 consecutive [256]-feature dL/dz tensors (last get_gradient) */
  const float* delta9x;   /* [160]-feature blocks: dL/dz9 | dz_density | dz_rgb | 0 */
  /* any-shape networks (generic != 0: every field above but M and zhead is NULL): row-major activations */
  int32_t generic;
  const float* gen_h;     /* net_depth consecutive [M][net_width] trunk activations */
  const float* gen_hc;    /* net_depth_condition consecutive [M][net_width_condition] (view layer first) */
} nof_mlp_debug;
nof_status nof_mlp_debug_view(nof_mlp* m, int32_t level, nof_mlp_debug* out);
/* Dispatch tally of the any-shape path (tests and tooling): how many launches of each kernel variant
 * (k_gemm / k_gemm_ws instantiations, the encoders, the slab and ray sums) this object has made since
 * its creation or the last clear.  counts[i] belongs to nof_gen_dispatch_name(i); *n = the number of
 * variants (min(cap, *n) counts are written), clear != 0 zeroes the tally after the read.  Host-side
 * counters only; a fused 8x256 network launches none of these kernels and reports all zeros.
 * nof_gen_dispatch_name: i outside [0, n) is NOF_ERR_INVALID_ARG (needs no device). */
nof_status nof_mlp_gen_dispatch(nof_mlp* m, int32_t clear, uint32_t* counts, int32_t cap, int32_t* n);
nof_status nof_gen_dispatch_name(int32_t i, const char** name);
/* The same pair for the fp16-product GEMMs of NOF_PRECISION_F16_PRODUCTS (k_gemm_h, a list of its own: one
 * name per instantiation and split / unsplit pick).  In that mode the tally above keeps counting the kernels
 * both modes share: the encoders, k_slab_sums, k_ray_sum and the one fp32 k_gemm per level (the view
 * encoding's weight gradient).  All zero in every other mode. */
nof_status nof_mlp_gen_dispatch_h(nof_mlp* m, int32_t clear, uint32_t* counts, int32_t cap, int32_t* n);
nof_status nof_gen_dispatch_h_name(int32_t i, const char** name);

/* ---- AcceleratedAdamOptimizer (AcceleratedAdamOptimizer.h:5-20) ------------------------------ */
/* ctor AcceleratedAdamOptimizer.cpp:6-21 (m, v zero-initialised: D18); cfg supplies device/stream */
nof_status nof_adam_create(const int32_t* layer_sizes, int32_t num_layers, const nof_config* cfg, nof_adam** out);
/* step AcceleratedAdamOptimizer.cpp:23-41: one fused launch when params/grads are views of flat arenas */
nof_status nof_adam_step(nof_adam* a, float* const* params, float* const* grads, float learning_rate);
nof_status nof_adam_iteration(nof_adam* a, int32_t* iteration);
nof_status nof_adam_destroy(nof_adam* a);
/* The training options the reference declares but never implements (Config.GradMaxNorm, Config.GradMaxVal,
 * TrainState.cs:58-59; Config.WeightDecayMult, TrainState.cs:70) and its statistics record (StatsUtil.cs:13,16-18,
 * which Program.LossFn fills with weightL2 = 0 alone, Program.cs:82-87), with mip-NeRF's meaning.  All in fp32,
 * element-wise over all P parameters (biases included), g = the gradient handed to nof_adam_step (data parallel:
 * the all-reduced one), p = the parameters before the update:
 *   g1 = g + ((2 weight_decay_mult) / P) p      (the loss term weight_decay_mult * sum p^2 / P; g when 0)
 *   g2 = clamp(g1, -grad_max_val, grad_max_val) (g1 when grad_max_val == 0)
 *   clip_scale = min(1, grad_max_norm / (1e-7 + |g2|))  (1 when grad_max_norm == 0);  Adam is fed g2 clip_scale
 * weight_l2 = sum p^2 / P, grad_norm = |g1|, grad_abs_max = max |g1|, grad_norm_clipped = clip_scale |g2|.  The
 * norms are global over all tensors and a pure function of the inputs (fixed summation order, no float atomics):
 * bit-identical run to run and replica to replica.  A step with any option set (stats != 0 gathers the record
 * alone) costs one launch more than the plain step, no host synchronisation and no allocation.  With every
 * option 0 (the default) the step is the plain one.  Options are hyper-parameters, not state: checkpoints do not
 * hold them.  Negative or NaN options are NOF_ERR_INVALID_ARG. */
typedef struct nof_step_stats {
  float weight_l2, grad_norm, grad_abs_max, grad_norm_clipped, clip_scale;
  int32_t iteration; /* the Adam step (nof_adam_iteration) the record belongs to */
} nof_step_stats;
nof_status nof_adam_set_options(nof_adam* a, float grad_max_norm, float grad_max_val, float weight_decay_mult,
                                int32_t stats);
nof_status nof_adam_get_options(nof_adam* a, float* grad_max_norm, float* grad_max_val, float* weight_decay_mult,
                                int32_t* stats);
/* Synchronises the optimizer's stream and returns the last step's record; NOF_ERR_INVALID_ARG when no step has
 * gathered statistics yet. */
nof_status nof_adam_stats(nof_adam* a, nof_step_stats* out);
/* The optimizer's moments (device memory, borrowed; *count floats each, in the order of the layer sizes): what a
 * checkpoint stores of it, for tests and tooling.  Work on the optimizer's stream may still be writing them. */
nof_status nof_adam_moments(nof_adam* a, float** m, float** v, int64_t* count);

/* ---- AcceleratedGradientCalculator (AcceleratedGradientCalculator.h:8-17) -------------------- */
nof_status nof_gradcalc_create(int32_t batch_size, const nof_config* cfg, nof_gradcalc** out);
/* get_output_gradient AcceleratedGradientCalculator.cpp:18-30: one output buffer per level (D15) */
nof_status nof_gradcalc_output_gradient(nof_gradcalc* g, uint64_t dev_comp_rgb, const float* host_pixels,
                                        int32_t n, uint64_t dev_loss_mults, float loss_mult_sum, int32_t level,
                                        uint64_t* out_dev_grad);
nof_status nof_gradcalc_destroy(nof_gradcalc* g);

/* ---- OutputRetriever::RetrieveOutput (OutputRetriever.cpp:6-14) ----------------------------- */
nof_status nof_retrieve_output(uint64_t dev_output, int32_t n, float* host_out /* [n][3] */);

/* ---- LearningRateDecay (MipHelpers.cs:758-773) ---------------------------------------------- */
float nof_lr_decay(int32_t step, float lr_init, float lr_final, int32_t max_steps, int32_t delay_steps,
                   float delay_mult);

/* ---- device memory / stream utilities (tooling and tests) ----------------------------------- */
nof_status nof_device_count(int32_t* count);
nof_status nof_set_device(int32_t device);
nof_status nof_malloc(void** ptr, size_t bytes);
nof_status nof_free(void* ptr);
nof_status nof_memcpy_h2d(void* dst, const void* src, size_t bytes);
nof_status nof_memcpy_d2h(void* dst, const void* src, size_t bytes);
nof_status nof_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
nof_status nof_memset(void* dst, int value, size_t bytes);
nof_status nof_stream_sync(void* stream);

/* ---- individual hot-path kernels (parity tests; all device pointers, async on `stream`) -----
 * get_sample_t_vals AF:222-242, get_resampled_t_vals AF:246-291, cast_rays AF:292-317,
 * encode_input_data AF:187-221, volumetric_rendering AF:318-344, volumetric_rendering_gradient
 * AF:362-402 (g = dL/dC given, or fused from pixels when dev_g == NULL). */
nof_status nof_kernel_sample_stratified(int32_t n, int32_t samples, const float* nears, const float* fars,
                                        int32_t randomized, uint64_t seed, uint32_t step, uint32_t level,
                                        uint32_t ray_base, float* t_out, void* stream);
/* ABI 2: the ray options as trailing arguments of _ex entry points (the round-4 signatures above are
 * unchanged, so a binding built against them keeps working): lindisp 1 = SampleAlongRay's disparity branch
 * (MipHelpers.cs:618-620); ray_shape NOF_RAY_CYLINDRICAL = CylinderToGaussian (MipHelpers.cs:403-409). */
nof_status nof_kernel_sample_stratified_ex(int32_t n, int32_t samples, const float* nears, const float* fars,
                                           int32_t randomized, uint64_t seed, uint32_t step, uint32_t level,
                                           uint32_t ray_base, float* t_out, void* stream, int32_t lindisp);
nof_status nof_kernel_sample_pdf(int32_t n, int32_t samples_in, const float* t_in, const float* weights,
                                 int32_t samples_out, float padding, int32_t randomized, uint64_t seed,
                                 uint32_t step, uint32_t level, uint32_t ray_base, float* t_out, int32_t* idx_out,
                                 void* stream);
nof_status nof_kernel_cast(int32_t n, int32_t samples, const float* t, const float* origins, const float* dirs,
                           const float* radii, float* means, float* covs, void* stream);
nof_status nof_kernel_cast_ex(int32_t n, int32_t samples, const float* t, const float* origins, const float* dirs,
                              const float* radii, float* means, float* covs, void* stream, int32_t ray_shape);
nof_status nof_kernel_encode(int32_t n, int32_t samples, const float* means, const float* covs, const float* dirs,
                             float* enc_pos, float* enc_dir, void* stream);
nof_status nof_kernel_render(int32_t n, int32_t samples, const float* density, const float* rgb, const float* t,
                             const float* dirs, int32_t white_bkgd, float* comp_rgb, float* weights, void* stream);
nof_status nof_kernel_render_grad(int32_t n, int32_t samples, const float* density, const float* rgb,
                                  const float* t, const float* dirs, int32_t white_bkgd, const float* comp_rgb,
                                  const float* dev_g, const float* pixels, const float* loss_mults,
                                  float loss_mult_sum, float lambda, float* density_grad, float* rgb_grad,
                                  void* stream);
/* The cross-level adjoints (nof_config.stop_level_grad = 0), for parity tests.
 * nof_kernel_render_grad_ex: nof_kernel_render_grad plus dev_w_grad ([n][S] or NULL: an extra dL/dw_k, folded into
 * e_k = g.c_k - G + q_k) and dev_t_grad ([n][S + 1] or NULL, overwritten: dL/dt through delta_k = t_{k+1} - t_k).
 * With both NULL it is nof_kernel_render_grad, bit for bit. */
nof_status nof_kernel_render_grad_ex(int32_t n, int32_t samples, const float* density, const float* rgb,
                                     const float* t, const float* dirs, int32_t white_bkgd, const float* comp_rgb,
                                     const float* dev_g, const float* pixels, const float* loss_mults,
                                     float loss_mult_sum, float lambda, float* density_grad, float* rgb_grad,
                                     const float* dev_w_grad, float* dev_t_grad, void* stream);
/* nof_kernel_render_grad_ex with the distortion loss (nof_config.distortion_loss_mult) of this level: nears / fars
 * [n] and lindisp give the normalised distance; dist_mult lossmult[r] / loss_mult_sum L_r is added to the objective
 * (loss_mults and loss_mult_sum are needed for it also when dev_g supplies dL/dC); dev_dist_rays ([n] or NULL)
 * receives that per-ray term.  dev_w_grad and dev_t_grad both NULL: k_render_bwd<., true>, else
 * k_render_bwd_x<., true> (the term's dL/dt added to dev_t_grad).  dist_mult = 0: the kernels without the term, so
 * nof_kernel_render_grad_ex bit for bit (dev_dist_rays zeroed). */
nof_status nof_kernel_render_grad_dist(int32_t n, int32_t samples, const float* density, const float* rgb,
                                       const float* t, const float* dirs, int32_t white_bkgd, const float* comp_rgb,
                                       const float* dev_g, const float* pixels, const float* loss_mults,
                                       float loss_mult_sum, float lambda, float* density_grad, float* rgb_grad,
                                       const float* dev_w_grad, float* dev_t_grad, const float* nears,
                                       const float* fars, int32_t lindisp, float dist_mult, float* dev_dist_rays,
                                       void* stream);
/* k_interlevel (nof_mipnerf_set_interlevel_loss): dev_w_grad [n][samples_prop] = d/dw_prop of
 * mult loss_mults[r] / loss_mult_sum L_r, the proposal (t_prop [n][samples_prop + 1], w_prop [n][samples_prop])
 * against the target (t_tgt [n][samples_tgt + 1], w_tgt [n][samples_tgt]); accumulate = 1 adds to dev_w_grad, 0
 * overwrites it; dev_rays ([n] or NULL) receives the per-ray term.  Both sample counts in {64, 128, 256, 512},
 * mult >= 0 (0: zeros), loss_mult_sum > 0; n = 0 launches nothing.  Every sum in a fixed order: the same bits
 * run to run. */
nof_status nof_kernel_interlevel(int32_t n, int32_t samples_prop, const float* t_prop, const float* w_prop,
                                 int32_t samples_tgt, const float* t_tgt, const float* w_tgt, const float* loss_mults,
                                 float loss_mult_sum, float mult, int32_t accumulate, float* dev_w_grad,
                                 float* dev_rays, void* stream);
/* The adjoint of nof_kernel_sample_pdf (the same sampling arguments; the forward's bin index, clamps, cdf
 * saturation, pad branch and blur-pool max picks are recomputed and held): dev_t_out_grad [n][S_out + 1] ->
 * dev_w_grad [n][S_in] and dev_t_in_grad [n][S_in + 1] (or NULL: not wanted), both overwritten. */
nof_status nof_kernel_sample_pdf_grad(int32_t n, int32_t samples_in, const float* t_in, const float* weights,
                                      int32_t samples_out, float padding, int32_t randomized, uint64_t seed,
                                      uint32_t step, uint32_t level, uint32_t ray_base, const float* dev_t_out_grad,
                                      float* dev_w_grad, float* dev_t_in_grad, void* stream);
/* The adjoint of cast + IPE with respect to t: dev_enc_pos / dev_enc_pos_grad [n S][6 (max_deg - min_deg)] in the
 * any-shape encoder's feature order (the stored forward encoding and dL/d of it) -> dev_t_grad [n][S + 1],
 * overwritten.  S a multiple of 64; 16-byte aligned encodings. */
nof_status nof_kernel_encode_grad(int32_t n, int32_t samples, const float* t, const float* origins,
                                  const float* dirs, const float* radii, int32_t ray_shape, int32_t min_deg,
                                  int32_t max_deg, const float* dev_enc_pos, const float* dev_enc_pos_grad,
                                  float* dev_t_grad, void* stream);
/* One level's share of the ray gradients (k_ray_grad, for parity tests): encodings as nof_kernel_encode_grad;
 * sigma / sigma_grad [n S] (the integrator's |d|: alpha = 1 - exp(-sigma delta |d|)); dev_enc_dir /
 * dev_enc_dir_grad [n][3 + 6 deg_view] (enc_dir_grad NULL: no view term) -> dev_o_grad, dev_d_grad [n][3],
 * overwritten, or added to when accumulate.  S a multiple of 32, at most 512. */
nof_status nof_kernel_ray_grad(int32_t n, int32_t samples, const float* t, const float* origins, const float* dirs,
                               const float* radii, int32_t ray_shape, int32_t min_deg, int32_t max_deg,
                               const float* dev_enc_pos, const float* dev_enc_pos_grad, const float* sigma,
                               const float* sigma_grad, int32_t deg_view, const float* dev_enc_dir,
                               const float* dev_enc_dir_grad, int32_t accumulate, float* dev_o_grad,
                               float* dev_d_grad, void* stream);
/* The scene contraction (nof_mipnerf_set_contraction) at the kernel entry points, for parity tests: the argument
 * lists above plus a trailing contraction mode.  NOF_CONTRACT_SPHERE: nof_kernel_cast_contract stores the contracted
 * Gaussians (k_cast_contract), and the two adjoints take dev_enc_pos as the encoding of the contracted Gaussians and
 * apply the map's adjoint at the uncontracted ones.  NOF_CONTRACT_NONE: each is the entry point it extends, bit for
 * bit. */
nof_status nof_kernel_cast_contract(int32_t n, int32_t samples, const float* t, const float* origins,
                                    const float* dirs, const float* radii, float* means, float* covs, void* stream,
                                    int32_t ray_shape, int32_t contraction);
nof_status nof_kernel_encode_grad_ex(int32_t n, int32_t samples, const float* t, const float* origins,
                                     const float* dirs, const float* radii, int32_t ray_shape, int32_t min_deg,
                                     int32_t max_deg, const float* dev_enc_pos, const float* dev_enc_pos_grad,
                                     float* dev_t_grad, void* stream, int32_t contraction);
nof_status nof_kernel_ray_grad_ex(int32_t n, int32_t samples, const float* t, const float* origins, const float* dirs,
                                  const float* radii, int32_t ray_shape, int32_t min_deg, int32_t max_deg,
                                  const float* dev_enc_pos, const float* dev_enc_pos_grad, const float* sigma,
                                  const float* sigma_grad, int32_t deg_view, const float* dev_enc_dir,
                                  const float* dev_enc_dir_grad, int32_t accumulate, float* dev_o_grad,
                                  float* dev_d_grad, void* stream, int32_t contraction);
nof_status nof_kernel_adam(int64_t n, float* params, const float* grads, float* m, float* v, float lr,
                           int32_t iteration, void* stream);

/* One product of NOF_PRECISION_F16_PRODUCTS (k_gemm_h), for parity tests:
 *   C[z slab_stride + i ci + j cj] = epilogue(inv_s sum_k f16(s X(i, k)) f16(Y(j, k))),  i < M, j < N,
 * k over chunk z = [z kchunk, min((z + 1) kchunk, K1 + K2)), z < ksplit.  Element (i, k) of an operand is
 * src1.p[(i / idiv) si + k sk] for k < K1, else src2.p[(i / idiv) si + (k - K1) sk] (idiv 0 reads as 1; K2 = 0: no
 * second source).  Epilogue: + bias[j], ReLU, then 0 where !(G[i gi + j gj] > 0), each optional (NULL / 0).
 * s = 2^(8 - floor(log2 amax)) with amax = the float whose bits *scale_amax holds (1 when NULL or scale_src = 0),
 * applied to X = A (scale_src 1) or B (2), inv_s its inverse.  rowsum (optional) [z M + i] = inv_s sum_k
 * f16(s A(i, k)).  ksplit > 1 takes K2 = 0 and G = NULL.  The caller owns every bound: all pointers are device
 * memory covering the indices above. */
typedef struct nof_gemm_src {
  const float* p;
  int64_t si, sk;
  int32_t idiv;
} nof_gemm_src;
typedef struct nof_gemm_args {
  int32_t M, N, K1, K2;
  nof_gemm_src A1, A2, B1, B2;
  const float* bias;
  int32_t relu;
  const float* G;
  int64_t gi, gj;
  float* C;
  int64_t ci, cj;
  int32_t kchunk;
  int64_t slab_stride;
  float* rowsum;
  const uint32_t* scale_amax;
  int32_t scale_src;
  int32_t ksplit;
} nof_gemm_args;
nof_status nof_kernel_gemm_h(const nof_gemm_args* args, void* stream);
/* The appearance embeddings' two kernels (appearance.hip), for parity tests.  gather: out [n][vd + dim]
 * = [enc_dir [n][vd] row | table [views][dim] row ids[r]]; ids == NULL: row const_view for every ray; an id outside
 * [0, views): zeros.  grad: d_table [views][dim] = per view, the sum of the rows of d_app [n][dim] whose id is that
 * view, in a fixed order; accumulate = 0 overwrites (a view without a ray: exactly 0), 1 adds (such a view: left
 * bitwise as it is).  dim in [1, 256]. */
nof_status nof_kernel_appearance_gather(int32_t n, int32_t vd, int32_t dim, int32_t views, const float* enc_dir,
                                        const float* table, const int32_t* ids, int32_t const_view, float* out,
                                        void* stream);
nof_status nof_kernel_appearance_grad(int32_t n, int32_t dim, int32_t views, const int32_t* ids, const float* d_app,
                                      float* d_table, int32_t accumulate, void* stream);

/* ---- per-kernel timing (hipEvents on the object's stream) ----------------------------------- */
#define NOF_NUM_TIMERS 8
/* timer ids: 0 pack, 1 sample, 2 mlp_fwd, 3 render_fwd, 4 render_bwd, 5 mlp_bwd, 6 wgrad, 7 wgrad_reduce */
nof_status nof_mipnerf_enable_timing(nof_mipnerf* h, int32_t enable);
/* only the timers whose bit is set in mask (bit i = timer id i); 0 disables.  Each timed launch is
 * bracketed by two hipEventRecords on the stream, which cost the launch sequence a few us each */
nof_status nof_mipnerf_enable_timing_mask(nof_mipnerf* h, uint32_t mask);
/* synchronises; returns summed milliseconds and launch counts per timer id since the last read */
nof_status nof_mipnerf_read_timing(nof_mipnerf* h, float* ms, int32_t* launches, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* NOF_H */
