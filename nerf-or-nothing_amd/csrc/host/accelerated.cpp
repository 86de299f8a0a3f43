// Host implementation of the AcceleratedNeRFUtils classes for MI355X (see accelerated.h).
#include "accelerated.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../kernels/common.h"
#include "../kernels/mlp_common.h"
#include "../kernels/mlp_h32.h"
#include "trace.h"

namespace AcceleratedNeRFUtils {

using nof::kBlk;

// ------------------------------------------------------------------------------------------------
// KernelTimer
// ------------------------------------------------------------------------------------------------
void KernelTimer::enable(uint32_t mask, hipStream_t st) {
  mask_ = mask;
  st_ = st;
  used_ = 0;
  recs_.clear();
  for (int i = 0; i < NOF_NUM_TIMERS; ++i) { tot_ms_[i] = 0.0f; tot_n_[i] = 0; }
}
void KernelTimer::fold() {
  if (!recs_.empty()) NOF_HIP(hipEventSynchronize(recs_.back().b));
  for (const Rec& r : recs_) {
    float t = 0.0f;
    NOF_HIP(hipEventElapsedTime(&t, r.a, r.b));
    if (r.id < NOF_NUM_TIMERS) { tot_ms_[r.id] += t; tot_n_[r.id] += 1; }
  }
  recs_.clear();
  used_ = 0;
}
hipEvent_t KernelTimer::get() {
  if (used_ == pool_.size()) {
    hipEvent_t e;
    NOF_HIP(hipEventCreate(&e));
    pool_.push_back(e);
  }
  return pool_[used_++];
}
void KernelTimer::begin(int id) {
  roctxRangePushA(timer_range_name(id));  // every bracketed launch is also a roctx range
  if (!((mask_ >> id) & 1u)) return;
  if (recs_.size() >= kMaxRecs) {  // bounded pool: fold what is finished (no record is open here)
    bool open = false;
    for (hipEvent_t e : open_) open = open || e != nullptr;
    if (!open) fold();
  }
  open_[id] = get();
  NOF_HIP(hipEventRecord(open_[id], st_));
}
void KernelTimer::end(int id) {
  roctxRangePop();
  if (!((mask_ >> id) & 1u) || !open_[id]) return;
  hipEvent_t b = get();
  NOF_HIP(hipEventRecord(b, st_));
  recs_.push_back({id, open_[id], b});
  open_[id] = nullptr;
}
void KernelTimer::read(float* ms, int* launches, int cap) {
  fold();
  for (int i = 0; i < cap; ++i) {
    ms[i] = i < NOF_NUM_TIMERS ? tot_ms_[i] : 0.0f;
    launches[i] = i < NOF_NUM_TIMERS ? tot_n_[i] : 0;
  }
  for (int i = 0; i < NOF_NUM_TIMERS; ++i) { tot_ms_[i] = 0.0f; tot_n_[i] = 0; }
}
KernelTimer::~KernelTimer() {
  for (hipEvent_t e : pool_) (void)hipEventDestroy(e);
}

// ------------------------------------------------------------------------------------------------
// Philox-based Glorot init (MLPcs:78-85 C# semantics, D6): W = sqrt(6/(in+out)) * (2u - 1), b = 0.
// ------------------------------------------------------------------------------------------------
static void glorot_host(float* P, const int* out, const int* in, const int* woff, int L, uint64_t seed) {
#pragma clang fp contract(off)
  for (int l = 0; l < L; ++l) {
    const float g = std::sqrt(6.0f / (float)(in[l] + out[l]));
    const size_t cnt = (size_t)out[l] * in[l];
    for (size_t e = 0; e < cnt; ++e) {
      const float u = nof::philox_uniform(seed, 0, (uint32_t)l, nof::kStreamInit, (uint32_t)(e >> 32), (uint32_t)e);
      P[woff[l] + e] = g * (u * 2.0f - 1.0f);
    }
  }
}

static void check_cfg(const nof_config& c) {
  NOF_REQUIRE(c.max_rays > 0, "max_rays must be > 0");
  NOF_REQUIRE(c.num_levels >= 1 && c.num_levels <= NOF_MAX_LEVELS, "num_levels out of range");
  for (int l = 0; l < c.num_levels; ++l) {
    const int S = c.num_samples[l];
    if (!(S == 64 || S == 128 || S == 256 || S == 512))
      throw Error(NOF_ERR_UNSUPPORTED, "GPU path supports 64/128/256/512 samples per level");
  }
  // the network (MLP.cs:64-86): any depth / width / skip / PE degrees within the checkpoint's 16 layers
  NOF_REQUIRE(c.net_depth >= 1 && c.net_depth_condition >= 1 &&
                  c.net_depth + c.net_depth_condition + 2 <= AcceleratedMLP::kMaxLayers,
              "net_depth >= 1, net_depth_condition >= 1, net_depth + net_depth_condition <= 14");
  NOF_REQUIRE(c.net_width >= 1 && c.net_width <= 4096 && c.net_width_condition >= 1 && c.net_width_condition <= 4096,
              "network widths must be in [1, 4096]");
  NOF_REQUIRE(c.skip_layer >= 1, "skip_layer must be >= 1");
  NOF_REQUIRE(c.min_deg_point >= 0 && c.max_deg_point > c.min_deg_point && c.max_deg_point <= 24,
              "point PE degrees: 0 <= min_deg_point < max_deg_point <= 24");
  NOF_REQUIRE(c.deg_view >= 0 && c.deg_view <= 24, "deg_view must be in [0, 24]");
  NOF_REQUIRE(c.precision == NOF_PRECISION_F32 || c.precision == NOF_PRECISION_F32_SPLIT ||
                  c.precision == NOF_PRECISION_F16X2 || c.precision == NOF_PRECISION_F32_F16SPLIT ||
                  c.precision == NOF_PRECISION_F16 || c.precision == NOF_PRECISION_F16_PRODUCTS,
              "unknown precision mode");
  const bool reference_net = c.net_depth == 8 && c.net_width == 256 && c.net_depth_condition == 1 &&
                             c.net_width_condition == 128 && c.skip_layer == 4 && c.min_deg_point == 0 &&
                             c.max_deg_point == 16 && c.deg_view == 4;
  if (!reference_net && c.precision != NOF_PRECISION_F32 && c.precision != NOF_PRECISION_F16_PRODUCTS)
    throw Error(NOF_ERR_UNSUPPORTED,
                "networks other than the reference's 8x256 / 1x128 / skip 4 / PE 16, 4 run in NOF_PRECISION_F32 "
                "or NOF_PRECISION_F16_PRODUCTS only (the any-shape path, generic.hip / gemm_h.hip)");
  NOF_REQUIRE(c.grad_buckets == 0 || c.grad_buckets == 1, "grad_buckets must be 0 or 1");
  NOF_REQUIRE(c.lindisp == 0 || c.lindisp == 1, "lindisp must be 0 or 1");
  NOF_REQUIRE(c.ray_shape == NOF_RAY_CONICAL || c.ray_shape == NOF_RAY_CYLINDRICAL, "unknown ray_shape");
  NOF_REQUIRE(std::isfinite(c.density_bias) && std::isfinite(c.rgb_padding) && c.rgb_padding >= 0.0f &&
                  c.rgb_padding < 0.5f,
              "density_bias must be finite, rgb_padding in [0, 0.5)");
  NOF_REQUIRE(c.stop_level_grad == 0 || c.stop_level_grad == 1, "stop_level_grad must be 0 or 1");
  NOF_REQUIRE(std::isfinite(c.distortion_loss_mult) && c.distortion_loss_mult >= 0.0f,
              "distortion_loss_mult must be finite and >= 0");
  if (c.stop_level_grad == 0 && c.precision != NOF_PRECISION_F32 && c.precision != NOF_PRECISION_F16_PRODUCTS)
    throw Error(NOF_ERR_UNSUPPORTED,
                "stop_level_grad = 0 needs the gradient with respect to the MLP's encoded input, which the fused "
                "8x256 kernels do not produce: use NOF_PRECISION_F32 or NOF_PRECISION_F16_PRODUCTS (the any-shape "
                "path, every network)");
}

// the network is not the reference's, or the mode / option is one only the any-shape path has
static bool any_shape(const nof_config& c) {
  return !(c.net_depth == 8 && c.net_width == 256 && c.net_depth_condition == 1 && c.net_width_condition == 128 &&
           c.skip_layer == 4 && c.min_deg_point == 0 && c.max_deg_point == 16 && c.deg_view == 4) ||
         c.precision == NOF_PRECISION_F16_PRODUCTS || c.stop_level_grad == 0;
}

void check_model(const nof_config& c, int app_views, int app_dim) {
  check_cfg(c);
  NOF_REQUIRE(app_dim >= 0 && app_dim <= 256, "appearance_dim must be in [0, 256]");
  if (app_dim == 0) return;
  NOF_REQUIRE(app_views > 0, "appearance_dim > 0 needs appearance_views > 0");
  NOF_REQUIRE((int64_t)app_views * app_dim < ((int64_t)1 << 31), "appearance table too large (views * dim >= 2^31)");
  if (!any_shape(c))
    throw Error(NOF_ERR_UNSUPPORTED,
                "appearance embeddings need the any-shape path: the fused 8x256 kernels have no per-ray operand "
                "beyond the view encoding (use NOF_PRECISION_F16_PRODUCTS, or NOF_PRECISION_F32 with "
                "stop_level_grad = 0)");
}

// ------------------------------------------------------------------------------------------------
// AcceleratedMLP
// ------------------------------------------------------------------------------------------------
AcceleratedMLP::AcceleratedMLP(int deg_point, int deg_view, const nof_config& cfg, int app_views, int app_dim)
    : cfg_(cfg) {
  check_model(cfg, app_views, app_dim);
  if (app_dim > 0) { gV_ = app_views; gG_ = app_dim; }
  NOF_REQUIRE(deg_point == cfg.max_deg_point - cfg.min_deg_point && deg_view == cfg.deg_view,
              "AcceleratedMLP(deg_point, deg_view) must match the config");
  NOF_HIP(hipSetDevice(cfg.device));
  st_ = (hipStream_t)cfg.stream;
  hipDeviceProp_t prop;
  NOF_HIP(hipGetDeviceProperties(&prop, cfg.device));
  num_cu_ = prop.multiProcessorCount;
  aligned_ = cfg.grad_buckets != 0;

  // layer dims (get_layer_sizes MLPcpp:131-154, generalised as MLP.cs:64-86): trunk 0..D-1 (the IPE
  // concatenated into every skip-th layer after the first), density D, view D+1 ([h | view PE], with appearance
  // embeddings [h | view PE | E[view]]),
  // condition layers D+2..D+Dc, rgb D+Dc+1
  const int D = cfg.net_depth, W = cfg.net_width, Dc = cfg.net_depth_condition, Wc = cfg.net_width_condition;
  const int pos = 6 * (cfg.max_deg_point - cfg.min_deg_point), dir = 3 * (2 * cfg.deg_view + 1);
  const int L = D + Dc + 2;
  out_.resize(L); in_.resize(L); woff_.resize(L); boff_.resize(L);
  for (int l = 0; l < D; ++l) { out_[l] = W; in_[l] = l == 0 ? pos : (l % cfg.skip_layer == 0 ? W + pos : W); }
  out_[D] = 1; in_[D] = W;
  out_[D + 1] = Wc; in_[D + 1] = W + dir + gG_;
  for (int i = 1; i < Dc; ++i) { out_[D + 1 + i] = Wc; in_[D + 1 + i] = Wc; }
  out_[D + 1 + Dc] = 3; in_[D + 1 + Dc] = Wc;
  size_t o = 0;
  for (int l = 0; l < L; ++l) { woff_[l] = (int)o; o += (size_t)out_[l] * in_[l]; }
  for (int l = 0; l < L; ++l) { boff_[l] = (int)o; o += out_[l]; }
  NOF_REQUIRE(o < (size_t)1 << 31, "network too large");
  P_ = o;
  // (F16_PRODUCTS is the any-shape path's mode: the reference network runs there too)
  generic_ = any_shape(cfg);
  cross_ = cfg.stop_level_grad == 0 && cfg.num_levels > 1;  // (one level: nothing crosses)

  params_.alloc(P_);
  grads_.alloc(P_);
  NOF_HIP(hipMemset(grads_.p, 0, P_ * sizeof(float)));
  std::vector<float> h(P_, 0.0f);
  glorot_host(h.data(), out_.data(), in_.data(), woff_.data(), L, cfg.seed);
  NOF_HIP(hipMemcpy(params_.p, h.data(), P_ * sizeof(float), hipMemcpyHostToDevice));
  for (int l = 0; l < L; ++l) { param_views_.push_back(params_.p + woff_[l]); grad_views_.push_back(grads_.p + woff_[l]); }
  for (int l = 0; l < L; ++l) { param_views_.push_back(params_.p + boff_[l]); grad_views_.push_back(grads_.p + boff_[l]); }

  precision_ = cfg.precision;
  numeric_.alloc(2);
  NOF_HIP(hipMemset(numeric_.p, 0, 2 * sizeof(uint32_t)));
  if (generic_) {
    gD_ = D; gW_ = W; gDc_ = Dc; gWc_ = Wc; gskip_ = cfg.skip_layer; gmin_deg_ = cfg.min_deg_point;
    gP_ = pos; gVd_ = dir;
    gen_alloc();
    return;
  }
  if (precision_ == NOF_PRECISION_F32_SPLIT) {  // bf16 (hi, mid, lo) slices + the fp32 tails (mlp_common.h)
    wimg_f_.alloc(nof::fwd_image_split_floats<1>() + nof::kFwdTail);
    wimg_b_.alloc(nof::bwd_image_split_floats<1>() + nof::kBwdTail);
  } else if (precision_ == NOF_PRECISION_F16) {  // fp16 k-step fragment streams + the fp32 tails (mlp_h32.h)
    wimg_f_.alloc(nof::kFwdH32Floats + nof::kFwdTail);
    wimg_b_.alloc(nof::kBwdH32Floats + nof::kBwdTail);
    amax_.alloc(cfg.num_levels);
  } else if (f16_pieces()) {  // f16 (hi, lo) slices + the fp32 tails
    wimg_f_.alloc(nof::fwd_image_split_floats<2>() + nof::kFwdTail);
    wimg_b_.alloc(nof::bwd_image_split_floats<2>() + nof::kBwdTail);
    amax_.alloc(cfg.num_levels);
  } else {
    wimg_f_.alloc(nof::kFwdImageFloats);
    wimg_b_.alloc(nof::kBwdImageFloats);
  }

  lv_.resize(cfg.num_levels);
  for (int l = 0; l < cfg.num_levels; ++l) {
    Level& L = lv_[l];
    L.cap = cfg.max_rays * cfg.num_samples[l];
    const size_t nb = (size_t)L.cap / kBlk;
    L.act_in.alloc(nb * nof::kInF * kBlk);
    L.act_h.alloc(8 * nb * 256 * kBlk);
    L.act_h9.alloc(nb * 128 * kBlk);
    L.masks.alloc(nb * nof::kMaskSlots * 256);
    L.zhead.alloc((size_t)L.cap * 4);
    L.sigma.alloc(L.cap);
    L.rgb.alloc((size_t)L.cap * 3);
    L.delta.alloc(8 * nb * 256 * kBlk);
    L.delta9x.alloc(nb * nof::kD9F * kBlk);
    NOF_HIP(hipMemset(L.delta9x.p, 0, L.delta9x.n * sizeof(float)));  // rows 132..159 stay zero
    max_M_ = std::max(max_M_, L.cap);
  }
  view_pe_.alloc((size_t)cfg.max_rays * 32);
  view_bias_.alloc((size_t)cfg.max_rays * 128);
  slab_cap_ = (size_t)(num_cu_ + 64) * 65536;
  slabs_.alloc(slab_cap_);
  bias_slabs_.alloc((size_t)(num_cu_ + 64) * 256);
}

std::vector<int> AcceleratedMLP::get_layer_sizes() const {
  const int L = num_layers();
  std::vector<int> s(2 * L);
  for (int l = 0; l < L; ++l) { s[l] = out_[l] * in_[l]; s[L + l] = out_[l]; }
  return s;
}

bool AcceleratedMLP::pack_weights(const nof::StratArgs* strat, const float* view_dirs, int view_n) {
  view_dirs_ = nullptr;  // the tables of an earlier step are stale: the weights may have moved
  view_n_ = 0;
  if (generic_) {  // the any-shape path reads the canonical arena directly
    if (f16_products()) {  // the step's delta-scale maxima start at 0
      NOF_HIP(hipMemsetAsync(amax_.p, 0, lv_.size() * sizeof(uint32_t), st_));
      amax_cleared_ = (1u << lv_.size()) - 1u;
      amax_given_ = 0u;
    }
    return false;
  }
  nof::PackArgs pa;
  if (strat) pa.strat = *strat;
  for (int l = 0; l < kLayers; ++l) { pa.woff[l] = woff_[l]; pa.boff[l] = boff_[l]; }
  if (f16_pieces()) {  // the step's delta-scale maxima start at 0 (no memset launch per level)
    pa.zero = amax_.p;
    pa.nzero = (int)lv_.size();
    amax_cleared_ = (1u << lv_.size()) - 1u;
    amax_given_ = 0u;
  }
  // the step's per-ray view tables, for the k_mlp_fwd16 modes (the split and F16 forwards have their own prologues)
  const bool fwd16 = precision_ == NOF_PRECISION_F32 || precision_ == NOF_PRECISION_F16X2 ||
                     precision_ == NOF_PRECISION_F32_F16SPLIT;
  if (view_dirs && view_n > 0 && view_n <= cfg_.max_rays && fwd16 && (step_fusion_ & NOF_STEP_FUSION_VIEW_TABLES)) {
    pa.view.n = view_n; pa.view.dirs = view_dirs; pa.view.pe = view_pe_.p; pa.view.bias = view_bias_.p;
    view_dirs_ = view_dirs;
    view_n_ = view_n;
  }
  tb(kTPack);
  if (precision_ == NOF_PRECISION_F16)
    NOF_HIP(nof::launch_pack_weights_h32(params_.p, pa, wimg_f_.p, wimg_b_.p, st_));
  else if (precision_ != NOF_PRECISION_F32)
    NOF_HIP(nof::launch_pack_weights_x3(params_.p, pa, wimg_f_.p, wimg_b_.p, f16_pieces() ? 2 : 1, st_));
  else NOF_HIP(nof::launch_pack_weights(params_.p, pa, wimg_f_.p, wimg_b_.p, st_));
  te(kTPack);
  return strat != nullptr;
}

uint32_t* AcceleratedMLP::claim_delta_amax(int level) {
  if (!(f16_pieces() || f16_products()) || level < 0 || level >= (int)lv_.size() || !((amax_cleared_ >> level) & 1u)) return nullptr;
  amax_cleared_ &= ~(1u << level);
  amax_given_ |= 1u << level;
  return amax_.p + level;
}

void AcceleratedMLP::run_forward(int level, const nof::FwdArgs& a0) {
  Level& L = lv_[level];
  nof::FwdArgs a = a0;
  a.split = precision_;
  a.dbias = cfg_.density_bias;  // MipNerfModel.DensityBias / RgbPadding (MNcs:20-22)
  a.rgb_pad = cfg_.rgb_padding;
  a.rgb_scale = rgb_scale();
  a.wimg = wimg_f_.p;
  a.act_in = L.act_in.p;
  a.act_h = L.act_h.p;
  a.act_h9 = L.act_h9.p;
  a.masks = L.masks.p;
  a.zhead = L.zhead.p;
  a.sigma = L.sigma.p;
  a.rgb = L.rgb.p;
  tb(kTMlpFwd);
  NOF_HIP(nof::launch_mlp_fwd(a, st_));
  te(kTMlpFwd);
}

void AcceleratedMLP::forward_fused(int level, int n, int samples, const float* t, const float* origins,
                                   const float* dirs, const float* radii, bool inference) {
  NOF_REQUIRE(level >= 0 && level < (int)lv_.size(), "level out of range");
  const int M = n * samples;
  NOF_REQUIRE(n > 0 && samples % kBlk == 0 && M <= lv_[level].cap, "batch exceeds the level's capacity");
  lv_[level].M = M; lv_[level].n = n; lv_[level].S = samples;
  if (generic_) {  // cast + encode, then the layer GEMMs
    // (per-ray buffers — the view encodings, the ray sums of the view-layer gradient — hold max_rays rays)
    NOF_REQUIRE(n <= cfg_.max_rays, "n_rays exceeds max_rays");
    GenLevel& G = gl_[level];
    tb(kTMlpFwd);
    NOF_HIP(nof::launch_cast(n, samples, t, origins, dirs, radii, G.mean.p, G.cov.p, st_, cfg_.ray_shape,
                             contraction_));
    int v;
    NOF_HIP(nof::launch_encode_g(n, samples, G.mean.p, G.cov.p, dirs, gmin_deg_, gP_, gVd_, G.enc_pos.p, G.enc_dir.p,
                                 st_, &v));
    tally(v);
    if (gG_) appearance_gather(level, n);
    te(kTMlpFwd);
    gen_forward(level, G.enc_pos.p, G.enc_dir.p);
    return;
  }
  nof::FwdArgs a{};
  a.M = M; a.S = samples; a.encoded = 0;
  a.no_store = inference ? 1 : 0;
  a.cylinder = cfg_.ray_shape == NOF_RAY_CYLINDRICAL ? 1 : 0;
  a.t = t; a.origins = origins; a.dirs = dirs; a.radii = radii;
  if (view_dirs_ && view_dirs_ == dirs && n <= view_n_) {  // this step's pack launch tabulated these rays
    a.view_pe = view_pe_.p;
    a.view_bias = view_bias_.p;
  }
  run_forward(level, a);
}

std::pair<float*, float*> AcceleratedMLP::get_output(const float* enc_pos, const float* enc_dir, int level,
                                                     int n_rays, int samples) {
  NOF_REQUIRE(level >= 0 && level < (int)lv_.size(), "level out of range");
  NOF_REQUIRE(enc_pos && enc_dir, "null encoded inputs");
  const int M = n_rays * samples;
  NOF_REQUIRE(n_rays > 0 && samples > 0 && samples % kBlk == 0 && M <= lv_[level].cap,
              "n_rays * samples must be a multiple of 32 within the level's capacity");
  pack_weights();
  lv_[level].M = M; lv_[level].n = n_rays; lv_[level].S = samples;
  if (generic_) {  // the encodings copied in: the backward reads them after the caller's buffers may be gone
    NOF_REQUIRE(n_rays <= cfg_.max_rays, "n_rays exceeds max_rays");  // enc_dir / the ray sums: max_rays rays
    GenLevel& G = gl_[level];
    NOF_HIP(hipMemcpyAsync(G.enc_pos.p, enc_pos, (size_t)M * gP_ * sizeof(float), hipMemcpyDeviceToDevice, st_));
    NOF_HIP(hipMemcpyAsync(G.enc_dir.p, enc_dir, (size_t)n_rays * gVd_ * sizeof(float), hipMemcpyDeviceToDevice,
                           st_));
    if (gG_) appearance_gather(level, n_rays);  // (no per-ray ids on this entry: the constant render view)
    gen_forward(level, G.enc_pos.p, G.enc_dir.p);
    return {lv_[level].sigma.p, lv_[level].rgb.p};
  }
  nof::FwdArgs a{};
  a.M = M; a.S = samples; a.encoded = 1;
  a.enc_pos = enc_pos; a.enc_dir = enc_dir;
  run_forward(level, a);
  return {lv_[level].sigma.p, lv_[level].rgb.p};
}

nof_mlp_debug AcceleratedMLP::debug_view(int level) const {
  NOF_REQUIRE(level >= 0 && level < (int)lv_.size(), "level out of range");
  const Level& L = lv_[level];
  nof_mlp_debug d{};
  d.M = L.M;
  if (generic_) {
    const GenLevel& G = gl_[level];
    d.generic = 1;
    d.gen_h = G.h.p; d.gen_hc = G.hc.p; d.zhead = G.z.p;
    return d;
  }
  d.act_in = L.act_in.p; d.act_h = L.act_h.p; d.act_h9 = L.act_h9.p; d.masks = L.masks.p; d.zhead = L.zhead.p;
  d.delta = L.delta.p; d.delta9x = L.delta9x.p;
  return d;
}

int grad_bucket_spans(const int* sizes, int num_layers, int b, int64_t* off, int64_t* cnt) {
  // arena [W0..W(L-1), b0..b(L-1)] (MLPcpp:131-154); bucket 0 = W5..W(L-1) (empty for L <= 5), bucket 1 =
  // the rest
  NOF_REQUIRE(sizes && num_layers >= 1 && b >= 0 && b < AcceleratedMLP::kBuckets, "bad bucket query");
  int64_t w5 = 0, wend = 0, total = 0;
  for (int l = 0; l < num_layers; ++l) {
    if (l < 5) w5 += sizes[l];
    wend += sizes[l];
    total += sizes[l] + sizes[num_layers + l];
  }
  if (b == 0) {
    off[0] = w5; cnt[0] = wend - w5;
    return 1;
  }
  off[0] = 0; cnt[0] = w5;
  off[1] = wend; cnt[1] = total - wend;
  return 2;
}

int AcceleratedMLP::bucket_spans(int b, int64_t* off, int64_t* cnt) const {
  const std::vector<int> s = get_layer_sizes();
  return grad_bucket_spans(s.data(), num_layers(), b, off, cnt);
}

AcceleratedMLP::Schedule& AcceleratedMLP::schedule(int lv0, int lv1, int bucket) {
  NOF_REQUIRE(lv0 >= 0 && lv0 < lv1 && lv1 <= (int)lv_.size(), "bad level range");
  std::vector<int64_t> key{lv0, lv1, bucket, aligned_ ? 1 : 0};
  for (int l = lv0; l < lv1; ++l) key.push_back(lv_[l].M);
  auto it = sched_.find(key);
  if (it != sched_.end()) return it->second;
  const int nlev = lv1 - lv0;
  std::vector<nof::WgProblem> P;
  std::vector<int> pbucket;  // bucket of each problem's outputs: layers 5..10 -> 0, 0..4 -> 1
  std::vector<int> pnblk;    // k-blocks of each problem (its level's M / 32)
  struct OutSpec { int prob, row_off, nrows, col_off, ncols; float* dst; int ld, dst_col; float* bias; };
  std::vector<OutSpec> os;
  float* G = grads_.p;
  // operand blocks hold fp16 in the f16 modes (mlp_common.h ActOut): element offsets in halves there
  const bool half = f16_blocks();
  auto at = [&](float* base, size_t off) -> const float* {
    return half ? reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(base) + off) : base + off;
  };
  auto Wg = [&](int l) { return G + woff_[l]; };
  auto Bg = [&](int l) { return G + boff_[l]; };
  // F16 (k_wgrad_s): the problems that share an A operand are one problem with more output columns —
  // delta_4 x [h3 | IPE] and delta_9x x [h7 | view PE | h9] — so each delta block is read once
  const bool merge = precision_ == NOF_PRECISION_F16;
  // The per-level problem list is the same for every level; problem q of level lev goes to index
  // q nlev + (lev - lv0), so a problem's items over all levels are contiguous (level order) and one
  // output spec (WgOut) reduces them all.
  for (int lev = lv0; lev < lv1; ++lev) {
    Level& L = lv_[lev];
    const int nblk = L.M / kBlk;
    const size_t ls = (size_t)nblk * 256 * kBlk;
    std::vector<nof::WgProblem> Pl;
    std::vector<int> bl;
    std::vector<OutSpec> ol;
    auto prob = [&](int layer, const float* A, int FA, int a0, int ntr, const float* B, int FB, int b0, int ntc) {
      nof::WgProblem q{};
      q.A = A; q.FA = FA; q.a_row0 = a0; q.ntr = ntr; q.B = B; q.FB = FB; q.b_col0 = b0; q.ntc = ntc; q.shape = 0;
      q.ntc1 = ntc;
      q.level = lev;
      Pl.push_back(q);
      bl.push_back(layer >= 5 ? 0 : 1);
      return (int)Pl.size() - 1;
    };
    auto extra_b = [&](int p, const float* B, int FB, int b0, int ntc) {
      nof::WgProblem& q = Pl[p];
      if (q.ntc2 == 0) { q.B2 = B; q.FB2 = FB; q.b2_col0 = b0; q.ntc2 = ntc; }
      else { q.B3 = B; q.FB3 = FB; q.b3_col0 = b0; q.ntc3 = ntc; }
      q.ntc += ntc;
    };
    float* dl = L.delta.p;
    float* d9 = L.delta9x.p;
    int p;
    p = prob(0, dl, 256, 0, 8, L.act_in.p, nof::kInF, 0, 3);
    ol.push_back({p, 0, 256, 0, 96, Wg(0), 96, 0, Bg(0)});
    for (int l = 1; l < 8; ++l) {
      p = prob(l, at(dl, l * ls), 256, 0, 8, at(L.act_h.p, (l - 1) * ls), 256, 0, 8);
      ol.push_back({p, 0, 256, 0, 256, Wg(l), in_[l], 0, Bg(l)});
      if (l == 4 && merge) {
        extra_b(p, L.act_in.p, nof::kInF, 0, 3);
        ol.push_back({p, 0, 256, 256, 96, Wg(4), in_[4], 256, nullptr});
      } else if (l == 4) {
        p = prob(4, at(dl, l * ls), 256, 0, 8, L.act_in.p, nof::kInF, 0, 3);
        ol.push_back({p, 0, 256, 0, 96, Wg(4), in_[4], 256, nullptr});
      }
    }
    p = prob(9, d9, nof::kD9F, 0, 5, at(L.act_h.p, 7 * ls), 256, 0, 8);
    ol.push_back({p, 0, 128, 0, 256, Wg(9), in_[9], 0, Bg(9)});
    ol.push_back({p, 128, 1, 0, 256, Wg(8), in_[8], 0, Bg(8)});
    if (merge) {  // columns 256..287: the view PE tile, 288..415: h9
      extra_b(p, L.act_in.p, nof::kInF, 96, 1);
      extra_b(p, L.act_h9.p, 128, 0, 4);
      ol.push_back({p, 0, 128, 256, 27, Wg(9), in_[9], 256, nullptr});
      ol.push_back({p, 129, 3, 288, 128, Wg(10), in_[10], 0, Bg(10)});
    } else {
      p = prob(9, d9, nof::kD9F, 0, 4, L.act_in.p, nof::kInF, 96, 1);
      ol.push_back({p, 0, 128, 0, 27, Wg(9), in_[9], 256, nullptr});
      p = prob(10, d9, nof::kD9F, 128, 1, L.act_h9.p, 128, 0, 4);
      ol.push_back({p, 1, 3, 0, 128, Wg(10), in_[10], 0, Bg(10)});
    }
    const int nq = (int)Pl.size();
    if (lev == lv0) {
      P.resize((size_t)nq * nlev);
      pbucket.resize(P.size());
      pnblk.resize(P.size());
      for (OutSpec o : ol) { o.prob *= nlev; os.push_back(o); }
    }
    NOF_REQUIRE(nq * nlev == (int)P.size(), "levels with different problem lists");
    for (int q = 0; q < nq; ++q) {
      const int i = q * nlev + (lev - lv0);
      P[i] = Pl[q];
      pbucket[i] = bl[q];
      pnblk[i] = nblk;
    }
  }
  if (bucket >= 0) {  // keep only this bucket's problems (and their outputs), renumbered
    std::vector<int> remap(P.size(), -1);
    std::vector<nof::WgProblem> Pb;
    std::vector<int> nb;
    for (size_t i = 0; i < P.size(); ++i)
      if (pbucket[i] == bucket) { remap[i] = (int)Pb.size(); Pb.push_back(P[i]); nb.push_back(pnblk[i]); }
    std::vector<OutSpec> ob;
    for (OutSpec o : os)
      if (remap[o.prob] >= 0) { o.prob = remap[o.prob]; ob.push_back(o); }
    P.swap(Pb);
    pnblk.swap(nb);
    os.swap(ob);
  }

  // cost per k-block, calibrated against per-item timings (stamps builds, make STAMPS=1,
  // tools/diag_item_time.py).  fp32 (k_wgrad, MFMA-bound): wgrad_block_cost.  f16x2 (k_wgrad_h, an
  // HBM stream): the bytes, 10 (ntr + ntc) — 1.57 / 1.11 / 1.28 / 0.49 us per block measured for the
  // 16 / 11 / 13 / 5-tile problems — and the one-column (4,1) problem 0.60 us (two active waves and
  // the bias sums on them: +12).  split (k_wgrad_x3): 10 RB CB (every wave's MFMA tiles, clamped
  // duplicates included) + 5 (ntr + ntc) (loads and splits) — 5.01 / 3.00 / 3.87 / 1.47 / 1.15 us
  // measured for the (8,8) / (8,3) / (5,8) / (4,1) / (1,4) problems = 160 / 96 / 124 / 47 / 37.
  std::vector<int64_t> cost(P.size());
  for (size_t i = 0; i < P.size(); ++i) {
    if (precision_ == NOF_PRECISION_F16) {
      // k_wgrad_s streams T = ntr + ntc tiles per block: 1.65 / 1.17 us per block measured for the
      // 16- / 11-tile problems (tools/diag_item_time.py f16); the merged 19- / 18-tile problems run
      // the unpipelined 12-accumulator path, 2.13 / 2.08 us
      const int RB = (P[i].ntr + 1) / 2, CB = (P[i].ntc + 3) / 4;
      cost[i] = (RB * CB > 8 ? 11 : 10) * (P[i].ntr + P[i].ntc);
    } else if (f16_blocks()) {
      cost[i] = 10 * (P[i].ntr + P[i].ntc) + (P[i].ntc == 1 ? 12 : 0);
    } else if (precision_ != NOF_PRECISION_F32) {
      const int WC = nof::wgrad_x3_grid_cols();  // C/2 waves per SIMD
      const int RB = (P[i].ntr + 1) / 2, CB = (P[i].ntc + WC - 1) / WC;
      // fp16 (hi, lo) pieces: 3 MFMAs per product instead of 6 (same loads and splits)
      cost[i] = (precision_ == NOF_PRECISION_F32_F16SPLIT ? 5 : 10) * RB * CB + 5 * (P[i].ntr + P[i].ntc);
    } else {
      cost[i] = nof::wgrad_block_cost(P[i].ntr, P[i].ntc, &P[i].shape);
    }
  }
  // Workgroup w takes the problem-major sequence of (problem, k-block) between the cumulative-cost
  // marks w * total / G and (w + 1) * total / G, each rounded to the nearest block: no workgroup is
  // off by more than one block and no rounding accumulates onto the last one (the greedy fill this
  // replaces closed every workgroup short and left the sum of the shortfalls to the last: measured
  // workgroup ends 229-324 us for a 253-us mean).  Problems may differ in k-blocks (levels of
  // different sample counts): a cut is a (problem, block) pair.
  // The sequence is cut as ONE group (the default) or, bucket-aligned (aligned_), as one group per
  // all-reduce bucket, workgroup w then taking its piece of every group: a bucket launch cuts its
  // group exactly so, hence an unbucketed and a bucketed step form the same items.
  const int np = (int)P.size();
  std::vector<std::vector<int>> groups;
  if (aligned_ && bucket < 0) {
    groups.resize(kBuckets);
    for (int i = 0; i < np; ++i) groups[pbucket[i]].push_back(i);
  } else {
    groups.resize(1);
    for (int i = 0; i < np; ++i) groups[0].push_back(i);
  }
  const int G_wg = num_cu_;
  // f16split (HBM-bound k_wgrad_x3<2>): problems of one level that read the same delta rows — δ4 x h3 |
  // δ4 x IPE and δ9x x h7 | δ9x x view PE | δ9x x h9, which F16 merges into wider problems instead — form
  // one scheduling unit: a workgroup's k-range of the unit becomes one item per member over the SAME
  // k-blocks, issued back to back, so the second read of the shared delta block comes from the CU's L2
  // instead of HBM.  Measured (tools/ab_multi.sh, two boxes): weight gradients 1.124 -> 1.017 ms and
  // 1.145 -> 1.034 ms, the reduce +11 us (more items per output), the step -1.9..-2.6 %.  Not kept for the
  // other modes (fp32 / split MFMA-bound: unchanged, f16x2's k_wgrad_h 4 % slower), nor for operands shared
  // as B (δ0 x IPE with δ4 x IPE: a larger reduce for no further gain).
  std::vector<int> unit_of(np);
  for (int i = 0; i < np; ++i) unit_of[i] = i;
  if (precision_ == NOF_PRECISION_F32_F16SPLIT) {
    auto root = [&](int i) {
      while (unit_of[i] != i) i = unit_of[i] = unit_of[unit_of[i]];
      return i;
    };
    for (int i = 0; i < np; ++i)
      for (int j = i + 1; j < np; ++j) {
        const nof::WgProblem &x = P[i], &y = P[j];
        if (x.level != y.level || pbucket[i] != pbucket[j] || pnblk[i] != pnblk[j] || x.A != y.A) continue;
        if (x.a_row0 < y.a_row0 + 32 * y.ntr && y.a_row0 < x.a_row0 + 32 * x.ntr) unit_of[root(j)] = root(i);
      }
    for (int i = 0; i < np; ++i) unit_of[i] = root(i);
  }
  std::vector<std::vector<nof::WgItem>> wg_items(G_wg);
  for (const std::vector<int>& grp0 : groups) {
    // the group's units in sequence order (a unit at its first member), each with its members
    std::vector<int> grp;
    std::vector<std::vector<int>> members;
    {
      std::vector<int> pos(np, -1);
      for (int i : grp0) {
        const int u = unit_of[i];
        if (pos[u] < 0) { pos[u] = (int)grp.size(); grp.push_back(u); members.emplace_back(); }
        members[pos[u]].push_back(i);
      }
    }
    const int ng = (int)grp.size();
    if (ng == 0) continue;
    std::vector<int64_t> ucost(ng, 0);
    for (int j = 0; j < ng; ++j)
      for (int i : members[j]) ucost[j] += cost[i];
    std::vector<int64_t> cum(ng + 1, 0);
    for (int j = 0; j < ng; ++j) cum[j + 1] = cum[j] + ucost[j] * pnblk[grp[j]];
    const int64_t total = cum.back();
    auto mark = [&](int w) -> std::pair<int, int> {  // the cut before workgroup w: (unit position, block)
      if (w >= G_wg) return {ng, 0};
      const double x = (double)total * w / G_wg;
      int pj = 0;
      while (pj + 1 < ng && (double)cum[pj + 1] <= x) ++pj;
      const int nb = pnblk[grp[pj]];
      const int kb = (int)std::min<int64_t>(nb, std::llround((x - (double)cum[pj]) / (double)ucost[pj]));
      return kb >= nb ? std::make_pair(pj + 1, 0) : std::make_pair(pj, kb);
    };
    for (int w = 0; w < G_wg; ++w) {
      std::pair<int, int> a = mark(w);
      const std::pair<int, int> b = std::max(a, mark(w + 1));
      while (a < b) {  // split the workgroup's range at unit boundaries
        const int pj = a.first, nb = pnblk[grp[pj]];
        const int kb1 = b.first == pj ? b.second : nb;
        if (kb1 > a.second)
          for (int i : members[pj]) {
            nof::WgItem itm;
            itm.prob = i; itm.kb0 = a.second; itm.kb1 = kb1; itm.slab = -1;
            wg_items[w].push_back(itm);
          }
        a = kb1 >= nb ? std::make_pair(pj + 1, 0) : std::make_pair(pj, kb1);
      }
    }
  }
  // slabs numbered problem-major (k-blocks ascending within a problem): the reduce sums a problem's
  // slabs first_item .. first_item + nitems - 1 in that order, whichever workgroup wrote them
  std::vector<std::pair<std::pair<int, int>, nof::WgItem*>> order;
  for (auto& v : wg_items)
    for (nof::WgItem& it : v) order.push_back({{it.prob, it.kb0}, &it});
  std::sort(order.begin(), order.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
  std::vector<int> first_item(np, -1), nitems(np, 0);
  std::vector<int> slab_prob(order.size());
  for (size_t i = 0; i < order.size(); ++i) {
    nof::WgItem& it = *order[i].second;
    it.slab = (int)i;
    slab_prob[i] = it.prob;
    if (first_item[it.prob] < 0) first_item[it.prob] = (int)i;
    nitems[it.prob]++;
  }
  std::vector<nof::WgItem> items;
  int nwg = 0;
  for (int w = 0; w < G_wg; ++w)
    if (!wg_items[w].empty()) nwg = w + 1;
  std::vector<int> item_ptr(nwg + 1, 0);
  for (int w = 0; w < nwg; ++w) {
    for (const nof::WgItem& it : wg_items[w]) items.push_back(it);
    item_ptr[w + 1] = (int)items.size();
  }
  std::vector<int64_t> slab_off(items.size());  // by slab index
  int64_t so = 0;
  for (size_t i = 0; i < slab_prob.size(); ++i) {
    slab_off[i] = so;
    so += (int64_t)P[slab_prob[i]].ntr * 32 * P[slab_prob[i]].ntc * 32;
  }
  if ((size_t)so > slab_cap_ || items.size() * 256 > bias_slabs_.n) {  // grow (schedules are built once per M)
    NOF_HIP(hipStreamSynchronize(st_));
    slab_cap_ = std::max((size_t)so, slab_cap_);
    slabs_.alloc(slab_cap_);
    bias_slabs_.alloc(std::max(items.size() * 256, bias_slabs_.n));
  }
  std::vector<nof::WgOut> outs;
  int max_elems = 0;
  for (const OutSpec& s : os) {
    nof::WgOut o;
    o.item0 = first_item[s.prob];
    o.nitems = 0;  // the problem's items at every level: problems s.prob .. s.prob + nlev - 1, contiguous
    NOF_REQUIRE(nlev <= nof::kWgMaxLevels, "too many levels");
    o.nlev = nlev;
    for (int l = 0; l < nlev; ++l) {
      NOF_REQUIRE(first_item[s.prob + l] == o.item0 + o.nitems, "a problem's items are not contiguous");
      o.lev_items[l] = nitems[s.prob + l];
      o.nitems += nitems[s.prob + l];
    }
    o.row_off = s.row_off; o.nrows = s.nrows; o.col_off = s.col_off; o.ncols = s.ncols;
    o.dst = s.dst; o.ld = s.ld; o.dst_col = s.dst_col; o.bias_dst = s.bias; o.prob = s.prob;
    outs.push_back(o);
    max_elems = std::max(max_elems, nof::wgrad_reduce_threads(s.nrows, s.ncols, s.col_off));
  }
  Schedule& sc = sched_[key];
  sc.probs.alloc(P.size());
  sc.items.alloc(items.size());
  sc.item_ptr.alloc(item_ptr.size());
  sc.slab_off.alloc(slab_off.size());
  sc.outs.alloc(outs.size());
  NOF_HIP(hipMemcpy(sc.probs.p, P.data(), P.size() * sizeof(P[0]), hipMemcpyHostToDevice));
  NOF_HIP(hipMemcpy(sc.items.p, items.data(), items.size() * sizeof(items[0]), hipMemcpyHostToDevice));
  NOF_HIP(hipMemcpy(sc.item_ptr.p, item_ptr.data(), item_ptr.size() * sizeof(int), hipMemcpyHostToDevice));
  NOF_HIP(hipMemcpy(sc.slab_off.p, slab_off.data(), slab_off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  NOF_HIP(hipMemcpy(sc.outs.p, outs.data(), outs.size() * sizeof(outs[0]), hipMemcpyHostToDevice));
  sc.nouts = (int)outs.size();
  sc.max_elems = max_elems;
  sc.num_wg = nwg;
  sc.lv0 = lv0;
  return sc;
}

void AcceleratedMLP::run_wgrad(Schedule& sc, int accumulate) {
  tb(kTWgrad);
  if (precision_ != NOF_PRECISION_F32)
    NOF_HIP(nof::launch_wgrad_x3(sc.probs.p, sc.items.p, sc.item_ptr.p, sc.num_wg, sc.slab_off.p, slabs_.p,
                                 bias_slabs_.p, precision_, st_));
  else
    NOF_HIP(nof::launch_wgrad(sc.probs.p, sc.items.p, sc.item_ptr.p, sc.num_wg, sc.slab_off.p, slabs_.p,
                              bias_slabs_.p, st_));
  te(kTWgrad);
  tb(kTWgradReduce);
  NOF_HIP(nof::launch_wgrad_reduce(sc.outs.p, sc.nouts, sc.max_elems, sc.items.p, sc.probs.p, sc.slab_off.p,
                                   slabs_.p, bias_slabs_.p, accumulate,
                                   f16_pieces() ? amax_.p + sc.lv0 : nullptr, st_));
  te(kTWgradReduce);
}

nof::BwdArgs AcceleratedMLP::bwd_args(int level, const float* color_grad, const float* density_grad) {
  Level& L = lv_[level];
  nof::BwdArgs b{};
  b.M = L.M;
  b.split = precision_;
  b.dbias = cfg_.density_bias;
  b.rgb_scale = rgb_scale();
  if (f16_pieces()) {  // the level's power-of-two delta scale
    if ((amax_given_ >> level) & 1u) {  // filled by the integrator adjoint (claim_delta_amax)
      amax_given_ &= ~(1u << level);
    } else {
      const bool cleared = (amax_cleared_ >> level) & 1u;  // by this step's pack launch, not used since
      amax_cleared_ &= ~(1u << level);
      NOF_HIP(nof::launch_delta_amax(density_grad, color_grad, L.M, amax_.p + level, st_, numeric_.p, cleared));
    }
    b.amax = amax_.p + level;
  }
  b.dsigma = density_grad; b.drgb = color_grad; b.zhead = L.zhead.p;
  b.masks = L.masks.p;
  b.wimg_b = wimg_b_.p;
  b.delta = L.delta.p; b.delta9x = L.delta9x.p;
  return b;
}

void AcceleratedMLP::run_backward(int level, const float* color_grad, const float* density_grad) {
  const nof::BwdArgs b = bwd_args(level, color_grad, density_grad);
  tb(kTMlpBwd);
  NOF_HIP(nof::launch_mlp_bwd(b, st_));
  te(kTMlpBwd);
}

// Two levels' dX chains as ONE launch (the same arithmetic per group as two launches).  F16: a persistent grid
// over level 0's groups, then level 1's; fp32 / f16x2 / f16split (k_mlp_bwd16): level 1's workgroups after level
// 0's on the grid, so the CUs are drained and refilled once per pair instead of once per level
void AcceleratedMLP::run_backward2(int level, const float* const* color_grads, const float* const* density_grads) {
  nof::BwdArgs b = bwd_args(level, color_grads[0], density_grads[0]);
  const nof::BwdArgs b1 = bwd_args(level + 1, color_grads[1], density_grads[1]);
  b.M1 = b1.M; b.dsigma1 = b1.dsigma; b.drgb1 = b1.drgb; b.zhead1 = b1.zhead; b.amax1 = b1.amax;
  b.masks1 = b1.masks; b.delta1 = b1.delta; b.delta9x1 = b1.delta9x;
  tb(kTMlpBwd);
  NOF_HIP(nof::launch_mlp_bwd(b, st_));
  te(kTMlpBwd);
}

// the weight gradients of levels [lv0, lv1) (their dX chains done): one scheduled launch + reduce, or
// with the bucket hook kBuckets of them in reverse layer order, the hook fired after each
float* const* AcceleratedMLP::wgrad_levels(int lv0, int lv1, int accumulate, bool buckets) {
  if (!buckets) {
    run_wgrad(schedule(lv0, lv1), accumulate);
  } else {
    // reverse layer order: the hook's all-reduce of layers 5..10 overlaps the layer-0..4 launch
    for (int bk = 0; bk < kBuckets; ++bk) {
      run_wgrad(schedule(lv0, lv1, bk), accumulate);
      int64_t off[2], cnt[2];
      const int ns = bucket_spans(bk, off, cnt);
      TraceRange hr("nof:gradient_bucket_hook");
      hook_(hook_user_, bk, ns, off, cnt);
    }
  }
  return grad_views_.data();
}

float* const* AcceleratedMLP::get_gradient(const float* color_grad, const float* density_grad, int level,
                                           uint32_t flags) {
  NOF_REQUIRE(level >= 0 && level < (int)lv_.size(), "level out of range");
  Level& L = lv_[level];
  NOF_REQUIRE(L.M > 0, "get_gradient before get_output for this level");
  NOF_REQUIRE(color_grad && density_grad, "null output gradients");
  NOF_REQUIRE((flags & ~(uint32_t)(NOF_GRAD_ACCUMULATE | NOF_GRAD_PUBLISH)) == 0, "unknown gradient flags");
  const bool buckets = (flags & NOF_GRAD_PUBLISH) && hook_;
  if (generic_) {
    gen_backward(level, color_grad, density_grad, (level > 0 || (flags & NOF_GRAD_ACCUMULATE)) ? 1 : 0);
    return gen_publish(buckets);
  }
  // build every schedule this call needs before the first launch (a schedule may grow the slabs,
  // which synchronises the stream)
  if (!buckets) (void)schedule(level, level + 1);
  else
    for (int b = 0; b < kBuckets; ++b) (void)schedule(level, level + 1, b);
  run_backward(level, color_grad, density_grad);
  return wgrad_levels(level, level + 1, (level > 0 || (flags & NOF_GRAD_ACCUMULATE)) ? 1 : 0, buckets);
}

float* const* AcceleratedMLP::get_gradient_levels(const float* const* color_grads, const float* const* density_grads,
                                                  uint32_t flags) {
  const int nl = (int)lv_.size();
  NOF_REQUIRE(color_grads && density_grads, "null output gradients");
  for (int l = 0; l < nl; ++l) {
    NOF_REQUIRE(lv_[l].M > 0, "get_gradient before get_output for a level");
    NOF_REQUIRE(color_grads[l] && density_grads[l], "null output gradients");
  }
  NOF_REQUIRE((flags & ~(uint32_t)(NOF_GRAD_ACCUMULATE | NOF_GRAD_PUBLISH)) == 0, "unknown gradient flags");
  const bool buckets = (flags & NOF_GRAD_PUBLISH) && hook_;
  if (generic_) {
    for (int l = 0; l < nl; ++l)
      gen_backward(l, color_grads[l], density_grads[l], (l > 0 || (flags & NOF_GRAD_ACCUMULATE)) ? 1 : 0);
    return gen_publish(buckets);
  }
  if (!buckets) (void)schedule(0, nl);
  else
    for (int b = 0; b < kBuckets; ++b) (void)schedule(0, nl, b);
  int l = 0;
  // levels in pairs, one backward launch per pair: F16 always (its persistent grid), the k_mlp_bwd16 modes unless
  // the diagnostic switch asks for per-level launches; the split mode's k_mlp_bwd<1> takes one level
  const bool pair16 = (step_fusion_ & NOF_STEP_FUSION_BWD_PAIR) &&
                      (precision_ == NOF_PRECISION_F32 || precision_ == NOF_PRECISION_F16X2 ||
                       precision_ == NOF_PRECISION_F32_F16SPLIT);
  if (precision_ == NOF_PRECISION_F16 || pair16)
    for (; l + 1 < nl; l += 2) run_backward2(l, color_grads + l, density_grads + l);
  for (; l < nl; ++l) run_backward(l, color_grads[l], density_grads[l]);
  return wgrad_levels(0, nl, (flags & NOF_GRAD_ACCUMULATE) ? 1 : 0, buckets);
}

// ------------------------------------------------------------------------------------------------
// Any-shape path (generic.hip; NOF_PRECISION_F16_PRODUCTS: the same sequence with every product but the view
// PE's weight gradient on gemm_h.hip's fp16 products, no weight-stationary kernel and no mask bits).  Per
// level: trunk activations h_l [M][W] (l < D), condition activations [M][Wc] (Dc of them), heads z [M][4]; the backward walks the layers in reverse (as
// mlp_backward_sample / MLPcpp:256-321), one dX GEMM (ReLU mask = the stored activation > 0) and one
// split-K weight-gradient GEMM + ordered slab sum per layer and input block.
// ------------------------------------------------------------------------------------------------
static nof::GemmSrc gsrc(const float* p, int64_t si, int64_t sk, int idiv = 1) {
  nof::GemmSrc s;
  s.p = p; s.si = si; s.sk = sk; s.idiv = idiv;
  return s;
}

// Every GEMM of the any-shape path picks its kernel here.  ksplit == 1: one k chunk.  ws: the weight-stationary
// kernel (gemm_ws.hip) may take the product where the mode is fp32 and the shape fits it; a masked product
// (a.G) is given the layer's ReLU bits in a.mask_in where the forward wrote them, and takes that kernel with the
// bits or k_gemm / k_gemm_h with G.  f32: fp32 k_gemm in every mode.  Returns whether the weight-stationary
// kernel ran.
bool AcceleratedMLP::gen_product(nof::GemmArgs a, int ksplit, bool ws, bool f32) {
  int v;
  if (ksplit == 1) {
    a.kchunk = (a.K1 + a.K2 + 15) / 16 * 16;
    a.slab_stride = 0;
  }
  if (ws && !f16_products() && (!a.G || a.mask_in)) {
    nof::GemmArgs w = a;
    w.G = nullptr;
    if (nof::gemm_ws_fits(w)) {
      NOF_HIP(nof::launch_gemm_ws(w, st_, &v));
      tally(v);
      return true;
    }
  }
  NOF_REQUIRE(a.G || !a.mask_in, "a ReLU-bit mask needs the weight-stationary kernel");
  a.mask_in = nullptr;
  a.mask_out = nullptr;
  if (f16_products() && !f32) {
    NOF_HIP(nof::launch_gemm_h(a, ksplit, st_, &v));
    tally_h(v);
  } else {
    NOF_HIP(nof::launch_gemm(a, ksplit, st_, &v));
    tally(v);
  }
  return false;
}

// split-K of a weight gradient (k = the level's M samples, or its rays): about 1024 workgroups (four per
// CU) over the output tiles, chunks of at least 64 k, a multiple of 16 (a chunk's k-steps run one after
// another at the loop's latency: 512-k chunks of the 4096-ray view-PE gradient, 16 workgroups, took 121 us)
void AcceleratedMLP::gen_split(int nout, int ncols, int M, int* ksplit, int* kchunk) {
  const int tiles = ((nout + 63) / 64) * ((ncols + 63) / 64);
  int ks = std::max(1, std::min((1024 + tiles - 1) / tiles, M / 64));
  const int kc = ((M + ks - 1) / ks + 15) / 16 * 16;
  *kchunk = kc;
  *ksplit = (M + kc - 1) / kc;
}

void AcceleratedMLP::gen_alloc() {
  const int NL = cfg_.num_levels;
  lv_.resize(NL);
  gl_.resize(NL);
  for (int l = 0; l < NL; ++l) {
    Level& L = lv_[l];
    GenLevel& G = gl_[l];
    L.cap = cfg_.max_rays * cfg_.num_samples[l];
    const size_t M = L.cap;
    G.mean.alloc(3 * M); G.cov.alloc(3 * M);
    G.enc_pos.alloc(M * gP_);
    G.enc_dir.alloc((size_t)cfg_.max_rays * gVd_);
    if (gG_) G.edx.alloc((size_t)cfg_.max_rays * (gVd_ + gG_));
    G.h.alloc((size_t)gD_ * M * gW_);
    G.hc.alloc((size_t)gDc_ * M * gWc_);
    G.z.alloc(4 * M);
    G.mbits.alloc((size_t)(gD_ + gDc_) * M * 4);
    G.mb_ok.assign(gD_ + gDc_, 0);
    L.sigma.alloc(M);
    L.rgb.alloc(3 * M);
    max_M_ = std::max(max_M_, L.cap);
  }
  const size_t Wm = std::max(gW_, gWc_);
  gd0_.alloc((size_t)max_M_ * Wm);
  gd1_.alloc((size_t)max_M_ * Wm);
  gdz_.alloc((size_t)max_M_ * 4);
  gray_.alloc((size_t)cfg_.max_rays * gWc_);
  if (gG_) {  // the table starts at zero: a new model renders as one without the option would
    const size_t T = (size_t)gV_ * gG_;
    app_table_.alloc(T);
    app_grad_.alloc(T);
    app_step_.alloc(T);
    NOF_HIP(hipMemset(app_table_.p, 0, T * sizeof(float)));
    NOF_HIP(hipMemset(app_grad_.p, 0, T * sizeof(float)));
    gdapp_.alloc((size_t)cfg_.max_rays * gG_);
  }
  if (cross_) denc_alloc(1);  // levels >= 1 only
  if (f16_products()) {
    amax_.alloc(NL);
    NOF_HIP(hipMemset(amax_.p, 0, NL * sizeof(uint32_t)));
  }
  // split-K slabs: a level's weight gradients each take their own region (their sums run at the end of the
  // level), sized by a dry run of gen_backward at every level's capacity (the split grows with M up to its
  // tile-count cap, so the capacity bounds every call): the same call sequence as a step, so a new layer
  // shape cannot outgrow the slab mid-step; the largest level's total
  size_t slab = 0;
  for (int l = 0; l < NL; ++l) {
    Level& L = lv_[l];
    size_t need = 0;
    wg_need_ = &need;
    L.M = L.cap; L.n = cfg_.max_rays; L.S = cfg_.num_samples[l];
    gen_backward(l, nullptr, nullptr, 0);
    L.M = L.n = L.S = 0;
    slab = std::max(slab, need);
  }
  wg_need_ = nullptr;
  gslab_.alloc(std::max<size_t>(slab, 1));
}

void AcceleratedMLP::denc_alloc(int first_level) {
  size_t Mx = 0;
  for (int l = first_level; l < (int)lv_.size(); ++l) Mx = std::max(Mx, (size_t)lv_[l].cap);
  int contrib = 1;  // layer 0 and the skip layers
  for (int l = 1; l < gD_; ++l) contrib += l % gskip_ == 0 ? 1 : 0;
  const size_t parts = contrib > 2 ? (size_t)((contrib + 1) / 2) : 0;
  if (gd2_.n >= Mx * gW_ && gdenc_.n >= Mx * gP_ && gdenc_part_.n >= parts * Mx * gP_) return;
  if (gd2_.p) NOF_HIP(hipStreamSynchronize(st_));  // (grown after construction: a step may still read them)
  gd2_.alloc(Mx * gW_);
  gdenc_.alloc(Mx * gP_);
  if (parts) gdenc_part_.alloc(parts * Mx * gP_);
}

void AcceleratedMLP::set_ray_grad(bool on) {
  if (on) {
    if (!generic_)
      throw Error(NOF_ERR_UNSUPPORTED,
                  "ray gradients need the any-shape path: the fused 8x256 kernels produce no gradient of the encoded "
                  "input (use NOF_PRECISION_F16_PRODUCTS, or NOF_PRECISION_F32 with stop_level_grad = 0)");
    denc_alloc(0);  // level 0's dEnc too
    if (!gddir_.p) {
      gddir_.alloc((size_t)cfg_.max_rays * gVd_);
      rg_o_.alloc(3 * (size_t)cfg_.max_rays);
      rg_d_.alloc(3 * (size_t)cfg_.max_rays);
    }
  }
  ray_grad_ = on;
  rg_job_ = RayGradJob();
}

void AcceleratedMLP::set_contraction(int mode) {
  NOF_REQUIRE(mode == NOF_CONTRACT_NONE || mode == NOF_CONTRACT_SPHERE, "unknown contraction mode");
  if (mode != NOF_CONTRACT_NONE && !generic_)
    throw Error(NOF_ERR_UNSUPPORTED,
                "scene contraction needs the any-shape path: the fused 8x256 kernels encode in world coordinates "
                "(use NOF_PRECISION_F16_PRODUCTS, or NOF_PRECISION_F32 with stop_level_grad = 0)");
  contraction_ = mode;
}

void AcceleratedMLP::set_render_appearance(int view) {
  NOF_REQUIRE(gG_ > 0, "the model has no appearance embeddings (nof_mipnerf_create_ex)");
  NOF_REQUIRE(view >= -1 && view < gV_, "render appearance view out of range");
  app_const_ = view;
}

void AcceleratedMLP::appearance_gather(int level, int n) {
  GenLevel& G = gl_[level];
  NOF_HIP(nof::launch_appearance_gather(n, gVd_, gG_, gV_, G.enc_dir.p, app_table_.p, app_ids_, app_const_, G.edx.p,
                                        st_));
}

void AcceleratedMLP::gen_wgrad(float* dst, int64_t ld, const float* dz, int64_t ldz, int nout, nof::GemmSrc x,
                               int ncols, int M, int accumulate, float* bias_dst, const uint32_t* scale) {
  int ks, kc;
  gen_split(nout, ncols, M, &ks, &kc);
  const size_t need = (size_t)ks * nout * (ncols + 1);  // + the bias partials
  if (wg_need_) {  // construction's dry run
    *wg_need_ += need;
    return;
  }
  NOF_REQUIRE(wg_off_ + need <= gslab_.n, "split-K slabs too small");
  float* slab = gslab_.p + wg_off_;
  wg_off_ += need;
  nof::GemmArgs a;
  a.M = nout; a.N = ncols; a.K1 = M;
  a.A1 = gsrc(dz, 1, ldz);  // A(o, m) = dZ[m][o]
  a.B1 = x;                 // B(j, m) = X[m][j]
  a.C = slab; a.ci = ncols; a.cj = 1;
  a.kchunk = kc; a.slab_stride = (int64_t)nout * ncols;
  float* bias_part = slab + (size_t)ks * nout * ncols;  // the bias gradient's per-chunk sums [ks][nout]
  if (bias_dst) a.rowsum = bias_part;
  // F16_PRODUCTS: dZ scaled inside each fp16 product, the partials unscaled; without a scale on fp32 k_gemm
  if (scale) { a.scale_amax = scale; a.scale_src = 1; }
  gen_product(a, ks, false, !scale);
  wg_jobs_.push_back({slab, dst, a.slab_stride, ld, nout, ncols, ncols, ks, accumulate});
  if (bias_dst) wg_jobs_.push_back({bias_part, bias_dst, nout, nout, 1, nout, nout, ks, accumulate});
}

void AcceleratedMLP::gen_forward(int level, const float* ep, const float* ed) {
  Level& L = lv_[level];
  GenLevel& G = gl_[level];
  const int M = L.M, S = L.S, D = gD_, W = gW_, Dc = gDc_, Wc = gWc_, P = gP_, Vd = gVd_, lr = D + 1 + Dc;
  G.ep = ep; G.ed = ed;
  const float* vx = gG_ ? G.edx.p : ed;  // the view layer's per-ray operand [n][Vx]
  const int Vx = Vd + gG_;
  const float* prm = params_.p;
  auto H = [&](int l) { return G.h.p + (size_t)l * M * W; };
  auto Hc = [&](int i) { return G.hc.p + (size_t)i * M * Wc; };
  auto MB = [&](int l) { return G.mbits.p + (size_t)l * M * 4; };  // trunk l, then condition D + i
  tb(kTMlpFwd);
  for (int l = 0; l < D; ++l) {  // trunk (MLPcs:90-100): [h | IPE] into every skip-th layer after the first
    nof::GemmArgs a;
    a.M = M; a.N = W;
    if (l == 0) {
      a.K1 = P; a.A1 = gsrc(ep, P, 1);
    } else {
      a.K1 = W; a.A1 = gsrc(H(l - 1), W, 1);
      if (l % gskip_ == 0) { a.K2 = P; a.A2 = gsrc(ep, P, 1); }
    }
    a.B1 = gsrc(prm + woff_[l], in_[l], 1);
    a.B2 = gsrc(prm + woff_[l] + a.K1, in_[l], 1);
    a.bias = prm + boff_[l]; a.relu = 1;
    a.C = H(l); a.ci = W; a.cj = 1;
    a.mask_out = MB(l);
    G.mb_ok[l] = gen_product(a, 1, true);
  }
  {  // density head (MLPcs:101): z[:, 0]
    nof::GemmArgs a;
    a.M = M; a.N = 1; a.K1 = W;
    a.A1 = gsrc(H(D - 1), W, 1);
    a.B1 = gsrc(prm + woff_[D], W, 1);
    a.bias = prm + boff_[D];
    a.C = G.z.p; a.ci = 4; a.cj = 1;
    gen_product(a, 1, true);
  }
  for (int i = 0; i < Dc; ++i) {  // view layer [h | view PE of the ray] (MLPcs:102-106), condition layers
    const int l = D + 1 + i;
    nof::GemmArgs a;
    a.M = M; a.N = Wc;
    if (i == 0) {
      a.K1 = W; a.A1 = gsrc(H(D - 1), W, 1);
      a.K2 = Vx; a.A2 = gsrc(vx, Vx, 1, S);
    } else {
      a.K1 = Wc; a.A1 = gsrc(Hc(i - 1), Wc, 1);
    }
    a.B1 = gsrc(prm + woff_[l], in_[l], 1);
    a.B2 = gsrc(prm + woff_[l] + a.K1, in_[l], 1);
    a.bias = prm + boff_[l]; a.relu = 1;
    a.C = Hc(i); a.ci = Wc; a.cj = 1;
    a.mask_out = MB(D + i);
    G.mb_ok[D + i] = gen_product(a, 1, true);
  }
  {  // rgb head (MLPcs:107): z[:, 1..3]
    nof::GemmArgs a;
    a.M = M; a.N = 3; a.K1 = Wc;
    a.A1 = gsrc(Hc(Dc - 1), Wc, 1);
    a.B1 = gsrc(prm + woff_[lr], Wc, 1);
    a.bias = prm + boff_[lr];
    a.C = G.z.p + 1; a.ci = 4; a.cj = 1;
    gen_product(a, 1, true);
  }
  NOF_HIP(nof::launch_heads_fwd(M, G.z.p, L.sigma.p, L.rgb.p, cfg_.density_bias, rgb_scale(), cfg_.rgb_padding, st_));
  te(kTMlpFwd);
}

void AcceleratedMLP::gradient_level_cross(int level, const float* color_grad, const float* density_grad,
                                          int accumulate, const float** denc) {
  NOF_REQUIRE(generic_ && cross_, "gradient_level_cross needs stop_level_grad = 0");
  NOF_REQUIRE(level >= 0 && level < (int)lv_.size() && lv_[level].M > 0, "get_gradient before get_output for this level");
  NOF_REQUIRE(color_grad && density_grad, "null output gradients");
  NOF_REQUIRE(!denc || level > 0, "level 0's encoding is a constant");
  gen_backward(level, color_grad, density_grad, accumulate, denc != nullptr);
  if (denc) *denc = gdenc_.p;
}

void AcceleratedMLP::gen_backward(int level, const float* color_grad, const float* density_grad, int acc,
                                  bool want_denc) {
  Level& L = lv_[level];
  GenLevel& G = gl_[level];
  const bool dry = wg_need_ != nullptr;  // slab sizing (gen_alloc): only gen_wgrad's records, no launches
  NOF_REQUIRE(dry || (G.ep && G.ed), "get_gradient before get_output for this level");
  const bool rays = !dry && ray_grad_ && rg_job_.n > 0;  // the owner's step wants dL/do, dL/dd (set_ray_grad)
  NOF_REQUIRE(!rays || (rg_job_.n == L.n && rg_job_.t[level]), "the ray-gradient job is not this step's");
  want_denc = want_denc || rays;
  const int M = L.M, S = L.S, D = gD_, W = gW_, Dc = gDc_, Wc = gWc_, P = gP_, Vd = gVd_, lr = D + 1 + Dc;
  const float* vx = gG_ ? G.edx.p : G.ed;  // the view layer's per-ray operand [n][Vx]
  const int Vx = Vd + gG_;
  const bool app = !dry && gG_ > 0 && app_job_.ids != nullptr;  // the owner's step: dE too
  const float* prm = params_.p;
  float* gr = grads_.p;
  auto H = [&](int l) { return G.h.p + (size_t)l * M * W; };
  auto Hc = [&](int i) { return G.hc.p + (size_t)i * M * Wc; };
  float* dz = gdz_.p;
  float *cur = gd0_.p, *nxt = gd1_.p;
  auto MB = [&](int l) -> const uint32_t* { return G.mbits.p + (size_t)l * M * 4; };
  // F16_PRODUCTS: the level's delta-scale word; every product with a delta operand scales it (null: no scale)
  const uint32_t* sc = f16_products() ? amax_.p + level : nullptr;
  // a dX product's mask, the masking layer's ReLU (mlay: trunk l, condition D + i): the activation `mask` > 0, and
  // its bits where the forward wrote them (gen_product takes one or the other)
  auto relu_mask = [&](nof::GemmArgs& a, int mlay, const float* mask, int width) {
    a.G = mask; a.gi = width; a.gj = 1;
    if (G.mb_ok[mlay]) a.mask_in = MB(mlay);
  };
  // dX of layer l into C, masked by the activation `mask` > 0: C[m][j] = sum_o dZ[m][o] W_l[o][j]
  auto dx = [&](const float* dzp, int64_t ldz, int nout, int l, int mlay, const float* mask, int width, float* C) {
    if (dry) return;
    nof::GemmArgs a;
    a.M = M; a.N = width; a.K1 = nout;
    a.A1 = gsrc(dzp, ldz, 1);
    a.B1 = gsrc(prm + woff_[l], 1, in_[l]);
    a.C = C; a.ci = width; a.cj = 1;
    if (sc) { a.scale_amax = sc; a.scale_src = 1; }
    relu_mask(a, mlay, mask, width);
    gen_product(a, 1, true);
  };
  wg_jobs_.clear();
  wg_off_ = 0;
  if (!dry) {
    if (sc) {  // the level's power-of-two delta scale (as bwd_args for the fused network)
      if ((amax_given_ >> level) & 1u) {  // filled by the integrator adjoint (claim_delta_amax)
        amax_given_ &= ~(1u << level);
      } else {
        const bool cleared = (amax_cleared_ >> level) & 1u;  // by this step's pack_weights, not used since
        amax_cleared_ &= ~(1u << level);
        NOF_HIP(nof::launch_delta_amax(density_grad, color_grad, M, amax_.p + level, st_, numeric_.p, cleared));
      }
    }
    tb(kTMlpBwd);
    NOF_HIP(nof::launch_heads_bwd(M, density_grad, color_grad, G.z.p, dz, cfg_.density_bias, rgb_scale(), st_));  // MNcs:23-28,184-189
  }
  // rgb head: dW, db from dz[:, 0..2] (k_heads_bwd: [dz_rgb, dz_sigma]); its dX into the last condition layer
  gen_wgrad(gr + woff_[lr], Wc, dz, 4, 3, gsrc(Hc(Dc - 1), 1, Wc), Wc, M, acc, gr + boff_[lr], sc);
  dx(dz, 4, 3, lr, D + Dc - 1, Hc(Dc - 1), Wc, cur);
  for (int i = Dc - 1; i >= 1; --i) {  // condition layers
    const int l = D + 1 + i;
    gen_wgrad(gr + woff_[l], Wc, cur, Wc, Wc, gsrc(Hc(i - 1), 1, Wc), Wc, M, acc, gr + boff_[l], sc);
    dx(cur, Wc, Wc, l, D + i - 1, Hc(i - 1), Wc, nxt);
    std::swap(cur, nxt);
  }
  // view layer: columns [0, W) against h_{D-1}, [W, W + Vx) against the ray's view PE (and embedding row)
  gen_wgrad(gr + woff_[D + 1], W + Vx, cur, Wc, Wc, gsrc(H(D - 1), 1, W), W, M, acc, gr + boff_[D + 1], sc);
  // (the view PE is per ray: dW_pe = sum over rays of (sum over the ray's samples of dZ) PE(ray)).  In every
  // mode on fp32 k_gemm: a sum over up to 512 samples does not share the head deltas' range (the scale
  // leaves 2^7 above their maximum), and with k = rays the product's FLOPs are negligible
  if (!dry) {
    NOF_HIP(nof::launch_ray_sum(M / S, S, Wc, cur, Wc, gray_.p, st_));
    tally(nof::kGvRaySum);
    if (rays) {  // dDir[r][f] = sum_o gray[r][o] W_view[o][W + f]: the per-ray deltas are unscaled fp32 in every mode
      nof::GemmArgs a;
      a.M = M / S; a.N = Vd; a.K1 = Wc;
      a.A1 = gsrc(gray_.p, Wc, 1);
      a.B1 = gsrc(prm + woff_[D + 1] + W, 1, W + Vx);
      a.C = gddir_.p; a.ci = Vd; a.cj = 1;
      gen_product(a, 1, false, true);
    }
    if (app) {  // dApp[r][g] = sum_o gray[r][o] W_view[o][W + Vd + g], as dDir
      nof::GemmArgs a;
      a.M = M / S; a.N = gG_; a.K1 = Wc;
      a.A1 = gsrc(gray_.p, Wc, 1);
      a.B1 = gsrc(prm + woff_[D + 1] + W + Vd, 1, W + Vx);
      a.C = gdapp_.p; a.ci = gG_; a.cj = 1;
      gen_product(a, 1, false, true);
    }
  }
  gen_wgrad(gr + woff_[D + 1] + W, W + Vx, gray_.p, Wc, Wc, gsrc(vx, 1, Vx), Vx, M / S, acc);
  // density head
  gen_wgrad(gr + woff_[D], W, dz + 3, 4, 1, gsrc(H(D - 1), 1, W), W, M, acc, gr + boff_[D], sc);
  if (!dry) {  // dh_{D-1} = dZ_view W_view[:, :W] + dz_density w_D (MLPcs:148-153, D11), masked
    nof::GemmArgs a;
    a.M = M; a.N = W; a.K1 = Wc; a.K2 = 1;
    a.A1 = gsrc(cur, Wc, 1);
    a.A2 = gsrc(dz + 3, 4, 1);
    a.B1 = gsrc(prm + woff_[D + 1], 1, W + Vx);
    a.B2 = gsrc(prm + woff_[D], 1, 0);
    a.C = nxt; a.ci = W; a.cj = 1;
    if (sc) { a.scale_amax = sc; a.scale_src = 1; }  // (A2 = dz_density is a delta as well)
    relu_mask(a, D - 1, H(D - 1), W);
    gen_product(a, 1, true);
    std::swap(cur, nxt);
  }
  // stop_level_grad = 0: dEnc = delta_0 W_0 + sum over skip layers s of delta_s W_s[:, W : W + P], two layers per
  // product (the second k source), in descending layer order.  A skip layer's delta waits in `pend` for its
  // partner: its buffer leaves the ping-pong and `spare` takes its place.  More than one product: each into its
  // own part, then one ordered sum.
  float *pend = nullptr, *spare = gd2_.p;
  int pend_l = -1, nparts = 0;
  const bool parts = want_denc && gdenc_part_.p != nullptr;
  auto denc_product = [&](const float* dA, int la, const float* dB, int lb) {
    nof::GemmArgs a;
    a.M = M; a.N = P; a.K1 = W;
    a.A1 = gsrc(dA, W, 1);
    a.B1 = gsrc(prm + woff_[la] + (la > 0 ? W : 0), 1, in_[la]);
    if (dB) {
      a.K2 = W;
      a.A2 = gsrc(dB, W, 1);
      a.B2 = gsrc(prm + woff_[lb] + (lb > 0 ? W : 0), 1, in_[lb]);
    }
    a.C = parts ? gdenc_part_.p + (size_t)nparts * M * P : gdenc_.p;
    a.ci = P; a.cj = 1;
    if (sc) { a.scale_amax = sc; a.scale_src = 1; }
    gen_product(a);
    ++nparts;
  };
  for (int l = D - 1; l >= 0; --l) {  // trunk
    float* gw = gr + woff_[l];
    if (l > 0) {
      gen_wgrad(gw, in_[l], cur, W, W, gsrc(H(l - 1), 1, W), W, M, acc, gr + boff_[l], sc);
      if (l % gskip_ == 0) gen_wgrad(gw + W, in_[l], cur, W, W, gsrc(G.ep, 1, P), P, M, acc, nullptr, sc);
    } else {
      gen_wgrad(gw, P, cur, W, W, gsrc(G.ep, 1, P), P, M, acc, gr + boff_[l], sc);
    }
    const bool contributes = want_denc && !dry && (l == 0 || l % gskip_ == 0);
    bool retire = false;  // cur becomes pend
    if (contributes) {
      if (pend) {
        denc_product(pend, pend_l, cur, l);
        spare = pend;
        pend = nullptr;
      } else if (l == 0) {
        denc_product(cur, 0, nullptr, -1);
      } else {
        retire = true;
      }
    }
    if (l > 0) {
      dx(cur, W, W, l, l - 1, H(l - 1), W, nxt);
      std::swap(cur, nxt);
      if (retire) {  // (nxt is the buffer delta_l lives in)
        pend = nxt;
        pend_l = l;
        nxt = spare;
        spare = nullptr;
      }
    }
  }
  if (nparts > 1)
    NOF_HIP(nof::launch_slab_sum(M, P, P, nparts, gdenc_part_.p, (int64_t)M * P, gdenc_.p, P, 0, st_));
  else if (nparts == 1 && parts)
    NOF_HIP(hipMemcpyAsync(gdenc_.p, gdenc_part_.p, (size_t)M * P * sizeof(float), hipMemcpyDeviceToDevice, st_));
  if (!dry) {
    int batches;
    NOF_HIP(nof::launch_slab_sums(wg_jobs_.data(), (int)wg_jobs_.size(), st_, &batches));
    tally(nof::kGvSlabSums, batches);
    te(kTMlpBwd);
  }
  if (rays) {  // before the next level's backward overwrites dEnc, the per-ray deltas and dDir
    nof::RayGradArgs ra{};
    ra.n = L.n; ra.S = S; ra.P = P; ra.min_deg = gmin_deg_; ra.Vd = Vd;
    ra.cylinder = cfg_.ray_shape == NOF_RAY_CYLINDRICAL ? 1 : 0;
    ra.contract = contraction_ != NOF_CONTRACT_NONE ? 1 : 0;
    ra.accumulate = rg_job_.first ? 0 : 1;
    ra.t = rg_job_.t[level]; ra.o = rg_job_.o; ra.d = rg_job_.d; ra.radius = rg_job_.radius;
    ra.enc = G.ep; ra.denc = gdenc_.p; ra.sigma = L.sigma.p; ra.dsigma = density_grad;
    ra.enc_dir = G.ed; ra.ddir = gddir_.p;
    ra.o_grad = rg_o_.p; ra.d_grad = rg_d_.p;
    NOF_HIP(nof::launch_ray_grad(ra, st_));
    rg_job_.first = false;
  }
  if (app) {  // before the next level's backward overwrites dApp.  The step's levels sum in launch order: all but
              // the last into app_step_ (the first overwrites), the last adds that sum and meets dE with the job's flag
    const bool last = --app_job_.left <= 0;
    if (last)
      NOF_HIP(nof::launch_appearance_grad(L.n, gG_, gV_, app_job_.ids, gdapp_.p, app_job_.first ? nullptr : app_step_.p,
                                          app_grad_.p, app_job_.accumulate, st_));
    else
      NOF_HIP(nof::launch_appearance_grad(L.n, gG_, gV_, app_job_.ids, gdapp_.p, nullptr, app_step_.p,
                                          app_job_.first ? 0 : 1, st_));
    app_job_.first = false;
  }
  wg_jobs_.clear();
}

float* const* AcceleratedMLP::gen_publish(bool buckets) {
  if (buckets)
    for (int bk = 0; bk < kBuckets; ++bk) {
      int64_t off[2], cnt[2];
      const int ns = bucket_spans(bk, off, cnt);
      TraceRange hr("nof:gradient_bucket_hook");
      hook_(hook_user_, bk, ns, off, cnt);
    }
  return grad_views_.data();
}

// ------------------------------------------------------------------------------------------------
// AcceleratedMipNeRF
// ------------------------------------------------------------------------------------------------
AcceleratedMipNeRF::AcceleratedMipNeRF(const nof_config& cfg, int app_views, int app_dim) : mlp(nullptr), cfg_(cfg) {
  check_model(cfg, app_views, app_dim);
  NOF_HIP(hipSetDevice(cfg.device));
  st_ = (hipStream_t)cfg.stream;
  seed_ = cfg.seed;
  mlp = new AcceleratedMLP(cfg.max_deg_point - cfg.min_deg_point, cfg.deg_view, cfg, app_views, app_dim);
  mlp->timer = &timer;
  const size_t N = cfg.max_rays;
  o_.alloc(3 * N); d_.alloc(3 * N); radii_.alloc(N); nears_.alloc(N); fars_.alloc(N); lm_.alloc(N); pix_.alloc(3 * N);
  const int L = cfg.num_levels;
  t_.resize(L); w_.resize(L); C_.resize(L); dsig_.resize(L); drgb_.resize(L); loss_rays_.resize(L);
  acc_.resize(L); dist_.resize(L);
  for (int l = 0; l < L; ++l) {
    const size_t S = cfg.num_samples[l];
    t_[l].alloc(N * (S + 1)); w_[l].alloc(N * S); C_[l].alloc(3 * N); acc_[l].alloc(N); dist_[l].alloc(N);
    dsig_[l].alloc(N * S); drgb_[l].alloc(3 * N * S); loss_rays_[l].alloc(N);
  }
  dist_rays_.alloc(N);
  cross_ = mlp->cross();
  if (cross_) {
    q_.resize(L); dtr_.resize(L); dtb_.resize(L); dt_.resize(L);
    for (int l = 0; l < L; ++l) {
      const size_t S = cfg.num_samples[l];
      if (l + 1 < L) q_[l].alloc(N * S);
      if (l >= 1) { dtr_[l].alloc(N * (S + 1)); dt_[l].alloc(N * (S + 1)); }
      if (l >= 1 && l + 1 < L) dtb_[l].alloc(N * (S + 1));
    }
  }
}

AcceleratedMipNeRF::~AcceleratedMipNeRF() {
  if (attached_dp) {
    mlp->set_bucket_hook(nullptr, nullptr);
    dp_model_destroyed(attached_dp, this);
  }
  delete mlp;
}

void AcceleratedMipNeRF::set_ray_views(const int32_t* ids) {
  NOF_REQUIRE(has_appearance(), "the model has no appearance embeddings (nof_mipnerf_create_ex)");
  mlp->set_ray_views(ids);
}

void AcceleratedMipNeRF::require_ray_views() const {
  NOF_REQUIRE(!has_appearance() || mlp->ray_views(),
              "a gradient step of an appearance model needs its ray views (nof_mipnerf_set_ray_views before every "
              "step)");
}

float* const* AcceleratedMipNeRF::GetGradient(int n, const float* origins, const float* directions,
                                              const float* radii, const float* nears, const float* fars,
                                              const float* loss_mults, nof_output_grad_fn cb, void* user) {
  NOF_REQUIRE(n > 0 && n <= cfg_.max_rays, "ray count out of range");
  NOF_REQUIRE(origins && directions && radii && nears && fars && loss_mults && cb, "null argument");
  require_ray_views();
  // loss-mult sum as float (D14: the reference truncates it into an int, MNcpp:61-65)
  float msum = 0.0f;
  for (int i = 0; i < n; ++i) msum += loss_mults[i];
  NOF_HIP(hipMemcpyAsync(o_.p, origins, 3 * n * sizeof(float), hipMemcpyHostToDevice, st_));
  NOF_HIP(hipMemcpyAsync(d_.p, directions, 3 * n * sizeof(float), hipMemcpyHostToDevice, st_));
  NOF_HIP(hipMemcpyAsync(radii_.p, radii, n * sizeof(float), hipMemcpyHostToDevice, st_));
  NOF_HIP(hipMemcpyAsync(nears_.p, nears, n * sizeof(float), hipMemcpyHostToDevice, st_));
  NOF_HIP(hipMemcpyAsync(fars_.p, fars, n * sizeof(float), hipMemcpyHostToDevice, st_));
  NOF_HIP(hipMemcpyAsync(lm_.p, loss_mults, n * sizeof(float), hipMemcpyHostToDevice, st_));
  return run(n, o_.p, d_.p, radii_.p, nears_.p, fars_.p, lm_.p, nullptr, msum, cb, user, NOF_GRAD_PUBLISH);
}

float* const* AcceleratedMipNeRF::GetGradientDevice(int n, const float* o, const float* d, const float* radii,
                                                    const float* nears, const float* fars, const float* loss_mults,
                                                    const float* pixels, float msum, uint32_t flags) {
  NOF_REQUIRE(n > 0 && n <= cfg_.max_rays, "ray count out of range");
  NOF_REQUIRE(o && d && radii && nears && fars && loss_mults && pixels, "null argument");
  NOF_REQUIRE(msum > 0.0f, "loss_mult_sum must be > 0");
  NOF_REQUIRE((flags & ~(uint32_t)(NOF_GRAD_ACCUMULATE | NOF_GRAD_PUBLISH)) == 0, "unknown gradient flags");
  require_ray_views();
  return run(n, o, d, radii, nears, fars, loss_mults, pixels, msum, nullptr, nullptr, flags);
}

float* const* AcceleratedMipNeRF::run(int n, const float* o, const float* d, const float* radii, const float* nears,
                                      const float* fars, const float* lm, const float* pix, float msum,
                                      nof_output_grad_fn cb_in, void* user, uint32_t flags) {
  static const char* const kFwd[] = {"nof:level0_forward", "nof:level1_forward", "nof:level2_forward",
                                     "nof:level3_forward"};
  static const char* const kBwd[] = {"nof:backward"};
  const int L = cfg_.num_levels;
  TraceRange step_range("nof:get_gradient");
  // appearance embeddings: the step's view ids feed every level's gather and its dE sum; they hold for this call
  struct ViewScope {
    AcceleratedMLP* m;
    ~ViewScope() { m->set_ray_views(nullptr); m->set_appearance_job(nullptr, 0, 0); }
  } view_scope{mlp};
  if (has_appearance()) mlp->set_appearance_job(mlp->ray_views(), (flags & NOF_GRAD_ACCUMULATE) ? 1 : 0, L);
  nof::StratArgs sa;  // level 0's t-values, by the pack launch's extra blocks
  sa.n = n; sa.S = cfg_.num_samples[0]; sa.nears = nears; sa.fars = fars; sa.randomized = cfg_.randomized;
  sa.lindisp = cfg_.lindisp; sa.seed = seed_; sa.step = step_; sa.ray_base = ray_base_; sa.t = t_[0].p;
  const bool sampled = mlp->pack_weights(&sa, d, n);  // (+ the step's per-ray view tables)
  for (int lv = 0; lv < L; ++lv) {  // MNcpp:85-123
    TraceRange lr(kFwd[lv & 3]);
    const int S = cfg_.num_samples[lv];
    if (lv == 0 && !sampled) {  // (levels >= 1: resampled by the previous level's fused integrator launch)
      timer.begin(kTSample);
      NOF_HIP(nof::launch_sample_stratified(n, S, nears, fars, cfg_.randomized, seed_, step_, 0, ray_base_,
                                            t_[0].p, st_, cfg_.lindisp));
      timer.end(kTSample);
    }
    mlp->forward_fused(lv, n, S, t_[lv].p, o, d, radii);
    // (stop_level_grad = 0 walks the levels one by one, as a callback does: the same forward launches)
    const bool cb = cb_in || cross_;
    if (lv + 1 < L || cb) timer.begin(kTRenderFwd);  // (a timer pair only around a launch)
    if (lv + 1 < L) {  // this level's integrator and the next level's resampler (ResampleAlongRay) in one launch
      nof::RenderPdfArgs ra{};
      ra.n = n; ra.S = S; ra.sigma = mlp->density(lv); ra.rgb = mlp->rgb(lv); ra.t = t_[lv].p; ra.d = d;
      ra.white = cfg_.white_bkgd; ra.C = C_[lv].p; ra.w = w_[lv].p; ra.nonfinite = mlp->numeric_flags();
      ra.S_out = cfg_.num_samples[lv + 1]; ra.padding = cfg_.resample_padding; ra.randomized = cfg_.randomized;
      ra.seed = seed_; ra.step = step_; ra.level = (uint32_t)(lv + 1); ra.ray_base = ray_base_; ra.t_out = t_[lv + 1].p;
      NOF_HIP(nof::launch_render_fwd_pdf(ra, st_));
    } else if (cb) {  // (without a callback the last level's integrator runs in the adjoint launch below)
      NOF_HIP(nof::launch_render_fwd(n, S, mlp->density(lv), mlp->rgb(lv), t_[lv].p, d, cfg_.white_bkgd, C_[lv].p,
                                     w_[lv].p, st_, nullptr, nullptr, mlp->numeric_flags()));
    }
    if (lv + 1 < L || cb) timer.end(kTRenderFwd);
  }
  // ray gradients: every level's backward below is followed by its k_ray_grad (AcceleratedMLP::RayGradJob)
  struct JobScope {
    AcceleratedMLP* m;
    ~JobScope() { m->set_ray_grad_job(nullptr); }
  } job_scope{mlp};
  if (mlp->ray_grad()) {
    AcceleratedMLP::RayGradJob job;
    job.n = n; job.o = o; job.d = d; job.radius = radii;
    for (int lv = 0; lv < L; ++lv) job.t[lv] = t_[lv].p;
    mlp->set_ray_grad_job(&job);
    ray_grad_valid_ = true;
  }
  if (cross_) {
    float* const* g = run_cross(n, o, d, radii, nears, fars, lm, pix, msum, cb_in, user, flags);
    dist_valid_ = true;
    prop_valid_ = true;
    last_n_ = n;
    last_fused_ = cb_in == nullptr;
    ++step_;
    return g;
  }
  nof_output_grad_fn cb = cb_in;
  // MNcpp:125-134: the loss gradient and the integrator adjoint of every level (with the f16 modes' delta
  // maxima), levels of equal sample count in one launch when no callback supplies dL/dC, else one level
  // at a time after its callback
  if (prop_mult_ > 0.0f && L >= 2) {
    run_interlevel(n, d, nears, fars, lm, pix, msum, cb, user);
  } else {
    nof::RenderBwdArgs ra{};
    ra.n = n; ra.d = d; ra.white = cfg_.white_bkgd; ra.pix = pix; ra.lossmult = lm; ra.msum = msum;
    ra.nonfinite = mlp->numeric_flags();
    const float dmult = cfg_.distortion_loss_mult;  // (0: the launches and instantiations without the term)
    if (dmult > 0.0f) { ra.nears = nears; ra.fars = fars; ra.lindisp = cfg_.lindisp; }
    int nb = 0;
    auto flush = [&]() {
      if (!nb) return;
      timer.begin(kTRenderBwd);
      NOF_HIP(nof::launch_render_bwd(ra, nb, st_));
      timer.end(kTRenderBwd);
      nb = 0;
    };
    for (int lv = 0; lv < L; ++lv) {
      const int S = cfg_.num_samples[lv];
      const float* g = nullptr;
      if (cb) {
        g = reinterpret_cast<const float*>(cb(user, (uint64_t)(uintptr_t)C_[lv].p, lv, msum, (uint64_t)(uintptr_t)lm));
        NOF_REQUIRE(g != nullptr, "output-gradient callback returned null");
      }
      if (nb && (cb || S != ra.S || nb == nof::kRenderMaxLevels)) flush();
      ra.S = S;
      nof::RenderBwdLevel& R = ra.lv[nb++];
      R.sigma = mlp->density(lv); R.rgb = mlp->rgb(lv); R.t = t_[lv].p; R.C = C_[lv].p; R.g_ext = g;
      R.lam = lv < L - 1 ? cfg_.coarse_loss_mult : 1.0f;
      R.dsigma = dsig_[lv].p; R.drgb = drgb_[lv].p; R.loss_rays = cb ? nullptr : loss_rays_[lv].p;
      R.amax = mlp->claim_delta_amax(lv);
      R.dist_mult = lv == L - 1 ? dmult : 0.0f;
      R.dist_rays = lv == L - 1 && dmult > 0.0f ? dist_rays_.p : nullptr;
      if (lv == L - 1 && !cb) {  // its integrator forward first, in its own blocks (k_render_bwd fwd_last)
        ra.fwd_last = 1; ra.fwd_C = C_[lv].p; ra.fwd_w = w_[lv].p;
      }
      if (cb) flush();
    }
    flush();
  }
  // MNcpp:135-142 (level 0 overwrites unless accumulating, later levels add): every level's dX chain,
  // then one weight-gradient launch over both levels' operands
  float* const* grads = nullptr;
  {
    TraceRange lr(kBwd[0]);
    std::vector<const float*> cg(L), dg(L);
    for (int lv = 0; lv < L; ++lv) { cg[lv] = drgb_[lv].p; dg[lv] = dsig_[lv].p; }
    grads = mlp->get_gradient_levels(cg.data(), dg.data(), flags);
  }
  dist_valid_ = true;
  prop_valid_ = true;
  last_n_ = n;
  last_fused_ = cb == nullptr;
  ++step_;
  return grads;
}

void AcceleratedMipNeRF::launch_interlevel_level(int n, int l, const float* lm, float msum, int accumulate) {
  const int L = cfg_.num_levels;
  nof::InterlevelArgs ia{};
  ia.n = n; ia.S_prop = cfg_.num_samples[l]; ia.S_tgt = cfg_.num_samples[L - 1]; ia.accumulate = accumulate;
  ia.t_prop = t_[l].p; ia.w_prop = w_[l].p; ia.t_tgt = t_[L - 1].p; ia.w_tgt = w_[L - 1].p;
  ia.lossmult = lm; ia.msum = msum; ia.mult = prop_mult_;
  ia.w_grad = q_[l].p; ia.rays = prop_rays_[l].p;
  timer.begin(kTRenderBwd);
  NOF_HIP(nof::launch_interlevel(ia, st_));
  timer.end(kTRenderBwd);
}

// The integrator adjoints of a stop_level_grad = 1 step with the interlevel loss (L >= 2): the last
// level alone through launch_render_bwd, exactly as without the option (its fwd_last forward gives the target w);
// k_interlevel per coarser level -> q^l; launch_render_bwd_x per coarser level with q = q^l and no t gradient.  The
// coarser levels claim no amax word: the f16 modes take theirs from the launch_delta_amax fallback of bwd_args /
// gen_backward.  With a callback the target's forward has run already, so k_interlevel goes first and the callbacks
// keep their order 0 .. L - 1, each followed by its level's launch.
void AcceleratedMipNeRF::run_interlevel(int n, const float* d, const float* nears, const float* fars, const float* lm,
                                        const float* pix, float msum, nof_output_grad_fn cb, void* user) {
  const int L = cfg_.num_levels;
  auto last = [&](const float* g) {
    const int lv = L - 1;
    nof::RenderBwdArgs ra{};
    ra.n = n; ra.S = cfg_.num_samples[lv]; ra.d = d; ra.white = cfg_.white_bkgd; ra.pix = pix; ra.lossmult = lm;
    ra.msum = msum; ra.nonfinite = mlp->numeric_flags();
    const float dmult = cfg_.distortion_loss_mult;
    if (dmult > 0.0f) { ra.nears = nears; ra.fars = fars; ra.lindisp = cfg_.lindisp; }
    nof::RenderBwdLevel& R = ra.lv[0];
    R.sigma = mlp->density(lv); R.rgb = mlp->rgb(lv); R.t = t_[lv].p; R.C = C_[lv].p; R.g_ext = g; R.lam = 1.0f;
    R.dsigma = dsig_[lv].p; R.drgb = drgb_[lv].p; R.loss_rays = cb ? nullptr : loss_rays_[lv].p;
    R.amax = mlp->claim_delta_amax(lv);
    R.dist_mult = dmult;
    R.dist_rays = dmult > 0.0f ? dist_rays_.p : nullptr;
    if (!cb) { ra.fwd_last = 1; ra.fwd_C = C_[lv].p; ra.fwd_w = w_[lv].p; }
    timer.begin(kTRenderBwd);
    NOF_HIP(nof::launch_render_bwd(ra, 1, st_));
    timer.end(kTRenderBwd);
  };
  auto coarse = [&](int lv, const float* g) {
    nof::RenderBwdXArgs ra{};
    ra.n = n; ra.S = cfg_.num_samples[lv]; ra.white = cfg_.white_bkgd; ra.d = d; ra.pix = pix; ra.lossmult = lm;
    ra.msum = msum; ra.nonfinite = mlp->numeric_flags();
    ra.sigma = mlp->density(lv); ra.rgb = mlp->rgb(lv); ra.t = t_[lv].p; ra.C = C_[lv].p; ra.g_ext = g;
    ra.lam = cfg_.coarse_loss_mult;
    ra.dsigma = dsig_[lv].p; ra.drgb = drgb_[lv].p; ra.loss_rays = cb ? nullptr : loss_rays_[lv].p;
    ra.q = q_[lv].p; ra.t_grad = nullptr;
    timer.begin(kTRenderBwd);
    NOF_HIP(nof::launch_render_bwd_x(ra, st_));
    timer.end(kTRenderBwd);
  };
  if (!cb) {
    last(nullptr);
    for (int lv = 0; lv < L - 1; ++lv) launch_interlevel_level(n, lv, lm, msum, 0);
    for (int lv = 0; lv < L - 1; ++lv) coarse(lv, nullptr);
    return;
  }
  for (int lv = 0; lv < L - 1; ++lv) launch_interlevel_level(n, lv, lm, msum, 0);
  for (int lv = 0; lv < L; ++lv) {
    const float* g = reinterpret_cast<const float*>(cb(user, (uint64_t)(uintptr_t)C_[lv].p, lv, msum, (uint64_t)(uintptr_t)lm));
    NOF_REQUIRE(g != nullptr, "output-gradient callback returned null");
    if (lv < L - 1) coarse(lv, g); else last(g);
  }
}

// stop_level_grad = 0: the backward of a step whose forward has run, levels descending.  Level l:
// the integrator adjoint with q^l (from level l + 1's resampler) -> dsigma, drgb and dt_render; the MLP backward
// (+ dEnc for l >= 1); the encoding adjoint, which also forms dt^l = (dt_render + dt_enc) + dt_bins; the
// resampler adjoint dt^l -> q^{l-1} and, for l - 1 >= 1, dt_bins^{l-1}.
float* const* AcceleratedMipNeRF::run_cross(int n, const float* o, const float* d, const float* radii,
                                            const float* nears, const float* fars, const float* lm, const float* pix,
                                            float msum, nof_output_grad_fn cb, void* user, uint32_t flags) {
  const int L = cfg_.num_levels;
  std::vector<const float*> g(L, nullptr);
  if (cb)  // every callback first, in order 0..L-1 (MNcpp:125-127)
    for (int lv = 0; lv < L; ++lv) {
      g[lv] = reinterpret_cast<const float*>(cb(user, (uint64_t)(uintptr_t)C_[lv].p, lv, msum, (uint64_t)(uintptr_t)lm));
      NOF_REQUIRE(g[lv] != nullptr, "output-gradient callback returned null");
    }
  TraceRange br("nof:backward");
  for (int lv = L - 1; lv >= 0; --lv) {
    const int S = cfg_.num_samples[lv];
    nof::RenderBwdXArgs ra{};
    ra.n = n; ra.S = S; ra.white = cfg_.white_bkgd; ra.d = d; ra.pix = pix; ra.lossmult = lm; ra.msum = msum;
    ra.nonfinite = mlp->numeric_flags();
    ra.sigma = mlp->density(lv); ra.rgb = mlp->rgb(lv); ra.t = t_[lv].p; ra.C = C_[lv].p; ra.g_ext = g[lv];
    ra.lam = lv < L - 1 ? cfg_.coarse_loss_mult : 1.0f;
    ra.dsigma = dsig_[lv].p; ra.drgb = drgb_[lv].p; ra.loss_rays = cb ? nullptr : loss_rays_[lv].p;
    ra.q = lv + 1 < L ? q_[lv].p : nullptr;
    ra.t_grad = lv >= 1 ? dtr_[lv].p : nullptr;
    // the interlevel loss joins the q^l that level l + 1's resampler adjoint has written (the target a constant)
    if (lv + 1 < L && prop_mult_ > 0.0f) launch_interlevel_level(n, lv, lm, msum, 1);
    if (lv == L - 1 && cfg_.distortion_loss_mult > 0.0f) {  // the distortion loss: dL/dw into e_k, dL/dt into dtr_
      ra.dist_mult = cfg_.distortion_loss_mult; ra.dist_rays = dist_rays_.p;
      ra.nears = nears; ra.fars = fars; ra.lindisp = cfg_.lindisp;
    }
    timer.begin(kTRenderBwd);
    NOF_HIP(nof::launch_render_bwd_x(ra, st_));
    timer.end(kTRenderBwd);
    const float* denc = nullptr;
    mlp->gradient_level_cross(lv, drgb_[lv].p, dsig_[lv].p, (lv < L - 1 || (flags & NOF_GRAD_ACCUMULATE)) ? 1 : 0,
                              lv >= 1 ? &denc : nullptr);
    if (lv == 0) break;
    timer.begin(kTSample);
    nof::EncodeGradArgs ea{};
    ea.n = n; ea.S = S; ea.P = 6 * (cfg_.max_deg_point - cfg_.min_deg_point); ea.min_deg = cfg_.min_deg_point;
    ea.cylinder = cfg_.ray_shape == NOF_RAY_CYLINDRICAL ? 1 : 0;
    ea.contract = mlp->contraction() != NOF_CONTRACT_NONE ? 1 : 0;
    ea.t = t_[lv].p; ea.o = o; ea.d = d; ea.radius = radii; ea.enc = mlp->enc_pos(lv); ea.denc = denc;
    ea.add0 = dtr_[lv].p; ea.add1 = lv + 1 < L ? dtb_[lv].p : nullptr;
    ea.t_grad = dt_[lv].p;
    NOF_HIP(nof::launch_encode_grad(ea, st_));
    nof::SamplePdfGradArgs sa{};
    sa.n = n; sa.S_in = cfg_.num_samples[lv - 1]; sa.S_out = S; sa.t_in = t_[lv - 1].p; sa.w = w_[lv - 1].p;
    sa.padding = cfg_.resample_padding; sa.randomized = cfg_.randomized; sa.seed = seed_; sa.step = step_;
    sa.level = (uint32_t)lv; sa.ray_base = ray_base_;
    sa.t_out_grad = dt_[lv].p; sa.w_grad = q_[lv - 1].p; sa.t_in_grad = lv - 1 >= 1 ? dtb_[lv - 1].p : nullptr;
    NOF_HIP(nof::launch_sample_pdf_grad(sa, st_));
    timer.end(kTSample);
  }
  return mlp->publish_cross(flags);
}

void AcceleratedMipNeRF::set_ray_grad(bool on) {
  mlp->set_ray_grad(on);
  ray_grad_valid_ = false;
}

void AcceleratedMipNeRF::ray_grad(const float** o_grad, const float** d_grad) const {
  NOF_REQUIRE(o_grad && d_grad, "null argument");
  NOF_REQUIRE(mlp->ray_grad() && ray_grad_valid_ && last_n_ > 0,
              "ray gradients are available after a step with nof_mipnerf_set_ray_grad(h, 1)");
  *o_grad = mlp->ray_o_grad();
  *d_grad = mlp->ray_d_grad();
}

void AcceleratedMipNeRF::set_interlevel_loss(float mult) {
  NOF_REQUIRE(std::isfinite(mult) && mult >= 0.0f, "interlevel_loss_mult must be finite and >= 0");
  const int L = cfg_.num_levels;
  if (mult > 0.0f && L >= 2 && prop_rays_.empty()) {  // first switched on: q^l (unless stop_level_grad = 0 has
    const size_t N = cfg_.max_rays;                   // them) and the per-ray terms
    prop_rays_.resize(L - 1);
    for (int l = 0; l + 1 < L; ++l) prop_rays_[l].alloc(N);
    if (q_.empty()) q_.resize(L);
    for (int l = 0; l + 1 < L; ++l)
      if (!q_[l].p) q_[l].alloc(N * (size_t)cfg_.num_samples[l]);
  }
  prop_mult_ = mult;
  prop_valid_ = false;  // (the stored terms belong to a step with another multiplier)
}

float AcceleratedMipNeRF::interlevel_loss() {
  const int L = cfg_.num_levels;
  if (!(prop_mult_ > 0.0f) || L < 2) return 0.0f;
  NOF_REQUIRE(prop_valid_ && last_n_ > 0, "the interlevel loss is available after a gradient step");
  std::vector<float> h(last_n_);
  double s = 0.0;
  for (int l = 0; l + 1 < L; ++l) {  // (level order, then ray order)
    NOF_HIP(hipMemcpyAsync(h.data(), prop_rays_[l].p, last_n_ * sizeof(float), hipMemcpyDeviceToHost, st_));
    NOF_HIP(hipStreamSynchronize(st_));
    for (float x : h) s += x;
  }
  return (float)s;
}

void AcceleratedMipNeRF::cross_view(int level, const float** w_grad, const float** t_grad) const {
  NOF_REQUIRE(level >= 0 && level < cfg_.num_levels, "level out of range");
  const bool prop = prop_mult_ > 0.0f && level + 1 < cfg_.num_levels;  // q^l holds the interlevel term
  *w_grad = (cross_ || prop) ? q_[level].p : nullptr;
  *t_grad = cross_ ? dt_[level].p : nullptr;
}

void AcceleratedMipNeRF::Render(int n, const float* o, const float* d, const float* radii, const float* nears,
                                const float* fars, int randomized, int white_bkgd, nof_render_out* out) {
  NOF_REQUIRE(n > 0 && n <= cfg_.max_rays, "ray count out of range");
  NOF_REQUIRE(o && d && radii && nears && fars && out, "null argument");
  const int L = cfg_.num_levels;
  struct ViewScope {  // (appearance embeddings: per-ray ids hold for this call)
    AcceleratedMLP* m;
    ~ViewScope() { m->set_ray_views(nullptr); }
  } view_scope{mlp};
  mlp->pack_weights();
  for (int lv = 0; lv < L; ++lv) {  // MNcs:40-95
    const int S = cfg_.num_samples[lv];
    if (lv == 0) {
      NOF_HIP(nof::launch_sample_stratified(n, S, nears, fars, randomized, seed_, step_, 0, ray_base_, t_[0].p, st_,
                                            cfg_.lindisp));
    } else {
      NOF_HIP(nof::launch_sample_pdf(n, cfg_.num_samples[lv - 1], t_[lv - 1].p, w_[lv - 1].p, S,
                                     cfg_.resample_padding, randomized, seed_, step_, (uint32_t)lv, ray_base_,
                                     t_[lv].p, nullptr, st_));
    }
    mlp->forward_fused(lv, n, S, t_[lv].p, o, d, radii, /*inference=*/true);
    NOF_HIP(nof::launch_render_fwd(n, S, mlp->density(lv), mlp->rgb(lv), t_[lv].p, d, white_bkgd, C_[lv].p,
                                   w_[lv].p, st_, acc_[lv].p, dist_[lv].p));
    out->comp_rgb[lv] = C_[lv].p;
    out->distance[lv] = dist_[lv].p;
    out->acc[lv] = acc_[lv].p;
  }
  out->num_levels = L;
  last_n_ = n;
  last_fused_ = false;  // no loss for a render
  dist_valid_ = false;
  prop_valid_ = false;
}

nof_level_view AcceleratedMipNeRF::level_view(int level) const {
  NOF_REQUIRE(level >= 0 && level < cfg_.num_levels, "level out of range");
  nof_level_view v;
  v.n = last_n_;
  v.samples = cfg_.num_samples[level];
  v.t = t_[level].p; v.weights = w_[level].p; v.comp_rgb = C_[level].p;
  v.density = mlp->density(level); v.rgb = mlp->rgb(level);
  v.density_grad = dsig_[level].p; v.rgb_grad = drgb_[level].p;
  return v;
}

float AcceleratedMipNeRF::loss() {
  NOF_REQUIRE(last_fused_ && last_n_ > 0, "loss is available after get_gradient_device");
  std::vector<float> h(last_n_);
  double s = 0.0;
  for (int l = 0; l < cfg_.num_levels; ++l) {
    NOF_HIP(hipMemcpyAsync(h.data(), loss_rays_[l].p, last_n_ * sizeof(float), hipMemcpyDeviceToHost, st_));
    NOF_HIP(hipStreamSynchronize(st_));
    for (float x : h) s += x;
  }
  return (float)s;
}

float AcceleratedMipNeRF::distortion_loss() {
  if (!(cfg_.distortion_loss_mult > 0.0f)) return 0.0f;
  NOF_REQUIRE(dist_valid_ && last_n_ > 0, "the distortion loss is available after a gradient step");
  std::vector<float> h(last_n_);
  NOF_HIP(hipMemcpyAsync(h.data(), dist_rays_.p, last_n_ * sizeof(float), hipMemcpyDeviceToHost, st_));
  NOF_HIP(hipStreamSynchronize(st_));
  double s = 0.0;
  for (float x : h) s += x;  // (ray order, as loss())
  return (float)s;
}

uint32_t AcceleratedMipNeRF::numeric_status(bool clear) {
  uint32_t f[2];
  NOF_HIP(hipMemcpyAsync(f, mlp->numeric_flags(), sizeof(f), hipMemcpyDeviceToHost, st_));
  NOF_HIP(hipStreamSynchronize(st_));
  if (clear) NOF_HIP(hipMemsetAsync(mlp->numeric_flags(), 0, sizeof(f), st_));
  return (f[0] ? NOF_NUMERIC_FORWARD : 0u) | (f[1] ? NOF_NUMERIC_DELTA : 0u);
}

// ------------------------------------------------------------------------------------------------
// AcceleratedAdamOptimizer
// ------------------------------------------------------------------------------------------------
AcceleratedAdamOptimizer::AcceleratedAdamOptimizer(const std::vector<int>& layer_sizes, const nof_config& cfg)
    : device_(cfg.device), sizes_(layer_sizes) {
  NOF_REQUIRE(!layer_sizes.empty(), "empty layer sizes");
  NOF_HIP(hipSetDevice(cfg.device));
  st_ = (hipStream_t)cfg.stream;
  for (int s : sizes_) {
    NOF_REQUIRE(s >= 0, "negative layer size");
    off_.push_back(total_);
    total_ += s;
  }
  m_.alloc(total_);
  v_.alloc(total_);
  NOF_HIP(hipMemset(m_.p, 0, total_ * sizeof(float)));  // D18: the reference never zeroes m, v
  NOF_HIP(hipMemset(v_.p, 0, total_ * sizeof(float)));
  partials_.alloc(4 * (size_t)nof::kAdamStatBlocks);  // the options' scratch, once: a step allocates nothing
  record_.alloc(1);
}

void AcceleratedAdamOptimizer::step(float* const* params, float* const* grads, float lr) {
  NOF_REQUIRE(params && grads, "null params/grads");
  TraceRange r("nof:adam");
  bool flat = true;
  for (size_t i = 0; i < sizes_.size(); ++i)
    flat = flat && params[i] == params[0] + off_[i] && grads[i] == grads[0] + off_[i];
  const bool opts = gathers() && total_ > 0;
  NOF_REQUIRE(!opts || flat || (int)sizes_.size() <= nof::kAdamMaxSegs,  // refused before the step counts
              "Adam's options take separately allocated tensors up to 64 of them: pass views of flat arenas");
  ++iteration_;
  // host-side bias corrections exactly as AcceleratedAdamOptimizer.cpp:26-28
  const float inv1 = 1.0f / (1.0f - std::pow(0.9f, (float)iteration_));
  const float inv2 = 1.0f / (1.0f - std::pow(0.999f, (float)iteration_));
  if (opts) {
    // the statistics pass, then the update with the decay and the clips: one launch more than the plain step,
    // both on st_ (in a data-parallel step st_ already waits for the last all-reduce), no host synchronisation.
    // The norm is global: separate tensors are the segments of one virtual arena, not one launch each.
    nof::AdamSegs s;
    if (flat) {
      s.n = 1;
      s.off[1] = total_;
      s.p[0] = params[0];
      s.g[0] = grads[0];
    } else {
      s.n = (int)sizes_.size();
      for (int i = 0; i < s.n; ++i) {
        s.off[i] = off_[i];
        s.p[i] = params[i];
        s.g[i] = grads[i];
      }
      s.off[s.n] = total_;
    }
    nof::AdamOpts o;
    o.grad_max_norm = gmn_;
    o.grad_max_val = gmv_;
    o.wdc = (2.0f * wd_) / (float)total_;
    static_assert(sizeof(nof::AdamStepStats) == sizeof(nof_step_stats), "the device record is nof_step_stats");
    NOF_HIP(nof::launch_adam_stats(total_, s, o, partials_.p, st_));
    NOF_HIP(nof::launch_adam_opt(total_, s, m_.p, v_.p, lr, inv1, inv2, o, gmn_ > 0.0f || gmv_ > 0.0f || wd_ > 0.0f,
                                 partials_.p, reinterpret_cast<nof::AdamStepStats*>(record_.p), iteration_, st_));
    gathered_ = true;
  } else if (flat) {
    NOF_HIP(nof::launch_adam(total_, params[0], grads[0], m_.p, v_.p, lr, inv1, inv2, st_));
  } else {
    for (size_t i = 0; i < sizes_.size(); ++i)
      NOF_HIP(nof::launch_adam(sizes_[i], params[i], grads[i], m_.p + off_[i], v_.p + off_[i], lr, inv1, inv2, st_));
  }
}

void AcceleratedAdamOptimizer::set_options(float grad_max_norm, float grad_max_val, float weight_decay_mult,
                                           bool stats) {
  // x >= 0 is false for a NaN too
  NOF_REQUIRE(grad_max_norm >= 0.0f && grad_max_val >= 0.0f && weight_decay_mult >= 0.0f,
              "Adam options must be >= 0 (0 = off)");
  gmn_ = grad_max_norm;
  gmv_ = grad_max_val;
  wd_ = weight_decay_mult;
  stats_ = stats;
}

void AcceleratedAdamOptimizer::get_options(float* grad_max_norm, float* grad_max_val, float* weight_decay_mult,
                                           bool* stats) const {
  if (grad_max_norm) *grad_max_norm = gmn_;
  if (grad_max_val) *grad_max_val = gmv_;
  if (weight_decay_mult) *weight_decay_mult = wd_;
  if (stats) *stats = stats_;
}

nof_step_stats AcceleratedAdamOptimizer::stats() {
  NOF_REQUIRE(gathered_, "no step has gathered statistics yet (nof_adam_set_options, then nof_adam_step)");
  nof_step_stats out;
  NOF_HIP(hipStreamSynchronize(st_));
  NOF_HIP(hipMemcpy(&out, record_.p, sizeof(out), hipMemcpyDeviceToHost));
  return out;
}

// ------------------------------------------------------------------------------------------------
// AcceleratedGradientCalculator
// ------------------------------------------------------------------------------------------------
AcceleratedGradientCalculator::AcceleratedGradientCalculator(int batch_size, const nof_config& cfg)
    : batch_(batch_size), cfg_(cfg) {
  NOF_REQUIRE(batch_size > 0, "batch_size must be > 0");
  NOF_HIP(hipSetDevice(cfg.device));
  st_ = (hipStream_t)cfg.stream;
  pixels_.alloc(3 * (size_t)batch_size);
  grad_.resize(NOF_MAX_LEVELS);
  for (auto& g : grad_) g.alloc(3 * (size_t)batch_size);
}

uint64_t AcceleratedGradientCalculator::get_output_gradient(uint64_t input, const float* host_pixels, int n,
                                                            uint64_t loss_mults, float loss_mult_sum, int level) {
  NOF_REQUIRE(n > 0 && n <= batch_, "n exceeds batch size");
  NOF_REQUIRE(level >= 0 && level < cfg_.num_levels, "level out of range");
  NOF_REQUIRE(input && host_pixels && loss_mults, "null argument");
  // D15: upload host -> device (the reference's memcpy has src/dst swapped) and keep one buffer per level
  NOF_HIP(hipMemcpyAsync(pixels_.p, host_pixels, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, st_));
  const float lam = level < cfg_.num_levels - 1 ? cfg_.coarse_loss_mult : 1.0f;
  NOF_HIP(nof::launch_output_gradient(n, reinterpret_cast<const float*>(input), pixels_.p,
                                      reinterpret_cast<const float*>(loss_mults), loss_mult_sum, lam,
                                      grad_[level].p, st_));
  return (uint64_t)(uintptr_t)grad_[level].p;
}

}  // namespace AcceleratedNeRFUtils
