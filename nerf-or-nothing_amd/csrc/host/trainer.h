// Data path and training-state persistence around the hot path:
//   * RayDataset — BinDataset (BinDataset.cs:10-53) made device-resident: the 64-byte records live
//     in HBM and a batch is one gather launch (dataset.hip) instead of 1024 file seeks per step;
//     or image-backed: poses and an image pyramid in HBM, the rays generated in the batch gather;
//   * checkpoints — Config.SaveEvery (TrainState.cs:59) is declared but never implemented by the
//     reference; here a step's full state (parameters, Adam moments and step, Philox state) is
//     written and restored bit-exactly.
#pragma once
#include <thread>

#include "accelerated.h"

namespace AcceleratedNeRFUtils {

// A scene for the image-backed dataset: poses (host, V x [R row-major | t]), full-resolution device
// images [V][H][W][3] (or null: rgb = 0), trained at num_scales resolutions (multiscale_layout).
struct ImageScene {
  const float* host_poses;
  int num_views, width, height;
  float focal, near, far;
  int ndc;
  const float* dev_images;
  int num_scales, disable_multiscale_loss;
};
// The multiscale record layout (launch.h), or NOF_ERR_INVALID_ARG; needs no device.
nof::MultiscaleLayout multiscale_layout(int width, int height, float focal, int num_scales,
                                        int disable_multiscale_loss, int num_views);

class RayDataset {
 public:
  RayDataset(const float* host_records, int64_t count, int device);  // copy of count x 16 floats
  // A record file.  max_resident < 0: the whole file in HBM unless it exceeds half the device's free
  // memory; otherwise in HBM iff it holds at most max_resident records.  A file that is not resident
  // is STREAMED: each batch's records are read from the file (BinDataset.cs:31-38) into pinned host
  // memory, copied to the device and unpacked by the same gather — bit-identical batches — with the
  // next step's records prefetched on a host thread while this step runs (double-buffered).
  RayDataset(const std::string& path, int device, int64_t max_resident = -1);
  ~RayDataset();
  // generate the records on the device from poses (V x 12 floats, host) and optional device images
  RayDataset(const float* host_poses, int V, int w, int h, float focal, float near, float far, int ndc,
             const float* dev_images, int device);
  // Image-backed: the pose table and the image pyramid (level 0 copied from scene.dev_images, which
  // is only read during the call) stay in HBM; no record is stored, next() generates the drawn ones.
  RayDataset(const ImageScene& scene, int device);
  int64_t count() const { return count_; }
  int device() const { return device_; }
  bool streaming() const { return fd_ >= 0; }
  bool image_backed() const { return poses_.p != nullptr; }
  // Every record in order into dev_records (count x 16 floats): generated for an image-backed
  // dataset, copied for a resident one; a streaming dataset refuses (NOF_ERR_UNSUPPORTED).
  void materialize(float* dev_records, hipStream_t st);
  // Gather n records for (seed, step, first global ray id); device SoA views owned by the dataset
  // (valid until the next call).  host_msum != null: also the loss-multiplier sum (synchronises st).
  void next(int n, uint64_t seed, uint32_t step, uint32_t ray_base, hipStream_t st, nof_batch* out, float* host_msum);
  // image-backed: the scene's shape (the layout's rows) and whether it keeps an image pyramid
  const nof::MultiscaleLayout& layout() const { return layout_; }
  bool has_images() const { return pyr_.p != nullptr; }
  // A whole view (or, host_pose != null, a novel pose: 12 floats) at `scale`, rendered by `model` on its
  // stream in chunks of its max_rays from pixel 0: per chunk the ray generator, model.Render (randomized 0,
  // the model's white_bkgd), then the store-and-score launch (view.hip).  metrics == null: no
  // synchronisation; else one, at the end.  Arguments are refused before any launch (include/nof.h
  // nof_dataset_render_view).  The chunk rays are buffers of their own: next()'s batch stays as it is.
  void render_view(AcceleratedMipNeRF& model, int view, const float* host_pose, int scale, const nof_view_out& out,
                   nof_view_metrics* metrics, uint32_t flags);
  // Image-backed, ndc = 0 (else NOF_ERR_UNSUPPORTED, before any launch): the gradients [n][3] of the LAST next()
  // batch's rays summed per view into dev_pose_grad [V][12] (dataset.hip k_pose_grad), on st.
  void pose_grad(int n, const float* dev_o_grad, const float* dev_d_grad, float* dev_pose_grad, int accumulate,
                 hipStream_t st);
  // Image-backed (else NOF_ERR_UNSUPPORTED): the view of every ray of the LAST next() batch -> dev_view_ids [n]
  // (dataset.hip k_batch_views), on st.
  void batch_views(int n, int32_t* dev_view_ids, hipStream_t st);
  // The pose table (V x 12, host).  set_poses waits for the device's work, then copies: the next gather and
  // render_view read the new poses.
  void get_poses(float* host_poses);
  void set_poses(const float* host_poses);

 private:
  void reserve(int n, hipStream_t st);
  void reserve_view(int chunk, bool scratch_rgb);
  // streaming: fetch the records of (seed, step, ray_base, n) into pinned buffer b
  void fetch(int b, int n, uint64_t seed, uint32_t step, uint32_t ray_base);
  int device_;
  int64_t count_ = 0;
  // resident: every record; streaming: the staging slot of one batch; image-backed: unused
  DevBuf<float> rec_;
  // image-backed state: the layout, the scene's constants, the pose table (V x 12) and the pyramid
  // (count x 3 floats in record order; unallocated for a scene without images)
  nof::MultiscaleLayout layout_{};
  float near_ = 0.0f, far_ = 0.0f;
  int ndc_ = 0;
  DevBuf<float> poses_, pyr_;
  // streaming state: the file, two pinned record buffers (n x 64 B), the device staging slots, the
  // event after each buffer's last copy, and the prefetch (its key and its host thread)
  int fd_ = -1;
  float* hrec_[2] = {nullptr, nullptr};
  hipEvent_t copied_[2] = {nullptr, nullptr};
  hipEvent_t gathered_ = nullptr;  // after the last gather from the staging slot
  int cur_ = 0, pre_buf_ = 1;
  struct Key {
    int n; uint64_t seed; uint32_t step, ray_base; bool valid;
    bool same(const Key& o) const {
      return valid && o.valid && n == o.n && seed == o.seed && step == o.step && ray_base == o.ray_base;
    }
  };
  Key pre_{0, 0, 0, 0, false};
  Key cur_key_{0, 0, 0, 0, false};  // the records held by pinned buffer cur_
  std::thread prefetch_;
  std::string prefetch_error_;
  int cap_ = 0;
  int last_n_ = 0;  // rays of the last next() batch (idx_ holds their record indices)
  DevBuf<float> o_, d_, vd_, r_, nr_, fr_, lm_, pix_, msum_;
  DevBuf<int> idx_;
  // render_view's state: the chunk's rays, the score's per-block partials ([levels][blocks of a scale-0
  // view]) and sums, the last level's image when SSIM is asked for and the caller keeps none, and the event
  // after the last call's work (a call on another stream waits for it before it reuses the buffers)
  int vcap_ = 0, vblocks_ = 0;
  DevBuf<float> vo_, vd_rays_, vr_, vnr_, vfr_, vrgb_;
  DevBuf<double> vpart_, vsum_;
  hipEvent_t view_done_ = nullptr;
};

// Dataset.GenerateRays (+ the LLFF NDC override) on the device: poses (host, V x [R row-major | t]),
// optional device images [V][H][W][3] -> device records (V*H*W x 16 floats).
void generate_rays(const float* host_poses, int V, int w, int h, float focal, float near, float far, int ndc,
                   const float* dev_images, float* dev_records, hipStream_t st);
// LLFFDataset.RecenterPoses (Dataset.cs:309-319), in place on host poses (fp32, C# evaluation order).
void recenter_poses(float* poses, int V);

void save_checkpoint(const std::string& path, AcceleratedMipNeRF& model, AcceleratedAdamOptimizer& adam);
void load_checkpoint(const std::string& path, AcceleratedMipNeRF& model, AcceleratedAdamOptimizer& adam);

}  // namespace AcceleratedNeRFUtils
