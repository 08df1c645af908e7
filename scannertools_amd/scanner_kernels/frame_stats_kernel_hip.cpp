// BrightnessCPP, ContrastCPP and SharpnessCPP ops for Scanner on MI355X.
//
// Drop-in for the legacy op library's kernels (libimgproc_op.so)
//   BrightnessKernel  /root/reference/scannertools/scannertools/old/cpp_ops/imgproc.cpp:50-79
//   ContrastKernel    .../imgproc.cpp:81-131
//   SharpnessKernel   .../imgproc.cpp:133-175
// Same op declarations (imgproc.cpp:245-270: frame_input("frame") -> output("brightness" / "contrast" / "sharpness"),
// protobuf_name("ImgProcArgs")), same element (one 4-byte float per row).  The reference parses ImgProcArgs{width, height} and
// never uses them; so does this file, and a malformed message fails validate().  The reference registers the ops on
// DeviceType::CPU only; here the CPU registration stages host frames through the GPU (6.2 MB up per 1080p frame, 4 B down) and
// a DeviceType::GPU registration reads frames that are already on the device.  Both are batched: the per-frame
// cvtColor / mean / Laplacian / meanStdDev calls become ONE st_frame_moments_u8c3_* launch and ONE st_frame_stats_finish
// launch per execute() (include/scannertools_hip.h; formulas and the ContrastCPP deviation: csrc/st_framestats.hip).
#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "proto_lite.h"
#include "scannertools_hip.h"
#include "stage.h"

namespace scanner {
namespace {
// ImgProcArgs { int32 width = 1; int32 height = 2; } (old/cpp_ops/imgproc.proto): read and ignored, as the reference does
bool parse_imgproc_args(const std::vector<u8>& args) {
  std::vector<proto_lite::Field> fields;
  return proto_lite::parse(args.data(), args.size(), &fields);
}

const char* const kOpNames[] = {"BrightnessCPP", "ContrastCPP", "SharpnessCPP"};
}  // namespace

// KIND: ST_FS_BRIGHTNESS_CPP, ST_FS_CONTRAST_CPP or ST_FS_SHARPNESS_CPP.  STAGED: registered on DeviceType::CPU (host frames
// uploaded, host elements out); otherwise DeviceType::GPU (device frames, device elements).
template <int KIND, bool STAGED>
class FrameStatsKernelHIP : public BatchedKernel, public VideoKernel {
 public:
  FrameStatsKernelHIP(const KernelConfig& config)
    : BatchedKernel(config), device_(config.devices[0]), gpu_(STAGED ? staging_device_id() : config.devices[0].id), stage_(gpu_) {
    if (!parse_imgproc_args(config.args)) {
      RESULT_ERROR(&valid_, "%s: could not parse ImgProcArgs", kOpNames[KIND]);
    } else if (!STAGED && device_.type != DeviceType::GPU) {
      RESULT_ERROR(&valid_, "%s: the GPU kernel class runs on DeviceType::GPU only", kOpNames[KIND]);
    } else {
      int st = st_ctx_create(gpu_, &ctx_);
      if (st != ST_OK) RESULT_ERROR(&valid_, "st_ctx_create(%d) failed: %s (no CPU fallback exists)", gpu_, st_status_string(st));
    }
  }
  ~FrameStatsKernelHIP() {
    if (ctx_) st_ctx_destroy(ctx_);
  }
  void validate(Result* result) override {
    result->set_msg(valid_.msg());
    result->set_success(valid_.success());
  }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    const i32 n = (i32)num_rows(frame_col);
    if (n == 0) return;
    check_frame(device_, frame_col[0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8) << kOpNames[KIND] << " expects U8 frames with 3 channels";
    for (i32 i = 0; i < n; ++i)
      LOG_IF(FATAL, frame_col[i].as_const_frame()->as_frame_info() != frame_info_)
          << kOpNames[KIND] << ": frame " << i << " changes shape inside a batch";
    const i32 h = frame_info_.height(), w = frame_info_.width();
    const int what = KIND == ST_FS_SHARPNESS_CPP ? ST_FM_LAPLACIAN : ST_FM_LUMA;   // brightness and contrast skip the Laplacian
    const size_t frame_bytes = frame_info_.size(), stride = DeviceStage::align(frame_bytes);
    const size_t moments_bytes = DeviceStage::align(sizeof(int64_t) * 8 * (size_t)n);
    int st;
    if (STAGED) {
      u8* dev = stage_.reserve(stride * n + moments_bytes + sizeof(float) * (size_t)n);
      for (i32 i = 0; i < n; ++i) stage_.upload(dev + stride * i, frame_col[i].as_const_frame()->data, frame_bytes);
      int64_t* moments = (int64_t*)(dev + stride * n);
      float* out = (float*)(dev + stride * n + moments_bytes);
      st = st_frame_moments_u8c3_strided(ctx_, dev, stride, n, h, w, what, moments);
      LOG_IF(FATAL, st != ST_OK) << "st_frame_moments_u8c3_strided: " << st_ctx_last_error(ctx_);
      st = st_frame_stats_finish(ctx_, moments, n, h, w, KIND, out);
      LOG_IF(FATAL, st != ST_OK) << "st_frame_stats_finish: " << st_ctx_last_error(ctx_);
      LOG_IF(FATAL, st_ctx_sync(ctx_) != ST_OK) << "st_ctx_sync: " << st_ctx_last_error(ctx_);
      u8* output_block = new_block_buffer_size(device_, sizeof(float), n);
      stage_.download(output_block, (const u8*)out, sizeof(float) * (size_t)n);
      for (i32 i = 0; i < n; ++i) insert_element(output_columns[0], output_block + i * sizeof(float), sizeof(float));
    } else {
      int64_t* moments = (int64_t*)stage_.reserve(moments_bytes);
      frames_.resize(n);
      for (i32 i = 0; i < n; ++i) frames_[i] = frame_col[i].as_const_frame()->data;
      // one device block for the whole batch, one reference per output element
      u8* output_block = new_block_buffer(device_, sizeof(float) * (size_t)n, n);
      st = st_frame_moments_u8c3_batch(ctx_, frames_.data(), n, h, w, what, moments);
      LOG_IF(FATAL, st != ST_OK) << "st_frame_moments_u8c3_batch: " << st_ctx_last_error(ctx_);
      st = st_frame_stats_finish(ctx_, moments, n, h, w, KIND, output_block);
      LOG_IF(FATAL, st != ST_OK) << "st_frame_stats_finish: " << st_ctx_last_error(ctx_);
      st = st_ctx_sync(ctx_);  // the engine may read the elements from another stream
      LOG_IF(FATAL, st != ST_OK) << "st_ctx_sync: " << st_ctx_last_error(ctx_);
      for (i32 i = 0; i < n; ++i) insert_element(output_columns[0], output_block + i * sizeof(float), sizeof(float));
    }
  }

 private:
  DeviceHandle device_;
  int gpu_;
  DeviceStage stage_;   // staged: frames + moments + results; GPU: the moments record
  Result valid_;
  st_ctx* ctx_ = nullptr;
  std::vector<const uint8_t*> frames_;
};

typedef FrameStatsKernelHIP<ST_FS_BRIGHTNESS_CPP, false> BrightnessKernelHIP;
typedef FrameStatsKernelHIP<ST_FS_BRIGHTNESS_CPP, true> BrightnessKernelHIPStaged;
typedef FrameStatsKernelHIP<ST_FS_CONTRAST_CPP, false> ContrastKernelHIP;
typedef FrameStatsKernelHIP<ST_FS_CONTRAST_CPP, true> ContrastKernelHIPStaged;
typedef FrameStatsKernelHIP<ST_FS_SHARPNESS_CPP, false> SharpnessKernelHIP;
typedef FrameStatsKernelHIP<ST_FS_SHARPNESS_CPP, true> SharpnessKernelHIPStaged;

REGISTER_OP(BrightnessCPP).frame_input("frame").output("brightness").protobuf_name("ImgProcArgs");
REGISTER_KERNEL(BrightnessCPP, BrightnessKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);
REGISTER_KERNEL(BrightnessCPP, BrightnessKernelHIP).device(DeviceType::GPU).batch().num_devices(1);

REGISTER_OP(ContrastCPP).frame_input("frame").output("contrast").protobuf_name("ImgProcArgs");
REGISTER_KERNEL(ContrastCPP, ContrastKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);
REGISTER_KERNEL(ContrastCPP, ContrastKernelHIP).device(DeviceType::GPU).batch().num_devices(1);

REGISTER_OP(SharpnessCPP).frame_input("frame").output("sharpness").protobuf_name("ImgProcArgs");
REGISTER_KERNEL(SharpnessCPP, SharpnessKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);
REGISTER_KERNEL(SharpnessCPP, SharpnessKernelHIP).device(DeviceType::GPU).batch().num_devices(1);
}  // namespace scanner
