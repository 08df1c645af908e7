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
#include "kernel_core.h"

namespace scanner {
namespace {
// ImgProcArgs { int32 width = 1; int32 height = 2; } (old/cpp_ops/imgproc.proto): read and ignored, as the reference does
bool parse_imgproc_args(const std::vector<u8>& args) {
  std::vector<proto_lite::Field> fields;
  return proto_lite::parse(args.data(), args.size(), &fields);
}

const char* const kOpNames[] = {"BrightnessCPP", "ContrastCPP", "SharpnessCPP"};
const char* const kClassNames[] = {"BrightnessKernelHIP", "ContrastKernelHIP", "SharpnessKernelHIP"};
}  // namespace

// KIND: ST_FS_BRIGHTNESS_CPP, ST_FS_CONTRAST_CPP or ST_FS_SHARPNESS_CPP.  STAGED: registered on DeviceType::CPU (host frames
// uploaded, host elements out); otherwise DeviceType::GPU (device frames, device elements).
template <int KIND, bool STAGED>
class FrameStatsKernelHIP : public BatchedKernel, public VideoKernel {
 public:
  FrameStatsKernelHIP(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    if (!parse_imgproc_args(config.args)) RESULT_ERROR(&core_.valid, "%s: could not parse ImgProcArgs", kOpNames[KIND]);
    else core_.open(kClassNames[KIND]);
  }
  void validate(Result* result) override { core_.validate(result); }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    const i32 n = (i32)num_rows(frame_col);
    if (n == 0) return;
    check_frame(core_.device, frame_col[0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8) << kOpNames[KIND] << " expects U8 frames with 3 channels";
    check_batch_shape(frame_col, frame_info_, kOpNames[KIND]);
    const i32 h = frame_info_.height(), w = frame_info_.width();
    const int what = KIND == ST_FS_SHARPNESS_CPP ? ST_FM_LAPLACIAN : ST_FM_LUMA;   // brightness and contrast skip the Laplacian
    const size_t frame_bytes = frame_info_.size(), stride = DeviceStage::align(frame_bytes);
    const size_t moments_bytes = DeviceStage::align(sizeof(int64_t) * 8 * (size_t)n);
    st_ctx* ctx = core_.ctx;
    if (STAGED) {
      // device layout: [n frames][moments][n results]
      u8* dev = stage_.reserve(stride * n + moments_bytes + sizeof(float) * (size_t)n);
      stage_.upload_frames(dev, stride, frame_col, frame_bytes);
      int64_t* moments = (int64_t*)(dev + stride * n);
      float* out = (float*)(dev + stride * n + moments_bytes);
      ST_CHECK(ctx, st_frame_moments_u8c3_strided(ctx, dev, stride, n, h, w, what, moments));
      ST_CHECK(ctx, st_frame_stats_finish(ctx, moments, n, h, w, KIND, out));
      core_.sync();
      u8* output_block = new_block_buffer_size(core_.device, sizeof(float), n);
      stage_.download(output_block, (const u8*)out, sizeof(float) * (size_t)n);
      for (i32 i = 0; i < n; ++i) insert_element(output_columns[0], output_block + i * sizeof(float), sizeof(float));
    } else {
      int64_t* moments = (int64_t*)stage_.reserve(moments_bytes);
      input_ptrs(frames_, frame_col);
      // one device block for the whole batch, one reference per output element
      u8* output_block = new_block_buffer(core_.device, sizeof(float) * (size_t)n, n);
      ST_CHECK(ctx, st_frame_moments_u8c3_batch(ctx, frames_.data(), n, h, w, what, moments));
      ST_CHECK(ctx, st_frame_stats_finish(ctx, moments, n, h, w, KIND, output_block));
      core_.sync();  // the engine may read the elements from another stream
      for (i32 i = 0; i < n; ++i) insert_element(output_columns[0], output_block + i * sizeof(float), sizeof(float));
    }
  }

 private:
  KernelCore core_;
  DeviceStage stage_;   // staged: frames + moments + results; GPU: the moments record
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
