// FacenetInput op for Scanner on MI355X: a decoded frame becomes the Facenet detector's float input.
//
// Drop-in for the reference's kernel
//   FacenetInputKernelCPU  /root/reference/scannertools_caffe/scannertools_caffe_cpp/facenet_input_kernel_cpu.cpp:9-145
// Same op declaration (frame_input("frame") -> frame_output("facenet_input"), protobuf_name("FacenetArgs")), same
// arguments (FacenetArgs{caffe_args = 1, templates_path = 2, scale = 3, threshold = 4}, scannertools_caffe.proto:38-43:
// `scale` and caffe_args.net_descriptor.mean_colors are used, templates_path and threshold are parsed and ignored, as in
// the reference), same output frame: FrameInfo(3, net_w, net_h, F32), every plane transposed, channels in frame order.
// The reference issues a resize, a conversion, a subtraction, a split, three transposes and three plane copies per
// frame; here ONE st_facenet_input_batch() call covers the whole batch.  Parity is with this CPU kernel: the reference's
// CUDA twin (facenet_input_kernel_gpu.cpp) resizes in float.
// Differences in registration: the reference registers the op without .batch() (Scanner then hands its BatchedKernel one
// row per call); both registrations here are batched, so that one launch serves a whole work packet.  mean_colors may
// arrive packed (what proto3 writes) or unpacked.
#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "caffe_args.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {
template <bool STAGED>
class FacenetInputKernelHIPImpl : public BatchedKernel, public VideoKernel {
 public:
  FacenetInputKernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    // FacenetArgs.scale (field 3) and FacenetArgs.caffe_args (1) . net_descriptor (1) . mean_colors (7)
    CaffeArgsLite args;
    std::vector<proto_lite::Field> top;
    const bool parsed = parse_wrapped_caffe_args(config.args.data(), config.args.size(), &args, &top);
    for (auto& f : top)
      if (f.number == 3 && f.wire == 5) scale_ = proto_lite::as_float(f);
    const std::vector<f32>& mean = args.mean_colors;
    if (!parsed) {
      RESULT_ERROR(&core_.valid, "Could not parse FacenetArgs");
    } else if (!(scale_ > 0.f)) {
      RESULT_ERROR(&core_.valid, "FacenetInput: scale must be positive, got %f", scale_);
    } else if (mean.size() != 3) {
      RESULT_ERROR(&core_.valid, "FacenetInput: net_descriptor.mean_colors must hold 3 values, got %d", (int)mean.size());
    } else {
      std::copy(mean.begin(), mean.end(), mean_);
      core_.open("FacenetInputKernelHIP");
    }
  }
  void validate(Result* result) override { core_.validate(result); }

  void new_frame_info() override {
    // facenet_input_kernel_cpu.cpp:21-29
    const bool ok = st_facenet_geometry(frame_info_.height(), frame_info_.width(), scale_, &net_input_height_, &net_input_width_) == ST_OK;
    LOG_IF(FATAL, !ok) << "FacenetInput: frame " << frame_info_.width() << "x" << frame_info_.height()
                       << " at scale " << scale_ << " gives an empty network input";
  }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    i32 input_count = (i32)num_rows(frame_col);
    if (input_count == 0) return;
    const auto eval_start = now();
    check_frame(core_.device, frame_col[0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8)
        << "FacenetInput expects U8 frames with 3 channels";
    check_batch_shape(frame_col, frame_info_, "FacenetInput");
    FrameInfo net_input_info(3, net_input_width_, net_input_height_, FrameType::F32);  // facenet_input_kernel_cpu.cpp:75
    std::vector<Frame*> output_frames = new_frames(core_.device, net_input_info, input_count);
    const size_t in_bytes = frame_info_.size(), out_bytes = net_input_info.size();
    const size_t in_stride = DeviceStage::align(in_bytes), out_stride = DeviceStage::align(out_bytes);
    u8* dev_out = nullptr;
    if (STAGED) {
      // device layout: [input_count frames][input_count network inputs]
      u8* dev = stage_.reserve((in_stride + out_stride) * input_count);
      dev_out = dev + in_stride * input_count;
      stage_.upload_frames(dev, in_stride, frame_col, in_bytes);
      strided_ptrs(src_, input_count, dev, in_stride);
      strided_ptrs(dst_, input_count, dev_out, out_stride);
    } else {
      input_ptrs(src_, frame_col);
      output_ptrs(dst_, output_frames);
    }
    ST_CHECK(core_.ctx, st_facenet_input_batch(core_.ctx, src_.data(), input_count, frame_info_.height(), frame_info_.width(), scale_, mean_, dst_.data()));
    core_.sync();
    if (STAGED) stage_.download_frames(output_frames, dev_out, out_stride, out_bytes);
    for (i32 i = 0; i < input_count; ++i) insert_frame(output_columns[0], output_frames[i]);
    if (profiler_) profiler_->add_interval("facenet_input", eval_start, now());
  }

 private:
  KernelCore core_;
  DeviceStage stage_;
  f32 scale_ = 0.f;
  f32 mean_[3] = {0.f, 0.f, 0.f};
  int net_input_width_ = 0, net_input_height_ = 0;
  std::vector<const uint8_t*> src_;
  std::vector<float*> dst_;
};

using FacenetInputKernelHIP = FacenetInputKernelHIPImpl<false>;
using FacenetInputKernelHIPStaged = FacenetInputKernelHIPImpl<true>;

REGISTER_OP(FacenetInput).frame_input("frame").frame_output("facenet_input").protobuf_name("FacenetArgs");

REGISTER_KERNEL(FacenetInput, FacenetInputKernelHIP).device(DeviceType::GPU).batch().num_devices(1);

REGISTER_KERNEL(FacenetInput, FacenetInputKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);
}
