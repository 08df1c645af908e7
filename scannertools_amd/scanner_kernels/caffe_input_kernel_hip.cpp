// CaffeInput op for Scanner on MI355X: a decoded frame becomes a Caffe network's float input.
//
// Drop-in for the reference's kernel
//   CaffeInputKernel  /root/reference/scannertools_caffe/scannertools_caffe_cpp/caffe_input_kernel.cpp:15-208,
//                     caffe_input_kernel_cpu.cpp (registration), caffe_input_transformer_base.h (the Halide pipeline)
// Same op declaration (frame_input("frame") -> frame_output("caffe_frame"), protobuf_name("CaffeInputArgs")), same
// arguments (CaffeInputArgs{net_descriptor = 1, batch_size = 2}, scannertools_caffe.proto:28-31), same output frame:
// FrameInfo(3, net_h, net_w, F32), planar, planes B, G, R.  Of NetDescriptor the fields input_width (5), input_height (6),
// mean_colors (7, in B, G, R order) and normalize (11) are used; input_width == -1 means the frame's own size.  Every other
// field (mean_image, preserve_aspect_ratio, transpose, pad_mod, ...) is ignored, as the reference kernel ignores it, and so
// is its unused transform_caffe path.  The reference runs a Halide pipeline per frame; here ONE st_caffe_input_batch()
// call covers the whole batch.
// Known deviation: a geometry in which some output's filter window is empty (non-integer enlargements such as 16 -> 24;
// the reference divides 0 by 0 there) is fatal in new_frame_info() instead of producing NaN.
#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "caffe_args.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {
template <bool STAGED>
class CaffeInputKernelHIPImpl : public BatchedKernel, public VideoKernel {
 public:
  CaffeInputKernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    if (!parse_caffe_args(config.args.data(), config.args.size(), &args_)) {   // CaffeInputArgs has CaffeArgs' fields
      RESULT_ERROR(&core_.valid, "Could not parse CaffeInputArgs");
    } else if (args_.mean_colors.size() != 3) {
      RESULT_ERROR(&core_.valid, "CaffeInput: net_descriptor.mean_colors must hold 3 values, got %d", (int)args_.mean_colors.size());
    } else if (args_.input_width != -1 && (args_.input_width <= 0 || args_.input_height <= 0)) {
      RESULT_ERROR(&core_.valid, "CaffeInput: net_descriptor.input_width and input_height must be positive (or input_width -1 for the frame's size), got %d x %d",
                   args_.input_width, args_.input_height);
    } else {
      core_.open("CaffeInputKernelHIP");
    }
  }
  void validate(Result* result) override { core_.validate(result); }

  void new_frame_info() override {
    // caffe_input_kernel.cpp:35-43
    if (args_.input_width == -1) {
      net_input_width_ = frame_info_.width();
      net_input_height_ = frame_info_.height();
    } else {
      net_input_width_ = args_.input_width;
      net_input_height_ = args_.input_height;
    }
    std::vector<int> b(std::max(net_input_width_, net_input_height_)), f(b.size()), c(b.size());
    const bool ok = st_caffe_input_axis(frame_info_.width(), net_input_width_, b.data(), f.data(), c.data()) == ST_OK &&
                    st_caffe_input_axis(frame_info_.height(), net_input_height_, b.data(), f.data(), c.data()) == ST_OK;
    LOG_IF(FATAL, !ok) << "CaffeInput: " << frame_info_.width() << "x" << frame_info_.height() << " -> " << net_input_width_ << "x"
                       << net_input_height_ << " has an empty filter window (the reference divides 0 by 0 there)";
  }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    i32 input_count = (i32)num_rows(frame_col);
    if (input_count == 0) return;
    const auto eval_start = now();  // caffe_input_kernel.cpp:179
    check_frame(core_.device, frame_col[0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8)
        << "CaffeInput expects U8 frames with 3 channels";
    check_batch_shape(frame_col, frame_info_, "CaffeInput");
    FrameInfo net_input_info(3, net_input_height_, net_input_width_, FrameType::F32);  // caffe_input_kernel.cpp:186
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
    ST_CHECK(core_.ctx, st_caffe_input_batch(core_.ctx, src_.data(), input_count, frame_info_.height(), frame_info_.width(), net_input_height_,
                                             net_input_width_, args_.mean_colors.data(), args_.normalize ? 1 : 0, dst_.data()));
    core_.sync();
    if (STAGED) stage_.download_frames(output_frames, dev_out, out_stride, out_bytes);
    for (i32 i = 0; i < input_count; ++i) insert_frame(output_columns[0], output_frames[i]);
    if (profiler_) profiler_->add_interval("caffe:transform_input", eval_start, now());  // caffe_input_kernel.cpp:197-199
  }

 private:
  KernelCore core_;
  DeviceStage stage_;
  CaffeArgsLite args_;
  int net_input_width_ = 0, net_input_height_ = 0;
  std::vector<const uint8_t*> src_;
  std::vector<float*> dst_;
};

using CaffeInputKernelHIP = CaffeInputKernelHIPImpl<false>;
using CaffeInputKernelHIPStaged = CaffeInputKernelHIPImpl<true>;

REGISTER_OP(CaffeInput).frame_input("frame").frame_output("caffe_frame").protobuf_name("CaffeInputArgs");

REGISTER_KERNEL(CaffeInput, CaffeInputKernelHIP).device(DeviceType::GPU).batch().num_devices(1);

REGISTER_KERNEL(CaffeInput, CaffeInputKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);
}
