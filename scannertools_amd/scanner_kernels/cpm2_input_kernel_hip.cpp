// CPM2Input op for Scanner on MI355X (pose path, BASELINE config 5).
//
// Drop-in for the reference's kernel
//   CPM2InputKernel  /root/reference/scannertools_caffe/scannertools_caffe_cpp/cpm2_input_kernel_gpu.cpp:26-187
// Same op declaration (frame_input("frame") -> frame_output("cpm2_input")), same arguments (CPM2Args{caffe_args
// = 1, scale = 2}, scannertools_caffe.proto:45-48; only `scale` is used, as in the reference), same output
// frame: FrameInfo(3, net_h, net_w, F32), planes B, G, R of the resized, padded, (x/256 - 0.5)-scaled frame.
// The reference issues six OpenCV-CUDA calls and a 2-D copy per frame on one of 32 streams; here ONE
// st_cpm2_input_batch() call covers the whole batch.  The reference registers the op on DeviceType::GPU
// only; a DeviceType::CPU registration (host frames staged through the GPU) is added, as for the imgproc ops.
#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "proto_lite.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {
namespace {
// CPM2Args (scannertools_caffe.proto:45-48): CaffeArgs caffe_args = 1; float scale = 2;
bool parse_cpm2_scale(const std::vector<u8>& args, f32* scale) {
  std::vector<proto_lite::Field> fields;
  *scale = 0.f;
  if (!proto_lite::parse(args.data(), args.size(), &fields)) return false;
  for (auto& f : fields)
    if (f.number == 2 && f.wire == 5) *scale = proto_lite::as_float(f);
  return true;
}
}  // namespace

template <bool STAGED>
class CPM2InputKernelHIPImpl : public BatchedKernel, public VideoKernel {
 public:
  CPM2InputKernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    if (!parse_cpm2_scale(config.args, &scale_)) {
      RESULT_ERROR(&core_.valid, "Could not parse CPM2Args");
    } else if (!(scale_ > 0.f)) {
      RESULT_ERROR(&core_.valid, "CPM2Input: scale must be positive, got %f", scale_);
    } else {
      core_.open("CPM2InputKernelHIP");
    }
  }
  void validate(Result* result) override { core_.validate(result); }

  void new_frame_info() override {
    // cpm2_input_kernel_gpu.cpp:44-55
    const bool ok = st_cpm2_geometry(frame_info_.height(), frame_info_.width(), scale_, &resize_height_, &resize_width_,
                                     &net_input_height_, &net_input_width_) == ST_OK;
    LOG_IF(FATAL, !ok) << "CPM2Input: frame " << frame_info_.width() << "x" << frame_info_.height()
                               << " at scale " << scale_ << " gives an empty network input";
  }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    i32 input_count = (i32)num_rows(frame_col);
    if (input_count == 0) return;
    const auto eval_start = now();  // cpm2_input_kernel_gpu.cpp:92
    check_frame(core_.device, frame_col[0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8)
        << "CPM2Input expects U8 frames with 3 channels";
    check_batch_shape(frame_col, frame_info_, "CPM2Input");
    FrameInfo net_input_info(3, net_input_height_, net_input_width_, FrameType::F32);
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
    ST_CHECK(core_.ctx, st_cpm2_input_batch(core_.ctx, src_.data(), input_count, frame_info_.height(), frame_info_.width(), scale_, dst_.data()));
    core_.sync();
    if (STAGED) stage_.download_frames(output_frames, dev_out, out_stride, out_bytes);
    for (i32 i = 0; i < input_count; ++i) insert_frame(output_columns[0], output_frames[i]);
    if (profiler_) profiler_->add_interval("cpm2_input", eval_start, now());  // cpm2_input_kernel_gpu.cpp:153-155
  }

 private:
  KernelCore core_;
  DeviceStage stage_;
  f32 scale_ = 0.f;
  int resize_width_ = 0, resize_height_ = 0, net_input_width_ = 0, net_input_height_ = 0;
  std::vector<const uint8_t*> src_;
  std::vector<float*> dst_;
};

using CPM2InputKernelHIP = CPM2InputKernelHIPImpl<false>;
using CPM2InputKernelHIPStaged = CPM2InputKernelHIPImpl<true>;

REGISTER_OP(CPM2Input).frame_input("frame").frame_output("cpm2_input").protobuf_name("CPM2Args");

REGISTER_KERNEL(CPM2Input, CPM2InputKernelHIP).device(DeviceType::GPU).batch().num_devices(1);

REGISTER_KERNEL(CPM2Input, CPM2InputKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);
}
