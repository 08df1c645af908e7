// Histogram op for Scanner on MI355X.
//
// Drop-in for the reference's kernels
//   HistogramKernelCPU  /root/reference/scannertools/scannertools_cpp/imgproc/histogram_kernel_cpu.cpp:11-57
//   HistogramKernelGPU  .../histogram_kernel_gpu.cpp:12-82 (OpenCV-CUDA wrapper, --build-cuda only)
// Same op declaration, same element format (3 x BINS int32, channel-major, one element per
// row), same registration shape (.device(GPU).batch().num_devices(1)); the per-frame
// cv::calcHist / cvc::histEven calls are replaced by ONE st_hist_u8c3_batch() call per
// execute(), i.e. one HIP launch for the whole batch.
//
// Extension over the reference (which has no op arguments): the op declares
// protobuf_name("HistogramArgs") -- message HistogramArgs { int32 bins = 1; }
// (scannertools_imgproc_amd.proto beside this file) -- so that sc.ops.Histogram(frame=..., bins=256)
// reaches the kernel through Scanner's ordinary argument path.  Without arguments (every existing
// graph) the bin count is the reference's BINS = 16.
#include <cstring>

#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "proto_lite.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {
namespace {
const i32 BINS = 16;  // histogram_kernel_cpu.cpp:8

// HistogramArgs { int32 bins = 1; }; empty args = the reference's op (16 bins).  false: malformed.
bool parse_histogram_args(const std::vector<u8>& args, i32* bins) {
  *bins = BINS;
  if (args.empty()) return true;
  std::vector<proto_lite::Field> fields;
  if (!proto_lite::parse(args.data(), args.size(), &fields)) return false;
  for (auto& f : fields)
    if (f.number == 1 && f.wire == 0) *bins = (i32)f.value;
  return true;
}
}

class HistogramKernelHIP : public BatchedKernel, public VideoKernel {
 public:
  HistogramKernelHIP(const KernelConfig& config) : BatchedKernel(config), core_(config, false), bins_(BINS) {
    if (!parse_histogram_args(config.args, &bins_)) {
      RESULT_ERROR(&core_.valid, "Could not parse HistogramArgs");
    } else if (bins_ < 1 || bins_ > 256) {
      RESULT_ERROR(&core_.valid, "Histogram bins must be in [1, 256], got %d", bins_);
    } else {
      core_.open("HistogramKernelHIP");
    }
  }
  void validate(Result* result) override { core_.validate(result); }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    i32 input_count = (i32)num_rows(frame_col);
    if (input_count == 0) return;
    check_frame(core_.device, frame_col[0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8)
        << "Histogram expects U8 frames with 3 channels";
    check_batch_shape(frame_col, frame_info_, "Histogram");

    size_t hist_size = bins_ * 3 * sizeof(i32);
    // one device block for the whole batch, one reference per output element
    u8* output_block = new_block_buffer(core_.device, hist_size * input_count, input_count);

    input_ptrs(frames_, frame_col);
    ST_CHECK(core_.ctx, st_hist_u8c3_batch(core_.ctx, frames_.data(), input_count, frame_info_.height(), frame_info_.width(), bins_,
                                           (int32_t*)output_block));
    core_.sync();  // the engine may read the elements from another stream

    for (i32 i = 0; i < input_count; ++i) insert_element(output_columns[0], output_block + i * hist_size, hist_size);
  }

 private:
  KernelCore core_;
  i32 bins_;
  std::vector<const uint8_t*> frames_;
};

// Same op for graphs that keep the reference's default device (CPU): host frames in, host
// elements out (histogram_kernel_cpu.cpp:16-46), computed on the GPU.  The kernel needs 0.3 us per
// 1080p frame and the upload 110 us, so the work is organising the uploads: sub-batches alternate
// between two device slots, uploads run back to back on a copy stream (straight out of Scanner's
// page-locked frame buffers; through a page-locked bounce ring when a buffer is pageable) while the
// compute stream histograms the sub-batch that has just arrived (stage.h: UploadPipeline).
class HistogramKernelHIPStaged : public BatchedKernel, public VideoKernel {
 public:
  HistogramKernelHIPStaged(const KernelConfig& config)
    : BatchedKernel(config), core_(config, true), bins_(BINS), sub_(env_int("SCANNERTOOLS_HIST_SUBBATCH", 8, 1)), out_stage_(core_.gpu) {
    if (!parse_histogram_args(config.args, &bins_)) {
      RESULT_ERROR(&core_.valid, "Could not parse HistogramArgs");
    } else if (bins_ < 1 || bins_ > 256) {
      RESULT_ERROR(&core_.valid, "Histogram bins must be in [1, 256], got %d", bins_);
    } else if (core_.open("HistogramKernelHIPStaged")) {
      core_.bind(&pipe_);
    }
  }
  void validate(Result* result) override { core_.validate(result); }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    i32 input_count = (i32)num_rows(frame_col);
    if (input_count == 0) return;
    check_frame(core_.device, frame_col[0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8)
        << "Histogram expects U8 frames with 3 channels";
    check_batch_shape(frame_col, frame_info_, "Histogram");
    const size_t hist_size = bins_ * 3 * sizeof(i32);
    const size_t frame_bytes = frame_info_.size(), stride = DeviceStage::align(frame_bytes);
    const i32 h = frame_info_.height(), w = frame_info_.width();
    u8* dev_out = out_stage_.reserve(hist_size * input_count);
    pipe_.run(input_count, sub_, frame_bytes, stride,
              [&](i32 i) { return (const u8*)frame_col[i].as_const_frame()->data; },
              [&](u8* dev, i32 first, i32 nb) {
                ST_CHECK(core_.ctx, st_hist_u8c3_strided(core_.ctx, dev, stride, nb, h, w, bins_, (int32_t*)(dev_out + hist_size * first)));
              });
    u8* output_block = new_block_buffer_size(core_.device, hist_size, input_count);
    HIP_CHECK(hipMemcpyAsync(output_block, dev_out, hist_size * input_count, hipMemcpyDeviceToHost, pipe_.compute_stream()));
    pipe_.drain();
    for (i32 i = 0; i < input_count; ++i) insert_element(output_columns[0], output_block + i * hist_size, hist_size);
  }

 private:
  UploadPipeline pipe_;  // before core_: the context leaves the pipeline's stream before the stream is destroyed
  KernelCore core_;
  i32 bins_;
  int sub_;
  DeviceStage out_stage_;
};

REGISTER_OP(Histogram).frame_input("frame").output("histogram", ColumnType::Bytes, "Histogram").protobuf_name("HistogramArgs");

REGISTER_KERNEL(Histogram, HistogramKernelHIPStaged)
    .device(DeviceType::CPU)
    .batch()
    .num_devices(1);

REGISTER_KERNEL(Histogram, HistogramKernelHIP)
    .device(DeviceType::GPU)
    .batch()
    .num_devices(1);
}
