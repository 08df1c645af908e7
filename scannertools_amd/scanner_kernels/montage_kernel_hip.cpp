// Montage op for Scanner on MI355X.
//
// Drop-in for the reference's kernels
//   MontageKernel     /root/reference/scannertools/scannertools_cpp/imgproc/montage_kernel_cpu.cpp
//   MontageKernelGPU  /root/reference/scannertools/scannertools_cpp/imgproc/montage_kernel_gpu.cpp
// Same op declaration (frame_input("frame") -> frame_output("montage"), unbounded_state(), protobuf_name("MontageArgs")),
// same arguments (MontageArgs{num_frames = 1, target_width = 4, frames_per_row = 6}, scannertools_imgproc.proto) and the
// same state machine: new_frame_info() derives the canvas geometry (st_montage_geometry) and calls reset(), which starts a
// fresh zeroed canvas; frame k of the stream goes to tile (k % frames_per_row, k / frames_per_row) through an INTER_LINEAR
// resize; the row of frame num_frames - 1 carries the canvas, every other row an unspecified frame of the canvas's shape.
// The reference's per-frame cvc::resize becomes ONE st_montage_u8c3_batch() launch per execute(), and the non-final rows
// share one ref-counted canvas-sized buffer per frame geometry instead of an allocation each (1 000 keyframes at 240 px,
// eight per row: 97 MB instead of 97 GB).
#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "proto_lite.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {
namespace {
struct MontageArgsLite {
  i64 num_frames = 0;
  i32 target_width = 0, frames_per_row = 0;
};

bool parse_montage_args(const std::vector<u8>& args, MontageArgsLite* out) {
  std::vector<proto_lite::Field> fields;
  if (!proto_lite::parse(args.data(), args.size(), &fields)) return false;
  *out = MontageArgsLite();
  for (auto& f : fields) {
    if (f.number == 1 && f.wire == 0) out->num_frames = (i64)f.value;
    if (f.number == 4 && f.wire == 0) out->target_width = (i32)f.value;
    if (f.number == 6 && f.wire == 0) out->frames_per_row = (i32)f.value;
  }
  return true;
}
}  // namespace

// STAGED: registered on DeviceType::CPU -- host frames go up through stage.h, the canvas lives on the device and comes
// back to a host buffer for the row that carries it.
template <bool STAGED>
class MontageKernelHIPImpl : public BatchedKernel, public VideoKernel {
 public:
  MontageKernelHIPImpl(const KernelConfig& config)
    : BatchedKernel(config), core_(config, STAGED), canvas_device_{DeviceType::GPU, core_.gpu} {
    if (!parse_montage_args(config.args, &args_)) {
      RESULT_ERROR(&core_.valid, "Montage: could not parse MontageArgs");
    } else if (args_.num_frames < 1) {
      RESULT_ERROR(&core_.valid, "Montage: num_frames must be at least 1 (got %lld)", (long long)args_.num_frames);
    } else if (args_.frames_per_row < 1) {
      RESULT_ERROR(&core_.valid, "Montage: frames_per_row must be at least 1 (got %d)", args_.frames_per_row);
    } else if (args_.target_width < 1) {
      RESULT_ERROR(&core_.valid, "Montage: target_width must be at least 1 (got %d)", args_.target_width);
    } else if (core_.open("MontageKernelHIP") && STAGED) {
      core_.bind(&pipe_);
    }
  }
  ~MontageKernelHIPImpl() {
    // every execute() ends synchronised, so an unfinished canvas has no work in flight
    if (canvas_) delete_buffer(canvas_device_, canvas_);
    if (placeholder_) delete_buffer(core_.device, placeholder_);  // the rows handed out keep their own references
  }
  void validate(Result* result) override { core_.validate(result); }

  // a fresh zeroed canvas; nothing before the first frame has fixed the geometry
  void reset() override {
    if (montage_w_ == 0) return;
    if (canvas_) delete_buffer(canvas_device_, canvas_);
    canvas_ = new_buffer(canvas_device_, canvas_bytes());
    ST_CHECK(core_.ctx, st_montage_clear(core_.ctx, canvas_, montage_h_, montage_w_));
    frames_seen_ = 0;
  }

  void new_frame_info() override {
    const bool ok = st_montage_geometry(frame_info_.height(), frame_info_.width(), args_.num_frames, args_.target_width,
                                        args_.frames_per_row, &target_h_, &montage_h_, &montage_w_) == ST_OK;
    LOG_IF(FATAL, !ok) << "Montage: no canvas for " << frame_info_.width() << "x" << frame_info_.height()
                               << " frames at target_width " << args_.target_width << " (tile height below 1 or canvas too large)";
    LOG_IF(FATAL, montage_h_ > INT32_MAX) << "Montage: a canvas of " << montage_h_ << " rows is taller than a frame can be";
    if (placeholder_) delete_buffer(core_.device, placeholder_);
    placeholder_ = nullptr;
    reset();
  }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    const i32 input_count = (i32)num_rows(frame_col);
    if (input_count == 0) return;
    const Frame* frame = frame_col[0].as_const_frame();
    LOG_IF(FATAL, frame->type != FrameType::U8 || frame->channels() != 3) << "Montage expects U8 frames of 3 channels";
    check_frame(core_.device, frame_col[0]);
    check_batch_shape(frame_col, frame_info_, "Montage");
    LOG_IF(FATAL, canvas_ == nullptr || frames_seen_ + input_count > args_.num_frames)
        << "Montage: row " << frames_seen_ + input_count - 1 << " is beyond num_frames = " << args_.num_frames;

    const i32 fh = frame->height(), fw = frame->width();
    const size_t in_bytes = frame->size();
    const int first_slot = (int)frames_seen_;
    src_.resize(input_count);
    auto launch = [&](const uint8_t* const* src, i32 first, i32 nb) {
      ST_CHECK(core_.ctx, st_montage_u8c3_batch(core_.ctx, src, nb, fh, fw, canvas_, montage_w_, args_.target_width, target_h_,
                                                args_.frames_per_row, first_slot + first));
    };
    frames_seen_ += input_count;
    const bool finished = frames_seen_ == args_.num_frames;
    u8* handed = nullptr;  // the canvas as the last row carries it
    if (STAGED) {
      // the whole batch in one sub-batch: one upload run, then one launch
      const size_t in_stride = DeviceStage::align(in_bytes);
      pipe_.run(input_count, input_count, in_bytes, in_stride,
                [&](i32 i) { return (const u8*)frame_col[i].as_const_frame()->data; },
                [&](u8* dev, i32 first, i32 nb) {
                  for (i32 i = 0; i < nb; ++i) src_[first + i] = dev + in_stride * i;
                  launch(src_.data() + first, first, nb);
                });
      if (finished) {
        handed = new_buffer(core_.device, canvas_bytes());
        HIP_CHECK(hipMemcpyAsync(handed, canvas_, canvas_bytes(), hipMemcpyDeviceToHost, pipe_.compute_stream()));
      }
      pipe_.drain();
      if (finished) {
        delete_buffer(canvas_device_, canvas_);
        canvas_ = nullptr;
      }
    } else {
      input_ptrs(src_, frame_col);
      launch(src_.data(), 0, input_count);
      core_.sync();
      if (finished) {
        handed = canvas_;  // now Scanner's
        canvas_ = nullptr;
      }
    }

    // rows other than the last one of the montage: unspecified contents, all of them references to one buffer the
    // kernel keeps (and holds one reference to) while the frame geometry stays
    FrameInfo info((int)montage_h_, montage_w_, 3, FrameType::U8);
    const i32 n_other = input_count - (finished ? 1 : 0);
    if (n_other > 0) {
      if (!placeholder_) placeholder_ = new_buffer(core_.device, canvas_bytes());
      add_buffer_refs(core_.device, placeholder_, (size_t)n_other);
    }
    for (i32 i = 0; i < input_count; ++i) {
      const bool last = finished && i == input_count - 1;
      insert_frame(output_columns[0], new Frame(info, last ? handed : placeholder_));
    }
  }

 private:
  size_t canvas_bytes() const { return (size_t)montage_h_ * (size_t)montage_w_ * 3; }

  UploadPipeline pipe_;  // before core_: the context leaves the pipeline's stream before the stream is destroyed
  KernelCore core_;
  DeviceHandle canvas_device_;
  MontageArgsLite args_;
  int target_h_ = 0, montage_w_ = 0;
  int64_t montage_h_ = 0;
  u8* canvas_ = nullptr;
  u8* placeholder_ = nullptr;
  i64 frames_seen_ = 0;
  std::vector<const uint8_t*> src_;
};

using MontageKernelHIP = MontageKernelHIPImpl<false>;
using MontageKernelHIPStaged = MontageKernelHIPImpl<true>;

REGISTER_OP(Montage).frame_input("frame").frame_output("montage").unbounded_state().protobuf_name("MontageArgs");

REGISTER_KERNEL(Montage, MontageKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);

REGISTER_KERNEL(Montage, MontageKernelHIP).device(DeviceType::GPU).batch().num_devices(1);
}
