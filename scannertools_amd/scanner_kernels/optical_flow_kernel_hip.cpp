// OpticalFlow op for Scanner on MI355X.
//
// Drop-in for the reference's kernels
//   OpticalFlowKernelCPU  /root/reference/scannertools/scannertools_cpp/imgproc/optical_flow_kernel_cpu.cpp:10-58
//   OpticalFlowKernelGPU  .../optical_flow_kernel_gpu.cpp:12-112 (OpenCV-CUDA wrapper, --build-cuda only)
// Same op declaration (frame in, frame out, stencil {0,1}) and the GPU wrapper's batched-stenciled
// registration.  Semantics follow the CPU kernel: output row i is the Farneback flow FROM stencil
// element 0 TO stencil element 1 of row i with create(3, 0.5, false, 15, 3, 5, 1.2, 0), after
// cv::cvtColor(COLOR_BGR2GRAY) of both frames.  Two defects of the reference GPU wrapper are
// not reproduced: its reversed (later, earlier) argument order (optical_flow_kernel_gpu.cpp:82-87)
// and its assumption that row i's second stencil element is row i+1's first (:53-57) -- every
// row's own window is honoured, and frames shared between windows are recognised by buffer
// address so that their pyramids are built once per execute().
#include <algorithm>
#include <memory>
#include <string>

#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {

namespace {
// every row is a window of two frames of the stream's shape
void check_windows(const std::vector<Elements>& col, const FrameInfo& info) {
  for (auto& window : col) {
    LOG_IF(FATAL, window.size() != 2) << "OpticalFlow needs a 2-element stencil, got " << window.size();
    check_batch_shape(window, info, "OpticalFlow stencil");
  }
}
}  // namespace

class OpticalFlowKernelHIP : public StenciledBatchedKernel, public VideoKernel {
 public:
  OpticalFlowKernelHIP(const KernelConfig& config) : StenciledBatchedKernel(config), core_(config, false) {
    st_fb_params_default(&params_);  // (3, 0.5, false, 15, 3, 5, 1.2, 0): optical_flow_kernel_cpu.cpp:16
    core_.open("OpticalFlowKernelHIP");
  }
  void validate(Result* result) override { core_.validate(result); }

  void new_frame_info() override {
    // scratch is sized for the new geometry on the next call; drop the old one now
    if (core_.ctx) st_ctx_release_workspace(core_.ctx);
  }

  void reset() override {}

  void execute(const StenciledBatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    i32 input_count = (i32)frame_col.size();
    if (input_count == 0) return;
    check_frame(core_.device, frame_col[0][0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8)
        << "OpticalFlow expects U8 frames with 3 channels";
    check_windows(frame_col, frame_info_);
    pair_table(frame_col, 0, input_count, &frames_, &pairs_);

    FrameInfo out_frame_info(frame_info_.height(), frame_info_.width(), 2, FrameType::F32);
    std::vector<Frame*> output_frames = new_frames(core_.device, out_frame_info, input_count);
    output_ptrs(outs_, output_frames);

    ST_CHECK(core_.ctx, st_farneback_pairs(core_.ctx, frames_.data(), (int)frames_.size(), pairs_.data(), input_count,
                                           frame_info_.height(), frame_info_.width(), &params_, outs_.data()));
    core_.sync();

    for (i32 i = 0; i < input_count; ++i) insert_frame(output_columns[0], output_frames[i]);
  }

 private:
  KernelCore core_;
  st_fb_params params_;
  std::vector<const uint8_t*> frames_;
  std::vector<int32_t> pairs_;
  std::vector<float*> outs_;
};

// Same op for graphs that keep the reference's default device (CPU): host frames in, host flow
// frames out (optical_flow_kernel_cpu.cpp:27-43), computed on the GPU.  Registered batched (the
// reference's CPU kernel is not) so that a `batch=` on the op amortises the frames shared by
// consecutive windows; batch 1 reproduces the reference's calling pattern.
//
// The batch is cut into sub-batches that alternate between two lanes (stream + context + device
// staging buffer each): while lane A computes sub-batch i and copies its flow fields back
// (asynchronously, into the Scanner-allocated outputs), the host thread uploads the frames of
// sub-batch i+1 for lane B.  A 1080p flow frame is 16.6 MB going back for 6.2 MB coming in, so
// the path is PCIe-bound; overlapping the three stages is what this structure buys.
class OpticalFlowKernelHIPStaged : public StenciledBatchedKernel, public VideoKernel {
 public:
  OpticalFlowKernelHIPStaged(const KernelConfig& config) : StenciledBatchedKernel(config), core_(config, true) {
    st_fb_params_default(&params_);
    sub_ = env_int("SCANNERTOOLS_FLOW_SUBBATCH", 8, 1, &sub_fixed_);
    for (int l = 0; l < 2 && core_.valid.success(); ++l) {
      lanes_[l].stage.reset(new DeviceStage(core_.gpu));
      if (!core_.open(&lanes_[l].ctx)) break;
      if (hipStreamCreateWithFlags(&lanes_[l].stream, hipStreamNonBlocking) != hipSuccess ||
          st_ctx_set_stream(lanes_[l].ctx, lanes_[l].stream) != ST_OK ||
          hipEventCreateWithFlags(&lanes_[l].up_done, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&lanes_[l].comp_done, hipEventDisableTiming) != hipSuccess)
        RESULT_ERROR(&core_.valid, "cannot create a HIP stream on device %d", core_.gpu);
    }
    // SCANNERTOOLS_FLOW_COPIES=overlap: every lane copies on its own stream (uploads of one lane run beside the other's
    // copy-back); default "serial": ALL copies of both lanes on one stream, so that an upload and a copy-back are never in
    // flight together -- this host's device-to-host copies run at 57 GB/s alone and at 36-38 GB/s beside an upload, and
    // the flow fields going back are 2.7x the frames coming in
    const char* cm = getenv("SCANNERTOOLS_FLOW_COPIES");
    serial_copies_ = !(cm && std::string(cm) == "overlap");
    if (core_.valid.success() && hipStreamCreateWithFlags(&copy_, hipStreamNonBlocking) != hipSuccess)
      RESULT_ERROR(&core_.valid, "cannot create a HIP stream on device %d", core_.gpu);
  }
  ~OpticalFlowKernelHIPStaged() {
    if (copy_) { (void)hipStreamSynchronize(copy_); (void)hipStreamDestroy(copy_); }
    for (auto& l : lanes_) {
      if (l.up_done) (void)hipEventDestroy(l.up_done);
      if (l.comp_done) (void)hipEventDestroy(l.comp_done);
      core_.close(&l.ctx);
      if (l.stream) (void)hipStreamDestroy(l.stream);
    }
  }
  void validate(Result* result) override { core_.validate(result); }
  void new_frame_info() override {
    for (auto& l : lanes_) if (l.ctx) st_ctx_release_workspace(l.ctx);
  }

  void execute(const StenciledBatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    i32 input_count = (i32)frame_col.size();
    if (input_count == 0) return;
    check_frame(core_.device, frame_col[0][0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8)
        << "OpticalFlow expects U8 frames with 3 channels";
    check_windows(frame_col, frame_info_);
    FrameInfo out_info(frame_info_.height(), frame_info_.width(), 2, FrameType::F32);
    const size_t frame_bytes = frame_info_.size(), fstride = DeviceStage::align(frame_bytes);
    const size_t out_bytes = out_info.size(), ostride = DeviceStage::align(out_bytes);
    std::vector<Frame*> output_frames = new_frames(core_.device, out_info, input_count);
    std::vector<u8*> host_outs;
    output_ptrs(host_outs, output_frames);
    HIP_CHECK(hipSetDevice(core_.gpu));

    // Sub-batch size: SCANNERTOOLS_FLOW_SUBBATCH when set; otherwise by bytes -- about 64 MB of frames + flow fields per
    // sub-batch, at least 8 rows (1080p: 8 rows = 180 MB), so that small frames (the legacy pipeline's 426x240: 1.1 MB per
    // row) are not cut into pieces whose fixed costs (two synchronisations, a dozen launches, two copies) outweigh them:
    // 64 rows of 426x240 went from 7.0 k to the rate printed by bench.py's legacy_flow_hist record.  Even split.
    i32 sub = sub_;
    if (!sub_fixed_) {
      const size_t per_row = frame_bytes + out_bytes;
      sub = (i32)std::min<size_t>(64, std::max<size_t>(8, ((size_t)64 << 20) / std::max<size_t>(per_row, 1)));
      const i32 pieces = (input_count + sub - 1) / sub;
      sub = (input_count + pieces - 1) / pieces;
    }
    // copy-back of the sub-batch a lane computed last (serial mode: enqueued on the shared copy stream behind the NEXT
    // sub-batch's upload, so that uploads stay one sub-batch ahead of the compute)
    struct Pending { bool any = false; i32 r0 = 0, nb = 0; std::vector<float*> dev_outs; };
    Pending pending[2];
    auto copy_back = [&](int li) {
      Pending& P = pending[li];
      if (!P.any) return;
      HIP_CHECK(hipStreamWaitEvent(copy_, lanes_[li].comp_done, 0));
      copy_runs(hipMemcpyDeviceToHost, host_outs.data() + P.r0, P.dev_outs.data(), P.nb, out_bytes, copy_);
      P.any = false;
    };
    int lane_idx = 0;
    for (i32 r0 = 0; r0 < input_count; r0 += sub, lane_idx ^= 1) {
      const i32 nb = std::min(sub, input_count - r0);
      Lane& L = lanes_[lane_idx];
      hipStream_t up_stream = serial_copies_ ? copy_ : L.stream;
      // the lane's previous sub-batch (compute + copy-back) must be done before its buffers are reused: own stream in
      // overlap mode; in serial mode its copy-back goes first on the copy stream, and this sub-batch's compute waits for
      // the upload behind it
      if (serial_copies_) copy_back(lane_idx);
      else st_sync(L.ctx);
      // distinct frames of this sub-batch; device layout: [frames][nb flow fields]
      std::vector<const u8*> host_frames, dev_frames;
      std::vector<int32_t> pairs;
      pair_table(frame_col, r0, nb, &host_frames, &pairs);
      u8* dev = L.stage->reserve(fstride * host_frames.size() + ostride * nb);
      strided_ptrs(dev_frames, (i32)host_frames.size(), dev, fstride);
      // One copy per RUN of frames that are adjacent in host memory (Scanner hands out a batch's frames from block
      // allocations) when a frame is a multiple of the staging alignment.
      // (Pageable sources: the call returns when the data is on its way; the other lane keeps computing.)
      copy_runs(hipMemcpyHostToDevice, host_frames.data(), dev_frames.data(), host_frames.size(), frame_bytes, up_stream);
      if (serial_copies_) {
        HIP_CHECK(hipEventRecord(L.up_done, copy_));
        HIP_CHECK(hipStreamWaitEvent(L.stream, L.up_done, 0));
        copy_back(lane_idx ^ 1);  // the other lane's finished sub-batch comes back behind this upload
      }
      std::vector<float*> dev_outs;
      strided_ptrs(dev_outs, nb, dev + fstride * host_frames.size(), ostride);
      ST_CHECK(L.ctx, st_farneback_pairs(L.ctx, dev_frames.data(), (int)dev_frames.size(), pairs.data(), nb,
                                         frame_info_.height(), frame_info_.width(), &params_, dev_outs.data()));
      if (serial_copies_) {
        HIP_CHECK(hipEventRecord(L.comp_done, L.stream));
        pending[lane_idx].any = true; pending[lane_idx].r0 = r0; pending[lane_idx].nb = nb; pending[lane_idx].dev_outs = dev_outs;
        continue;
      }
      // the output frames of a batch are one host block (new_frames) and the staged flows are adjacent on the device
      // whenever a flow field is a multiple of the staging alignment: then the whole sub-batch comes back in ONE copy
      // (16.6 MB copies reach 33 GB/s on this host, a 133 MB copy 57)
      copy_runs(hipMemcpyDeviceToHost, host_outs.data() + r0, dev_outs.data(), nb, out_bytes, L.stream);
    }
    if (serial_copies_) {
      // the last two sub-batches, oldest first
      copy_back(lane_idx);
      copy_back(lane_idx ^ 1);
      HIP_CHECK(hipStreamSynchronize(copy_));
    }
    for (auto& l : lanes_) st_sync(l.ctx);
    for (i32 i = 0; i < input_count; ++i) insert_frame(output_columns[0], output_frames[i]);
  }

 private:
  struct Lane {
    st_ctx* ctx = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t up_done = nullptr, comp_done = nullptr;
    std::unique_ptr<DeviceStage> stage;
  };
  hipStream_t copy_ = nullptr;
  bool serial_copies_ = true;
  KernelCore core_;  // the GPU and the result; the two contexts are the lanes'
  int sub_ = 8;
  bool sub_fixed_ = false;
  Lane lanes_[2];
  st_fb_params params_;
};

REGISTER_OP(OpticalFlow)
    .frame_input("frame")
    .frame_output("flow")
    .stencil({0, 1});

REGISTER_KERNEL(OpticalFlow, OpticalFlowKernelHIP)
    .device(DeviceType::GPU)
    .batch()
    .num_devices(1);

REGISTER_KERNEL(OpticalFlow, OpticalFlowKernelHIPStaged)
    .device(DeviceType::CPU)
    .batch()
    .num_devices(1);
}
