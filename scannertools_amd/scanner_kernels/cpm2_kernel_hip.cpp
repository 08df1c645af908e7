// CPM2 op for Scanner on MI355X (pose path, BASELINE config 5): the network between CPM2Input and CPM2Output.
//
// Drop-in for the reference's kernel
//   CPM2Kernel  /root/reference/scannertools_caffe/scannertools_caffe_cpp/cpm2_kernel.cpp:8-52
// Same op declaration (frame_input("cpm2_input") -> frame_output("cpm2_resized_map"), frame_output("cpm2_joints")),
// same arguments (CPM2Args{caffe_args = 1 {net_descriptor = 1 {model_path = 1, model_weights_path = 2, ...},
// batch_size = 2}, scale = 2}, scannertools_caffe.proto:1-48), registered on DeviceType::GPU and DeviceType::CPU
// with .batch() like the reference.  The reference is a CaffeKernel: it loads prototxt + caffemodel into Caffe, and
// net_config() (cpm2_kernel.cpp:13-29) points the fork's `resize` layer at the network input size.  Here the
// forward pass is pose_net.h (MFMA convolution kernels through the C ABI) followed by st_cpm2_resize_maps and
// st_cpm2_nms; the architecture is the COCO body model's (pose_net.h says where the layer list comes from), the
// weights are read from the caffemodel the arguments name.  Outputs:
//   cpm2_resized_map  FrameInfo(57, H, W, F32): 19 part heat maps, then 38 part-affinity planes, at the network
//                     input size (what cpm2_output_kernel_cpu.cpp:84-88 indexes)
//   cpm2_joints       FrameInfo(18, max_peaks + 1, 3, F32): per part [count, -, -] then (x, y, score) peaks
//                     (cpm2_output_kernel_cpu.cpp:481-499)
#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "caffe_args.h"
#include "pose_net.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {
namespace {
constexpr int kMaxPeaks = 64;           // cpm2_output_kernel_cpu.cpp:760-761 (max_peaks_)
constexpr float kNmsThreshold = 0.05f;  // the model's nms_param ([EXT] pose_deploy_linevec.prototxt)
}  // namespace

template <bool STAGED>
class CPM2KernelHIPImpl : public BatchedKernel, public VideoKernel {
 public:
  CPM2KernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    // CPM2Args.caffe_args.net_descriptor.model_weights_path (and .model_path, the deploy prototxt, when given)
    CaffeArgsLite args;
    std::vector<proto_lite::Field> top;   // CPM2Args.scale is CPM2Input's and CPM2Output's
    if (!parse_wrapped_caffe_args(config.args.data(), config.args.size(), &args, &top)) {
      RESULT_ERROR(&core_.valid, "Could not parse CPM2Args");
      return;
    }
    const std::string &path = args.model_weights_path, &prototxt = args.model_path;
    if (path.empty()) {
      RESULT_ERROR(&core_.valid, "CPM2: CPM2Args.caffe_args.net_descriptor.model_weights_path is empty");
      return;
    }
    if (!core_.open("CPM2KernelHIP")) return;
    if (hipSetDevice(core_.gpu) != hipSuccess) {
      RESULT_ERROR(&core_.valid, "CPM2: hipSetDevice(%d) failed", core_.gpu);
      return;
    }
    std::string err;
    if (!net_.load(path, &err, prototxt)) RESULT_ERROR(&core_.valid, "CPM2: %s", err.c_str());
    for (int c = 0; c < 57; ++c) chan_[c] = c < pose::kHeat ? pose::kOffHeat + c : pose::kOffPaf + (c - pose::kHeat);
  }
  ~CPM2KernelHIPImpl() {
    (void)hipSetDevice(core_.gpu);  // the network's buffers are freed by its destructor, on their device
  }
  void validate(Result* result) override { core_.validate(result); }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& in_col = input_columns[0];
    const i32 n = (i32)num_rows(in_col);
    if (n == 0) return;
    check_frame(core_.device, in_col[0]);
    // the input frame is CPM2Input's: FrameInfo(3, H, W, F32) (cpm2_input_kernel_gpu.cpp:112-113)
    LOG_IF(FATAL, frame_info_.shape[0] != 3 || frame_info_.type != FrameType::F32) << "CPM2 expects planar (3, H, W) F32 frames";
    const int H = frame_info_.shape[1], W = frame_info_.shape[2];
    LOG_IF(FATAL, H % 8 || W % 8) << "CPM2: the network input must be padded to a multiple of 8 (CPM2Input does)";
    check_batch_shape(in_col, frame_info_, "CPM2");
    HIP_CHECK(hipSetDevice(core_.gpu));
    FrameInfo map_info(57, H, W, FrameType::F32), joint_info(pose::kHeat - 1, kMaxPeaks + 1, 3, FrameType::F32);
    std::vector<Frame*> maps = new_frames(core_.device, map_info, n), joints = new_frames(core_.device, joint_info, n);
    const size_t in_bytes = frame_info_.size(), map_bytes = map_info.size(), joint_bytes = joint_info.size();
    if (STAGED) {
      // device layout: [n inputs][n map stacks][n joint tables]
      const size_t is = DeviceStage::align(in_bytes), ms = DeviceStage::align(map_bytes), js = DeviceStage::align(joint_bytes);
      u8* dev = stage_.reserve((is + ms + js) * n);
      stage_.upload_frames(dev, is, in_col, in_bytes);
      strided_ptrs(src_, n, dev, is);
      strided_ptrs(map_ptr_, n, dev + is * n, ms);
      strided_ptrs(joint_ptr_, n, dev + (is + ms) * n, js);
    } else {
      input_ptrs(src_, in_col);
      output_ptrs(map_ptr_, maps);
      output_ptrs(joint_ptr_, joints);
    }
    std::string err;
    const auto net_start = now();  // caffe_kernel.cpp:381
    const float* final_maps = net_.forward(core_.ctx, src_.data(), n, H, W, &err);
    LOG_IF(FATAL, !final_maps) << "CPM2: " << err;
    ST_CHECK(core_.ctx, st_cpm2_resize_maps(core_.ctx, final_maps, n, H / 8, W / 8, pose::kCatPad, chan_, 57, H, W, map_ptr_.data()));
    cmap_ptr_.assign(map_ptr_.begin(), map_ptr_.end());
    ST_CHECK(core_.ctx, st_cpm2_nms(core_.ctx, cmap_ptr_.data(), n, H, W, pose::kHeat - 1, kMaxPeaks, kNmsThreshold, joint_ptr_.data()));
    core_.sync();
    // the network + its resize / nms layers, complete on the device (the reference brackets net->Forward() the same way and
    // notes that the interval is only meaningful with a synchronisation, caffe_kernel.cpp:384-387)
    if (profiler_) profiler_->add_interval("caffe:net", net_start, now());
    if (STAGED)
      for (i32 i = 0; i < n; ++i) {
        stage_.download(maps[i]->data, (const u8*)map_ptr_[i], map_bytes);
        stage_.download(joints[i]->data, (const u8*)joint_ptr_[i], joint_bytes);
      }
    for (i32 i = 0; i < n; ++i) {
      insert_frame(output_columns[0], maps[i]);
      insert_frame(output_columns[1], joints[i]);
    }
  }

 private:
  KernelCore core_;
  DeviceStage stage_;
  pose::Net net_;
  int chan_[57];
  std::vector<const float*> src_, cmap_ptr_;
  std::vector<float*> map_ptr_, joint_ptr_;
};

}  // namespace scanner

// Model-file check without a GPU: number of layers whose weights were found with the architecture's sizes (92 = all),
// or -1 with the reason in `err`.
extern "C" __attribute__((visibility("default"))) int scannertools_caffe_check_model(const char* caffemodel, char* err, size_t err_len) {
  std::string msg;
  const bool ok = caffemodel ? scanner::pose::check_caffemodel(caffemodel, std::string(), &msg) : (msg = "null path", false);
  if (err && err_len) { strncpy(err, msg.c_str(), err_len - 1); err[err_len - 1] = 0; }
  return ok ? (int)scanner::pose::all_layers().size() : -1;
}

// Deploy-description check without a GPU: 92 when the prototxt describes the network the kernels implement and, if
// `caffemodel` is given, the weights of every one of ITS layer names are in that file with the architecture's sizes;
// -1 with the reason in `err`.
extern "C" __attribute__((visibility("default"))) int scannertools_caffe_check_prototxt(const char* prototxt, const char* caffemodel, char* err,
                                                                                        size_t err_len) {
  std::string msg;
  std::vector<std::string> names;
  const bool ok = !prototxt ? (msg = "null path", false)
                  : caffemodel ? scanner::pose::check_caffemodel(caffemodel, prototxt, &msg)
                               : scanner::pose::prototxt_layer_names(prototxt, &names, &msg);
  if (err && err_len) { strncpy(err, msg.c_str(), err_len - 1); err[err_len - 1] = 0; }
  return ok ? (int)scanner::pose::all_layers().size() : -1;
}

namespace scanner {
using CPM2KernelHIP = CPM2KernelHIPImpl<false>;
using CPM2KernelHIPStaged = CPM2KernelHIPImpl<true>;

REGISTER_OP(CPM2).frame_input("cpm2_input").frame_output("cpm2_resized_map").frame_output("cpm2_joints").protobuf_name("CPM2Args");

REGISTER_KERNEL(CPM2, CPM2KernelHIPStaged).device(DeviceType::CPU).num_devices(1).batch();
REGISTER_KERNEL(CPM2, CPM2KernelHIP).device(DeviceType::GPU).num_devices(1).batch();
}
