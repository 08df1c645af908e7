// The kernel class behind the Caffe and Facenet ops for Scanner on MI355X: a Caffe model's forward pass.
//
// Drop-in for the reference's kernels
//   CaffeKernel    /root/reference/scannertools_caffe/scannertools_caffe_cpp/caffe_kernel.cpp:226-420 (caffe_kernel_cpu.cpp,
//                  caffe_kernel_gpu.cpp: the registrations)
//   FacenetKernel  /root/reference/scannertools_caffe/scannertools_caffe_cpp/facenet_kernel.cpp:6-46
// Same arguments: CaffeArgs{net_descriptor = 1, batch_size = 2}; of NetDescriptor (scannertools_caffe.proto:5-26) model_path (1),
// model_weights_path (2), input_layer_names (3), output_layer_names (4), input_width / input_height (5 / 6),
// preserve_aspect_ratio (12), transpose (13), pad_mod (14) are used; uses_python (15) is refused.  Facenet takes FacenetArgs and
// unwraps caffe_args (1); both are read by caffe_args.h.  The reference hands both files to Caffe; here the forward pass is
// caffe_net.h (a plan over the C-ABI layer calls).  Input frames are planar (C, H, W) float32 (CaffeInput's and FacenetInput's
// output), taken batch_size at a time (caffe_kernel.cpp:355-361; 0: the whole call); the output is one FrameInfo(shape[1],
// shape[2] or 1, shape[3] or 1, F32) frame per input frame, the output blob's item as Caffe lays it out (:397-400).
// The input blob's size follows CaffeKernel::new_frame_info() (:284-333) with two readings of proto3's defaults: input_width 0
// and pad_mod 0 mean "not set", as -1 does (the reference compares with -1 only and would then size the blob 0 x 0 or divide by
// zero).  The frames are copied into the blob as they are (:372-376), so the blob must hold exactly a frame's values: anything
// else is fatal here where the reference reads past the frame.  Facenet's blob is (C, shape[1], shape[2]) of the frame
// (facenet_kernel.cpp:11-19): FacenetInput's W x H planes.
#pragma once
#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "caffe_args.h"
#include "caffe_net.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {

template <bool STAGED, bool FACENET>
class CaffeKernelHIPImpl : public BatchedKernel, public VideoKernel {
 public:
  CaffeKernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    const char* op = FACENET ? "Facenet" : "Caffe";
    std::vector<proto_lite::Field> top;   // FacenetArgs' own scalars are FacenetInput's and FacenetOutput's
    const bool parsed = FACENET ? parse_wrapped_caffe_args(config.args.data(), config.args.size(), &args_, &top)
                                : parse_caffe_args(config.args.data(), config.args.size(), &args_);
    if (!parsed) {
      RESULT_ERROR(&core_.valid, "Could not parse %s", FACENET ? "FacenetArgs" : "CaffeArgs");
      return;
    }
    std::string probe;
    if (args_.uses_python) {
      RESULT_ERROR(&core_.valid, "%s: net_descriptor.uses_python is set; Python layers are not implemented", op);
    } else if (!caffe_files::read_file(args_.model_path, &probe)) {
      RESULT_ERROR(&core_.valid, "Model path %s does not exist.", args_.model_path.c_str());            // caffe_kernel.cpp:238-242
    } else if (!caffe_files::read_file(args_.model_weights_path, &probe)) {
      RESULT_ERROR(&core_.valid, "Model weights path %s does not exist.", args_.model_weights_path.c_str());   // :243-247
    } else if (args_.input_layer_names.empty()) {
      RESULT_ERROR(&core_.valid, "%s: net_descriptor.input_layer_names is empty", op);
    } else if (args_.output_layer_names.size() != config.output_columns.size()) {
      RESULT_ERROR(&core_.valid, "# output columns in net descriptor (%lu) does not match number of output columns registered for op (%lu)",   // :265-276
                   (unsigned long)args_.output_layer_names.size(), (unsigned long)config.output_columns.size());
    } else if (args_.batch_size < 0) {
      RESULT_ERROR(&core_.valid, "%s: batch_size must not be negative, got %d", op, args_.batch_size);
    } else {
      probe.clear();
      std::string err;
      if (!net_.load(args_.model_path, args_.model_weights_path, args_.input_layer_names[0], args_.output_layer_names[0], &err))
        RESULT_ERROR(&core_.valid, "%s: %s", op, err.c_str());
      else core_.open(FACENET ? "FacenetKernelHIP" : "CaffeKernelHIP");
    }
  }
  ~CaffeKernelHIPImpl() {
    (void)hipSetDevice(core_.gpu);  // the network's buffers are freed by its destructor, on their device
  }
  void validate(Result* result) override { core_.validate(result); }

  void new_frame_info() override {
    const char* op = FACENET ? "Facenet" : "Caffe";
    LOG_IF(FATAL, frame_info_.type != FrameType::F32) << op << " expects planar (C, H, W) F32 frames";
    const i32 frame_height = frame_info_.shape[1], frame_width = frame_info_.shape[2];
    i32 width = frame_width, height = frame_height;
    if (!FACENET) {
      // caffe_kernel.cpp:299-327
      const bool has_w = args_.input_width != -1 && args_.input_width != 0, has_h = args_.input_height != -1 && args_.input_height != 0;
      if (args_.transpose) { width = frame_height; height = frame_width; }
      if (args_.preserve_aspect_ratio) {
        if (has_w) {
          width = args_.input_width;
          const f32 scale = static_cast<f32>(args_.input_width) / width;
          width = width * scale;
          height = height * scale;
        } else if (has_h) {
          const f32 scale = static_cast<f32>(args_.input_height) / height;
          width = width * scale;
          height = height * scale;
        }
      } else if (has_w) {
        width = args_.input_width;
        height = args_.input_height;
      }
      if (args_.pad_mod != -1 && args_.pad_mod != 0) {
        const i32 pad = args_.pad_mod;
        width += (width % pad) ? pad - (width % pad) : 0;
        height += (height % pad) ? pad - (height % pad) : 0;
      }
    }
    LOG_IF(FATAL, width <= 0 || height <= 0 || (long long)width * height != (long long)frame_width * frame_height)
        << op << ": the input blob is " << height << " x " << width << ", the frames are " << frame_height << " x " << frame_width
        << ": a frame does not fill the blob";
    HIP_CHECK(hipSetDevice(core_.gpu));
    std::string err;
    LOG_IF(FATAL, !net_.prepare(core_.ctx, frame_info_.shape[0], height, width, &err)) << op << ": " << err;
    const caffe_net::Shape& s = net_.plan().out_shape;
    out_info_ = FrameInfo(s.c, s.h, s.w, FrameType::F32);   // caffe_kernel.cpp:397-400
  }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& in_col = input_columns[0];
    const i32 n = (i32)num_rows(in_col);
    if (n == 0) return;
    check_frame(core_.device, in_col[0]);
    check_batch_shape(in_col, frame_info_, FACENET ? "Facenet" : "Caffe");
    HIP_CHECK(hipSetDevice(core_.gpu));
    std::vector<Frame*> outs = new_frames(core_.device, out_info_, n);
    const size_t in_bytes = frame_info_.size(), out_bytes = out_info_.size();
    if (STAGED) {
      // device layout: [n inputs][n outputs]
      const size_t is = DeviceStage::align(in_bytes), os = DeviceStage::align(out_bytes);
      u8* dev = stage_.reserve((is + os) * n);
      stage_.upload_frames(dev, is, in_col, in_bytes);
      strided_ptrs(src_, n, dev, is);
      strided_ptrs(dst_, n, dev + is * n, os);
    } else {
      input_ptrs(src_, in_col);
      output_ptrs(dst_, outs);
    }
    const i32 batch = args_.batch_size > 0 ? args_.batch_size : n;   // caffe_kernel.cpp:354-361
    for (i32 frame = 0; frame < n; frame += batch) {
      const i32 count = std::min(n - frame, batch);
      std::string err;
      const auto net_start = now();  // caffe_kernel.cpp:381
      LOG_IF(FATAL, !net_.forward(core_.ctx, src_.data() + frame, count, dst_.data() + frame, &err)) << (FACENET ? "Facenet: " : "Caffe: ") << err;
      core_.sync();
      // complete on the device (the reference notes that its interval needs a synchronisation to mean anything, :384-387)
      if (profiler_) profiler_->add_interval("caffe:net", net_start, now());
    }
    if (STAGED)
      for (i32 i = 0; i < n; ++i) stage_.download(outs[i]->data, (const u8*)dst_[i], out_bytes);
    for (i32 i = 0; i < n; ++i) insert_frame(output_columns[0], outs[i]);
  }

 private:
  KernelCore core_;
  DeviceStage stage_;
  CaffeArgsLite args_;
  caffe_net::Net net_;
  FrameInfo out_info_;
  std::vector<const float*> src_;
  std::vector<float*> dst_;
};

}  // namespace scanner
