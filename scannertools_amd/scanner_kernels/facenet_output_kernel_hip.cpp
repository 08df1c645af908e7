// FacenetOutput op for Scanner on MI355X: the Facenet detector's maps become the `bboxes` column.
//
// Drop-in for the reference's kernel
//   FacenetOutputKernel  scannertools_caffe/scannertools_caffe_cpp/facenet_output_kernel_cpu.cpp:11-184
// Same op declaration (:186-190: frame_input("facenet_output"), input("original_frame_info") -> output("bboxes"),
// protobuf_name("FacenetArgs")), same arguments (FacenetArgs{caffe_args = 1, templates_path = 2, scale = 3, threshold = 4},
// scannertools_caffe.proto:38-43: scale, threshold and templates_path are used, caffe_args is parsed and ignored, as in the
// reference), same element: Scanner's serialised proto vector (u64 count, then per box a u64 byte length and a BoundingBox
// message), a frame without boxes the 8-byte count 0.  The reference's triple loop and best_nms per frame are ONE
// st_facenet_output_batch() call for the batch (contract and deviations: include/scannertools_hip.h); the
// kept rows come back in one copy and are serialised here on the host.
// Differences in registration: the reference registers the op on DeviceType::CPU without .batch(); here the CPU
// registration stages host maps through the GPU, a DeviceType::GPU registration reads the Facenet op's device maps where
// they are, and both are batched.
//
// BoundingBox is Scanner's message (scanner/types.proto), which is not part of the reference tree: float x1 = 1, y1 = 2,
// x2 = 3, y2 = 4, score = 5 are stated from knowledge of that file and have not been checked against it (the same numbers
// sharpness_bbox_kernel_hip.cpp reads).  proto3 leaves out a field whose value is 0.
#include <cmath>
#include <cstdio>
#include <fstream>

#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "proto_lite.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {
namespace {
// best_nms(bboxes, 0.1), facenet_output_kernel_cpu.cpp:156
constexpr float kNmsOverlap = 0.1f;
// The "+ 1" of the classic pixel-coordinate overlap formula.  Scanner's util/bbox.cpp is not in the reference tree, so whether
// its best_nms carries it is unpinned; this op's coordinates are normalised to [0, 1], where an offset of 1 would make every
// pair of boxes overlap almost completely (measured: 1-2 boxes kept of 74 - 13 800), so 0 it is.  [EXT] known unpinned.
constexpr float kNmsOffset = 0.0f;

constexpr size_t kTemplateFloats = 25 * 4;

// FacenetArgs: templates_path (2), scale (3), threshold (4); caffe_args (1) only has to parse
bool parse_facenet_output_args(const std::vector<u8>& args, f32* scale, f32* threshold, std::string* templates_path) {
  std::vector<proto_lite::Field> fields, caffe_args;
  *scale = 0.f;
  *threshold = 0.f;
  templates_path->clear();
  if (!proto_lite::parse(args.data(), args.size(), &fields)) return false;
  for (auto& f : fields) {
    if (f.number == 3 && f.wire == 5) *scale = proto_lite::as_float(f);
    if (f.number == 4 && f.wire == 5) *threshold = proto_lite::as_float(f);
    if (f.number == 2 && f.wire == 2) *templates_path = f.bytes;
  }
  return proto_lite::nested(fields, 1, &caffe_args);
}

void put_u64(std::vector<u8>* out, uint64_t v) {
  u8 b[8];
  memcpy(b, &v, 8);
  out->insert(out->end(), b, b + 8);
}

// rows [x1, y1, x2, y2, score] -> one bboxes element
void serialize_boxes(const float* rows, size_t count, std::vector<u8>* out) {
  out->clear();
  put_u64(out, count);
  for (size_t i = 0; i < count; ++i) {
    u8 msg[25];
    size_t len = 0;
    for (int k = 0; k < 5; ++k) {
      const float v = rows[5 * i + k];
      if (v == 0.0f) continue;   // proto3: a default value is not written
      msg[len++] = (u8)(((k + 1) << 3) | 5);
      memcpy(msg + len, &v, 4);
      len += 4;
    }
    put_u64(out, len);
    out->insert(out->end(), msg, msg + len);
  }
}
}  // namespace

// STAGED: registered on DeviceType::CPU (host maps uploaded, host elements out); otherwise DeviceType::GPU (device maps,
// device elements).
template <bool STAGED>
class FacenetOutputKernelHIPImpl : public BatchedKernel, public VideoKernel {
 public:
  FacenetOutputKernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    std::string path;
    if (!parse_facenet_output_args(config.args, &scale_, &threshold_, &path)) {
      RESULT_ERROR(&core_.valid, "Could not parse FacenetArgs");
      return;
    }
    if (!(scale_ > 0.f)) {
      RESULT_ERROR(&core_.valid, "FacenetOutput: scale must be positive, got %f", scale_);
      return;
    }
    if (!std::isfinite(threshold_)) {
      RESULT_ERROR(&core_.valid, "FacenetOutput: threshold must be a finite number, got %f", threshold_);
      return;
    }
    // facenet_output_kernel_cpu.cpp:20-30
    std::ifstream template_file(path, std::ifstream::binary);
    if (!template_file.good()) {
      RESULT_ERROR(&core_.valid, "Could not find template file.");
      return;
    }
    template_file.read(reinterpret_cast<char*>(templates_), sizeof templates_);
    if ((size_t)template_file.gcount() != sizeof templates_) {
      RESULT_ERROR(&core_.valid, "Template file not correct.");
      return;
    }
    core_.open("FacenetOutputKernelHIP");
  }
  void validate(Result* result) override { core_.validate(result); }

  void new_frame_info() override {
    // facenet_output_kernel_cpu.cpp:33-56; frame_info_ is the ORIGINAL frame's (second input column)
    const bool ok = st_facenet_geometry(frame_info_.height(), frame_info_.width(), scale_, &net_input_height_, &net_input_width_) == ST_OK;
    LOG_IF(FATAL, !ok) << "FacenetOutput: frame " << frame_info_.width() << "x" << frame_info_.height() << " at scale " << scale_
                       << " gives an empty network input";
    grid_width_ = (net_input_width_ + 7) / 8;
    grid_height_ = (net_input_height_ + 7) / 8;
  }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    LOG_IF(FATAL, input_columns.size() != 2) << "FacenetOutput takes two input columns";
    auto& frame_col = input_columns[0];
    auto& info_col = input_columns[1];
    const i32 n = (i32)num_rows(frame_col);
    if (n == 0) return;
    for (i32 i = 0; i < n; ++i)
      LOG_IF(FATAL, info_col[i].size < sizeof(FrameInfo)) << "FacenetOutput: row " << i << ": original_frame_info element of " << info_col[i].size
                                                           << " bytes is shorter than a FrameInfo";
    check_frame_info(CPU_DEVICE, info_col[0]);
    const size_t map_bytes = (size_t)125 * grid_width_ * grid_height_ * sizeof(f32);
    for (i32 i = 0; i < n; ++i) {
      const Frame* frame = frame_col[i].as_const_frame();
      LOG_IF(FATAL, frame->type != FrameType::F32) << "FacenetOutput: row " << i << ": the map is not F32";
      LOG_IF(FATAL, frame->size() != map_bytes) << "FacenetOutput: row " << i << ": map of " << frame->size() << " bytes, expected " << map_bytes
                                                << " (125 planes of " << grid_width_ << "x" << grid_height_ << ")";
    }
    if (STAGED) {
      const size_t stride = DeviceStage::align(map_bytes);
      u8* dev = stage_.reserve(stride * n);
      stage_.upload_frames(dev, stride, frame_col, map_bytes);
      maps_.resize(n);
      for (i32 i = 0; i < n; ++i) maps_[i] = (const float*)(dev + stride * i);
    } else {
      input_ptrs(maps_, frame_col);
    }
    st_ctx* ctx = core_.ctx;
    counts_.assign(n, 0);
    ST_CHECK(ctx, st_facenet_output_batch(ctx, maps_.data(), n, frame_info_.height(), frame_info_.width(), scale_, templates_, threshold_,
                                          kNmsOverlap, kNmsOffset, counts_.data()));
    size_t total = 0;
    for (i32 i = 0; i < n; ++i) total += (size_t)counts_[i];
    rows_.resize(5 * total);
    ST_CHECK(ctx, st_facenet_output_fetch(ctx, rows_.data(), (int64_t)total));
    size_t first = 0;
    for (i32 i = 0; i < n; ++i) {
      serialize_boxes(rows_.data() + 5 * first, (size_t)counts_[i], &bytes_);
      first += (size_t)counts_[i];
      u8* buffer = new_buffer(core_.device, bytes_.size());
      memcpy_buffer(buffer, core_.device, bytes_.data(), CPU_DEVICE, bytes_.size());
      insert_element(output_columns[0], buffer, bytes_.size());
    }
  }

 private:
  KernelCore core_;
  DeviceStage stage_;   // staged: the maps
  f32 scale_ = 0.f, threshold_ = 0.f;
  f32 templates_[kTemplateFloats];
  int net_input_width_ = 0, net_input_height_ = 0, grid_width_ = 0, grid_height_ = 0;
  std::vector<const float*> maps_;
  std::vector<int32_t> counts_;
  std::vector<float> rows_;
  std::vector<u8> bytes_;
};

using FacenetOutputKernelHIP = FacenetOutputKernelHIPImpl<false>;
using FacenetOutputKernelHIPStaged = FacenetOutputKernelHIPImpl<true>;

REGISTER_OP(FacenetOutput).frame_input("facenet_output").input("original_frame_info").output("bboxes").protobuf_name("FacenetArgs");

REGISTER_KERNEL(FacenetOutput, FacenetOutputKernelHIP).device(DeviceType::GPU).batch().num_devices(1);

REGISTER_KERNEL(FacenetOutput, FacenetOutputKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);
}  // namespace scanner
