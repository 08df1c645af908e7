// SharpnessBBoxCPP op for Scanner on MI355X.
//
// Drop-in for the legacy op library's kernel (libimgproc_op.so)
//   SharpnessBBoxKernel  /root/reference/scannertools/scannertools/old/cpp_ops/imgproc.cpp:177-234
// Same op declaration (imgproc.cpp:272-276: frame_input("frame"), input("bboxes") -> output("sharpness_bbox"),
// protobuf_name("ImgProcArgs")), same elements: `bboxes` is Scanner's serialised proto vector (u64 count, then per box a u64
// byte length and a BoundingBox message), `sharpness_bbox` one 4-byte float per box, a row without boxes an element of zero
// bytes (imgproc.cpp:227-228).  ImgProcArgs is parsed and ignored, as the reference does.  The reference registers the op on
// DeviceType::CPU only; here the CPU registration stages host frames through the GPU and a DeviceType::GPU registration reads
// frames that are already on the device; the bboxes column is read on the host in both.  Both are batched: the per-box
// cv::resize / cv::Laplacian / cv::meanStdDev calls of every row of an execute() become ONE st_bbox_sharpness_u8c3_* launch
// (include/scannertools_hip.h; contract and deviations: csrc/st_framestats.hip).
//
// BoundingBox is Scanner's message (scanner/types.proto), which is not part of the reference tree: the field numbers below
// (float x1 = 1, y1 = 2, x2 = 3, y2 = 4; score = 5 and further fields follow) are stated from knowledge of that file and have
// not been checked against it.  Fields other than 1..4 are skipped by wire type; proto3 omits a field that is 0.
//
// Where the reference is undefined this fails instead, before anything is launched: a box whose truncated coordinates do
// not satisfy 0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h (the reference trips a CV_Assert inside cv::Mat's ROI constructor), a
// coordinate that is not finite or does not fit an int32, and truncated or over-long bboxes bytes.
#include <cmath>
#include <cstdio>

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

// (int)coordinate as the reference truncates it (imgproc.cpp:205-208); false if it is not finite or outside int32
bool truncate_coord(float v, int32_t* out) {
  if (!std::isfinite(v) || v < -2147483648.0f || v >= 2147483648.0f) return false;
  *out = (int32_t)v;
  return true;
}

// One bboxes element -> records {frame, x1, y1, x2, y2} appended to `boxes`; returns an empty string, or what is wrong
std::string parse_bboxes(const u8* p, size_t size, int32_t frame, int h, int w, std::vector<int32_t>* boxes, size_t* count) {
  char msg[160];
  uint64_t m;
  if (size < 8) return "bboxes element shorter than its u64 count";
  memcpy(&m, p, 8);
  size_t off = 8;
  if (m > (size - off) / 8) return "bboxes element shorter than its count says";
  for (uint64_t i = 0; i < m; ++i) {
    uint64_t len;
    if (size - off < 8) return "bboxes element ends inside a length";
    memcpy(&len, p + off, 8);
    off += 8;
    if (len > size - off) {
      snprintf(msg, sizeof msg, "box %llu: bboxes element ends inside the message", (unsigned long long)i);
      return msg;
    }
    std::vector<proto_lite::Field> fields;
    if (!proto_lite::parse(p + off, (size_t)len, &fields)) {
      snprintf(msg, sizeof msg, "box %llu: malformed BoundingBox message", (unsigned long long)i);
      return msg;
    }
    off += (size_t)len;
    float c[4] = {0.f, 0.f, 0.f, 0.f};   // x1, y1, x2, y2; absent = 0
    for (const auto& f : fields)
      if (f.number >= 1 && f.number <= 4) {
        if (f.wire != 5) {
          snprintf(msg, sizeof msg, "box %llu: coordinate field %u is not a float", (unsigned long long)i, f.number);
          return msg;
        }
        c[f.number - 1] = proto_lite::as_float(f);
      }
    int32_t t[4];
    for (int k = 0; k < 4; ++k)
      if (!truncate_coord(c[k], &t[k])) {
        snprintf(msg, sizeof msg, "box %llu: a coordinate is not finite or does not fit an int32", (unsigned long long)i);
        return msg;
      }
    if (!(0 <= t[0] && t[0] < t[2] && t[2] <= w && 0 <= t[1] && t[1] < t[3] && t[3] <= h)) {
      snprintf(msg, sizeof msg, "box %llu: x %d..%d, y %d..%d is empty or not inside the %dx%d frame", (unsigned long long)i, t[0], t[2],
               t[1], t[3], w, h);
      return msg;
    }
    const int32_t rec[5] = {frame, t[0], t[1], t[2], t[3]};
    boxes->insert(boxes->end(), rec, rec + 5);
  }
  if (off != size) return "bboxes element is longer than its boxes";
  *count = (size_t)m;
  return "";
}
}  // namespace

// STAGED: registered on DeviceType::CPU (host frames uploaded, host elements out); otherwise DeviceType::GPU (device frames,
// device elements).
template <bool STAGED>
class SharpnessBBoxKernelHIPImpl : public BatchedKernel, public VideoKernel {
 public:
  SharpnessBBoxKernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    if (!parse_imgproc_args(config.args)) RESULT_ERROR(&core_.valid, "SharpnessBBoxCPP: could not parse ImgProcArgs");
    else core_.open("SharpnessBBoxKernelHIP");
  }
  void validate(Result* result) override { core_.validate(result); }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    auto& bbox_col = input_columns[1];
    const i32 n = (i32)num_rows(frame_col);
    if (n == 0) return;
    check_frame(core_.device, frame_col[0]);
    LOG_IF(FATAL, frame_info_.channels() != 3 || frame_info_.type != FrameType::U8) << "SharpnessBBoxCPP expects U8 frames with 3 channels";
    check_batch_shape(frame_col, frame_info_, "SharpnessBBoxCPP");
    const i32 h = frame_info_.height(), w = frame_info_.width();
    // every box of every row is parsed and checked before anything is uploaded or launched
    boxes_.clear();
    counts_.assign(n, 0);
    for (i32 i = 0; i < n; ++i) {
      const std::string err = parse_bboxes(bbox_col[i].buffer, bbox_col[i].size, i, h, w, &boxes_, &counts_[i]);
      LOG_IF(FATAL, !err.empty()) << "SharpnessBBoxCPP: row " << i << " of the batch: " << err;
    }
    const size_t m = boxes_.size() / 5;
    // one block for the whole batch, element i a slice of 4 * m_i bytes; 4 bytes of slack keep a trailing empty element
    // inside the block
    const size_t out_bytes = sizeof(float) * m;
    u8* output_block = new_block_buffer(core_.device, out_bytes + sizeof(float), n);
    st_ctx* ctx = core_.ctx;
    if (m > 0) {
      if (STAGED) {
        const size_t frame_bytes = frame_info_.size(), stride = DeviceStage::align(frame_bytes);
        u8* dev = stage_.reserve(stride * n + out_bytes);   // device layout: [n frames][m results]
        stage_.upload_frames(dev, stride, frame_col, frame_bytes);
        float* out = (float*)(dev + stride * n);
        ST_CHECK(ctx, st_bbox_sharpness_u8c3_strided(ctx, dev, stride, n, h, w, boxes_.data(), (int64_t)m, ST_FS_SHARPNESS_CPP, out));
        core_.sync();
        stage_.download(output_block, (const u8*)out, out_bytes);
      } else {
        input_ptrs(frames_, frame_col);
        ST_CHECK(ctx, st_bbox_sharpness_u8c3_batch(ctx, frames_.data(), n, h, w, boxes_.data(), (int64_t)m, ST_FS_SHARPNESS_CPP, output_block));
        core_.sync();  // the engine may read the elements from another stream
      }
    }
    size_t first = 0;
    for (i32 i = 0; i < n; ++i) {
      insert_element(output_columns[0], output_block + sizeof(float) * first, sizeof(float) * counts_[i]);
      first += counts_[i];
    }
  }

 private:
  KernelCore core_;
  DeviceStage stage_;   // staged: frames + results
  std::vector<const uint8_t*> frames_;
  std::vector<int32_t> boxes_;
  std::vector<size_t> counts_;
};

typedef SharpnessBBoxKernelHIPImpl<false> SharpnessBBoxKernelHIP;
typedef SharpnessBBoxKernelHIPImpl<true> SharpnessBBoxKernelHIPStaged;

REGISTER_OP(SharpnessBBoxCPP).frame_input("frame").input("bboxes").output("sharpness_bbox").protobuf_name("ImgProcArgs");
REGISTER_KERNEL(SharpnessBBoxCPP, SharpnessBBoxKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);
REGISTER_KERNEL(SharpnessBBoxCPP, SharpnessBBoxKernelHIP).device(DeviceType::GPU).batch().num_devices(1);
}  // namespace scanner
