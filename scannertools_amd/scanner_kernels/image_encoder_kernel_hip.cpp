// ImageEncoder op for Scanner on MI355X: the counterpart of ImageDecoder.
//
// Scanner's own stdlib has an ImageEncoder (a cv::imencode wrapper on the CPU); it is not part of the reference tree, so the
// declaration here is this library's: frame_input("frame") -> output("img"), protobuf_name("ImageEncoderArgs"), `frame` a
// U8 frame with 3 channels in R, G, B order, `img` the bytes of one baseline JPEG -- what ImageDecoder's `img` column reads.
// ImageEncoderArgs { int32 quality = 1; string subsampling = 2; Restart restart = 3; }: quality 0 or absent means 95, an empty
// subsampling means "4:2:0".  Those are cv::imencode's defaults for JPEG (IMWRITE_JPEG_QUALITY 95, 4:2:0 sampling) as restated
// from OpenCV's documentation; OpenCV is not available to check them against, so they are unpinned.  restart: MCU_ROW (0 or
// absent) writes one restart interval per MCU row, NONE (1) no DRI segment and no RSTn markers -- the stream cv::imencode,
// Pillow and cjpeg write by default; any other value fails validate().  optimize = 4 (a varint; declared as `bool optimize = 4`
// in ImageEncoderArgsWithRestart): 1 writes each frame with Huffman tables built on the device from its own symbol counts
// (libjpeg's optimize_coding); 0 or absent the Annex K tables; any other value fails validate().
// format = 5 and png_filter = 6 (varints; declared in ImageEncoderArgsWithFormat): format JPEG (0 or absent) is all of the above;
// PNG (1) takes U8 frames of 1, 3 or 4 channels and writes lossless PNG streams through st_png_encode_batch / st_png_encode_fetch
// (DESIGN.md 4.18), filtered as png_filter says: ADAPTIVE (0 or absent), NONE (1), SUB (2), UP (3), AVERAGE (4), PAETH (5).  With
// PNG the JPEG-only fields are still checked as above and otherwise ignored; any other format or png_filter fails validate().
//
// One st_jpeg_encode_batch_opt() call per execute(): colour conversion, downsampling, forward DCT, quantisation and Huffman coding
// run in HIP kernels (include/scannertools_hip.h), the streams come back in one copy of exactly their bytes
// (st_jpeg_encode_fetch).  A stream is byte for byte what libjpeg writes at the same settings with one restart interval per
// MCU row, or with restart = NONE with none at all.  Registered twice like the other classes: DeviceType::GPU reads device frames, the staged DeviceType::CPU form
// uploads host frames first; both are batched.  No CPU fallback: without a GPU validate() fails.
#include "scanner/api/kernel.h"
#include "scanner/api/op.h"
#include "scanner/util/hip.h"
#include "scanner/util/memory.h"
#include "proto_lite.h"
#include "scannertools_hip.h"
#include "kernel_core.h"

namespace scanner {
namespace {
// false: not a message.  quality: 0 when the field is absent; subsampling: empty when absent; restart: 0 (MCU_ROW) when absent
// optimize: 0 when absent
bool parse_image_encoder_args(const std::vector<u8>& args, int* quality, std::string* subsampling, long long* restart, long long* optimize,
                              long long* format, long long* png_filter) {
  std::vector<proto_lite::Field> fields;
  *quality = 0;
  *restart = 0;
  *optimize = 0;
  *format = 0;
  *png_filter = 0;
  subsampling->clear();
  if (!proto_lite::parse(args.data(), args.size(), &fields)) return false;
  for (auto& f : fields) {
    if (f.number == 1 && f.wire == 0) *quality = (int)(int64_t)f.value;
    if (f.number == 2 && f.wire == 2) *subsampling = f.bytes;
    if (f.number == 3 && f.wire == 0) *restart = (long long)(int64_t)f.value;
    if (f.number == 4 && f.wire == 0) *optimize = (long long)(int64_t)f.value;
    if (f.number == 5 && f.wire == 0) *format = (long long)(int64_t)f.value;
    if (f.number == 6 && f.wire == 0) *png_filter = (long long)(int64_t)f.value;
  }
  return true;
}
}  // namespace

template <bool STAGED>
class ImageEncoderKernelHIPImpl : public BatchedKernel {
 public:
  ImageEncoderKernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    std::string sub;
    long long restart = 0, optimize = 0, format = 0, png_filter = 0;
    if (!parse_image_encoder_args(config.args, &quality_, &sub, &restart, &optimize, &format, &png_filter)) {
      RESULT_ERROR(&core_.valid, "ImageEncoder: could not parse ImageEncoderArgs");
      return;
    }
    if (quality_ == 0) quality_ = 95;
    if (quality_ < 1 || quality_ > 100) {
      RESULT_ERROR(&core_.valid, "ImageEncoder: quality %d is outside 1..100", quality_);
      return;
    }
    if (sub.empty() || sub == "4:2:0") { h_samp_ = 2; v_samp_ = 2; }
    else if (sub == "4:2:2") { h_samp_ = 2; v_samp_ = 1; }
    else if (sub == "4:4:4") { h_samp_ = 1; v_samp_ = 1; }
    else {
      RESULT_ERROR(&core_.valid, "ImageEncoder: subsampling \"%s\" is not supported (4:4:4, 4:2:2 or 4:2:0)", sub.c_str());
      return;
    }
    if (restart != ST_JPEG_RESTART_ROW && restart != ST_JPEG_RESTART_NONE) {
      RESULT_ERROR(&core_.valid, "ImageEncoder: restart %lld is not supported (MCU_ROW or NONE)", restart);
      return;
    }
    restart_ = (int)restart;
    if (optimize != 0 && optimize != 1) {
      RESULT_ERROR(&core_.valid, "ImageEncoder: optimize %lld is not supported (0 or 1)", optimize);
      return;
    }
    optimize_ = (int)optimize;
    if (format != 0 && format != 1) {
      RESULT_ERROR(&core_.valid, "ImageEncoder: format %lld is not supported (JPEG or PNG)", format);
      return;
    }
    png_ = format == 1;
    if (png_filter < 0 || png_filter > 5) {
      RESULT_ERROR(&core_.valid, "ImageEncoder: png_filter %lld is not supported (ADAPTIVE, NONE, SUB, UP, AVERAGE or PAETH)", png_filter);
      return;
    }
    // the message's ADAPTIVE is 0 so that an absent field means it; the library's filter types are PNG's, ADAPTIVE after them
    png_filter_ = png_filter == 0 ? ST_PNG_FILTER_ADAPTIVE : (int)png_filter - 1;
    core_.open("ImageEncoderKernelHIP");
  }
  void validate(Result* result) override { core_.validate(result); }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& frame_col = input_columns[0];
    const i32 n = (i32)num_rows(frame_col);
    if (n == 0) return;
    const Frame* first = frame_col[0].as_const_frame();
    const FrameInfo info = first->as_frame_info();
    for (i32 i = 0; i < n; ++i) {
      const Frame* frame = frame_col[i].as_const_frame();
      const int ch = frame->channels();
      LOG_IF(FATAL, frame->type != FrameType::U8 || (png_ ? ch != 1 && ch != 3 && ch != 4 : ch != 3))
          << "ImageEncoder: row " << i << " of the batch is not a U8 frame with " << (png_ ? "1, 3 or 4" : "3") << " channels (" << ch << " channel(s))";
    }
    check_batch_shape(frame_col, info, "ImageEncoder");
    const int h = info.height(), w = info.width();
    const size_t frame_bytes = info.size();
    if (STAGED) {
      const size_t stride = DeviceStage::align(frame_bytes);
      u8* dev = stage_.reserve(stride * n);
      stage_.upload_frames(dev, stride, frame_col, frame_bytes);
      strided_ptrs(src_, n, dev, stride);
    } else {
      input_ptrs(src_, frame_col);
    }
    st_ctx* ctx = core_.ctx;
    if (png_) ST_CHECK(ctx, st_png_encode_batch(ctx, src_.data(), n, h, w, info.channels(), png_filter_));
    else ST_CHECK(ctx, st_jpeg_encode_batch_opt(ctx, src_.data(), n, h, w, quality_, h_samp_, v_samp_, restart_, optimize_));
    sizes_.assign(n, 0);
    const auto fetch = png_ ? st_png_encode_fetch : st_jpeg_encode_fetch;
    ST_CHECK(ctx, fetch(ctx, nullptr, sizes_.data(), 0));   // the sizes alone
    size_t total = 0, most = 0;
    for (i32 i = 0; i < n; ++i) {
      total += sizes_[i];
      most = std::max(most, sizes_[i]);
    }
    // the fetch hands every stream a buffer of one capacity: rows of the longest stream's size
    bytes_.resize(most * (size_t)n);
    strided_ptrs(dst_, n, bytes_.data(), most);
    ST_CHECK(ctx, fetch(ctx, dst_.data(), sizes_.data(), most));
    for (i32 i = 0; i < n; ++i) {
      u8* buffer = new_buffer(core_.device, sizes_[i]);
      memcpy_buffer(buffer, core_.device, dst_[i], CPU_DEVICE, sizes_[i]);
      insert_element(output_columns[0], buffer, sizes_[i]);
    }
  }

 private:
  KernelCore core_;
  DeviceStage stage_;   // staged: the frames
  int quality_ = 95, h_samp_ = 2, v_samp_ = 2, restart_ = ST_JPEG_RESTART_ROW, optimize_ = 0, png_filter_ = ST_PNG_FILTER_ADAPTIVE;
  bool png_ = false;
  std::vector<const uint8_t*> src_;
  std::vector<uint8_t*> dst_;
  std::vector<size_t> sizes_;
  std::vector<u8> bytes_;
};

using ImageEncoderKernelHIP = ImageEncoderKernelHIPImpl<false>;
using ImageEncoderKernelHIPStaged = ImageEncoderKernelHIPImpl<true>;

REGISTER_OP(ImageEncoder).frame_input("frame").output("img").protobuf_name("ImageEncoderArgs");

REGISTER_KERNEL(ImageEncoder, ImageEncoderKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);

REGISTER_KERNEL(ImageEncoder, ImageEncoderKernelHIP).device(DeviceType::GPU).batch().num_devices(1);
}  // namespace scanner
