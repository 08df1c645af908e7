// ImageDecoder op for Scanner on MI355X.
//
// Drop-in for the reference's kernels
//   ImageDecoderKernelCPU  /root/reference/scannertools/scannertools_cpp/imgproc/image_decoder_kernel_cpu.cpp:10-58
//   ImageDecoderKernelGPU  /root/reference/scannertools/scannertools_cpp/imgproc/image_decoder_kernel_gpu.cpp
// Same op declaration (input("img") -> frame_output("frame"); the GPU file adds protobuf_name("ImageDecoderArgs")), same
// elements: `img` is the bytes of one encoded image, `frame` the decoded U8 frame in R, G, B order (cv::imdecode(
// IMREAD_UNCHANGED) + COLOR_BGR2RGB, :23-29) or with one channel.  The per-image cv::imdecode calls of the reference's
// 32-thread pool become ONE st_jpeg_decode_batch_scaled() call per execute(), whose scale_denom, entropy mode and opts the
// fields below map to once.  Without them it does what st_jpeg_decode_batch() does: Huffman decoding on host threads,
// everything dense in HIP kernels, bit-exact to libjpeg's defaults (include/scannertools_hip.h).
//
// JPEG only, as the reference's GPU kernel (:78-88 is fatal on PNG and ANY).  ImageDecoderArgs { image_type: PNG = 0 | JPEG = 1
// | ANY = 2 }: JPEG and a message without the field (the reference's CPU kernel takes no arguments at all) are accepted; the
// field present with PNG or ANY fails validate().  (proto3 does not write a field that holds its default, so a PNG request
// serialised by protoc is an empty message and cannot be told from "no arguments": it is accepted, and a PNG stream then
// fails in execute() as any stream that is not a JPEG does.)
//
// ImageDecoderArgs { ..., entropy = 2: HOST = 0 | GPU = 1 | AUTO = 2 } (this build's own field, scannertools_imgproc_amd.proto)
// chooses where the Huffman decoder runs: HOST, and a message without the field, is ST_JPEG_ENTROPY_HOST as above; GPU is
// ST_JPEG_ENTROPY_INTERVAL (st_jpeg_decode_batch_gpu()'s), the Huffman decoder a HIP kernel with one lane per restart interval, and a row without restart
// intervals is then fatal with the row and the cause; AUTO takes GPU for an execute() whose rows all have restart intervals
// and HOST otherwise.  Any other value fails validate().  The frames are the same bytes either way.
//
// ImageDecoderArgs { ..., split = 3: INTERVAL = 0 | SUBSEQUENCE = 1 } (this build's own field too) chooses how the device decoder
// cuts the work.  INTERVAL, and a message without the field, is the above.  SUBSEQUENCE with entropy GPU or AUTO is
// ST_JPEG_ENTROPY_SUBSEQUENCE (st_jpeg_decode_batch_gpu_split()'s): one lane per fixed-size piece of the entropy-coded bytes, and a row without restart
// intervals is no error.  SUBSEQUENCE with entropy HOST (or absent) fails validate(), as any other value of split does.
//
// ImageDecoderArgs { ..., scale_denom = 4 } (this build's own field too) decodes at 1 / scale_denom: 1, 2, 4 or 8, libjpeg's
// scaled decoding (cv::IMREAD_REDUCED_COLOR_2 / _4 / _8), and the frame's FrameInfo is (ceil(h / d), ceil(w / d), channels).  Absent
// or 0 means 1; any other value fails validate().  It composes with whatever entropy and split select.
//
// ImageDecoderArgs { ..., png = 5: REFUSE = 0 | DECODE = 1 } (this build's own field too) decides whether PNG rows are decoded.
// REFUSE, and a message without the field, is all of the above, the validate() failures for image_type PNG / ANY included.
// DECODE makes image_type mean what it means in the reference: PNG -- every row must be a PNG, and a JPEG row is fatal with the
// row and the cause; JPEG -- as above; ANY or absent -- each row is told apart by its first 8 bytes, and an execute() may mix
// PNG and JPEG rows.  The PNG rows then go to ONE st_png_decode_batch() call (inflate on host threads, filter reconstruction
// and expansion in HIP kernels) and the JPEG rows to the JPEG call the other fields select: both take pointer
// arrays, so a subset needs no copy.  entropy, split and scale_denom apply to JPEG rows; a PNG row in an execute() with
// scale_denom other than 1 is fatal with the row and the cause.  Frames may then have 4 channels (R, G, B, A).  Any other
// value of png fails validate().
//
// The frame shape of an execute() is that of its first element.  Where the reference is undefined this fails instead: an
// element of another shape (the reference's CPU kernel copies it into a frame of the first one's size, :46-50), and an element
// that is not a baseline JPEG this library decodes ("Failed to decode image" there) are fatal with the row and the cause.
// Registered twice like the other classes: DeviceType::GPU reads host bytes and produces device frames, the staged
// DeviceType::CPU form decodes into a device buffer and copies host frames out.
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
enum { ENTROPY_HOST = 0, ENTROPY_GPU = 1, ENTROPY_AUTO = 2 };
enum { SPLIT_INTERVAL = 0, SPLIT_SUBSEQUENCE = 1 };
enum { PNG_REFUSE = 0, PNG_DECODE = 1 };
enum { TYPE_PNG = 0, TYPE_JPEG = 1, TYPE_ANY = 2 };
// false: not a message; *image_type: -1 when the field is absent; *entropy: ENTROPY_HOST, *split: SPLIT_INTERVAL, *scale: 1 when absent (or 0),
// *png: PNG_REFUSE when absent
bool parse_image_decoder_args(const std::vector<u8>& args, int* image_type, long long* entropy, long long* split, long long* scale, long long* png) {
  std::vector<proto_lite::Field> fields;
  *image_type = -1;
  *entropy = ENTROPY_HOST;
  *split = SPLIT_INTERVAL;
  *scale = 1;
  *png = PNG_REFUSE;
  if (!proto_lite::parse(args.data(), args.size(), &fields)) return false;
  for (auto& f : fields) {
    if (f.number == 1 && f.wire == 0) *image_type = (int)f.value;
    if (f.number == 2 && f.wire == 0) *entropy = (long long)f.value;
    if (f.number == 3 && f.wire == 0) *split = (long long)f.value;
    if (f.number == 4 && f.wire == 0) *scale = (int32_t)f.value == 0 ? 1 : (long long)(int32_t)f.value;   // an int32 field
    if (f.number == 5 && f.wire == 0) *png = (long long)f.value;
  }
  return true;
}
}  // namespace

template <bool STAGED>
class ImageDecoderKernelHIPImpl : public BatchedKernel {
 public:
  ImageDecoderKernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
    int image_type = -1;
    long long entropy = ENTROPY_HOST, split = SPLIT_INTERVAL, scale = 1, png = PNG_REFUSE;
    if (!parse_image_decoder_args(config.args, &image_type, &entropy, &split, &scale, &png)) RESULT_ERROR(&core_.valid, "ImageDecoder: could not parse ImageDecoderArgs");
    else if (png < PNG_REFUSE || png > PNG_DECODE) RESULT_ERROR(&core_.valid, "ImageDecoder: invalid png %lld (REFUSE = 0, DECODE = 1)", png);
    else if (png != PNG_DECODE && (image_type == 0 || image_type == 2))
      RESULT_ERROR(&core_.valid, "ImageDecoder: image_type %s is not supported (JPEG only)", image_type == 0 ? "PNG" : "ANY");
    else if (image_type != -1 && (image_type < 0 || image_type > 2)) RESULT_ERROR(&core_.valid, "ImageDecoder: invalid image_type %d", image_type);
    else if (entropy < ENTROPY_HOST || entropy > ENTROPY_AUTO)
      RESULT_ERROR(&core_.valid, "ImageDecoder: invalid entropy %lld (HOST = 0, GPU = 1, AUTO = 2)", entropy);
    else if (split < SPLIT_INTERVAL || split > SPLIT_SUBSEQUENCE)
      RESULT_ERROR(&core_.valid, "ImageDecoder: invalid split %lld (INTERVAL = 0, SUBSEQUENCE = 1)", split);
    else if (split == SPLIT_SUBSEQUENCE && entropy == ENTROPY_HOST)
      RESULT_ERROR(&core_.valid, "ImageDecoder: split = SUBSEQUENCE decodes on the device: entropy must be GPU or AUTO, not HOST");
    else if (scale != 1 && scale != 2 && scale != 4 && scale != 8)
      RESULT_ERROR(&core_.valid, "ImageDecoder: invalid scale_denom %lld (1, 2, 4 or 8)", scale);
    else core_.open("ImageDecoderKernelHIP");
    scale_ = scale == 2 || scale == 4 || scale == 8 ? (int)scale : 1;
    entropy_ = (int)entropy;
    by_subsequence_ = split == SPLIT_SUBSEQUENCE;
    png_ = png == PNG_DECODE;
    image_type_ = image_type;
  }
  void validate(Result* result) override { core_.validate(result); }

  void execute(const BatchedElements& input_columns, BatchedElements& output_columns) override {
    auto& img_col = input_columns[0];
    const i32 n = (i32)num_rows(img_col);
    if (n == 0) return;
    // the shape of the batch is that of its first element; every element is probed before anything is launched
    static const u8 kPngSignature[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    struct { int h, w, channels; } first = {0, 0, 0};
    bool restarts = true;   // every JPEG row has restart intervals
    is_png_.assign(n, 0);
    i32 n_png = 0;
    for (i32 i = 0; i < n; ++i) {
      int h, w, channels;
      // png = DECODE: image_type PNG takes every row for one, JPEG none, ANY (or absent) those that begin with the signature
      const bool is_png = png_ && (image_type_ == TYPE_PNG || (image_type_ != TYPE_JPEG && img_col[i].size >= 8 && memcmp(img_col[i].buffer, kPngSignature, 8) == 0));
      if (is_png) {
        st_png_info info;
        const int st = st_png_probe(img_col[i].buffer, img_col[i].size, &info);
        LOG_IF(FATAL, st != ST_OK) << "ImageDecoder: row " << i << " of the batch: " << info.message;
        LOG_IF(FATAL, scale_ != 1) << "ImageDecoder: row " << i << " of the batch: a PNG row cannot be decoded at scale_denom " << scale_
                                   << " (scaled decoding is JPEG's)";
        h = info.h; w = info.w; channels = info.channels;
        is_png_[i] = 1;
        ++n_png;
      } else {
        st_jpeg_info info;
        const int st = st_jpeg_probe(img_col[i].buffer, img_col[i].size, &info);
        LOG_IF(FATAL, st != ST_OK) << "ImageDecoder: row " << i << " of the batch: " << info.message;
        LOG_IF(FATAL, entropy_ == ENTROPY_GPU && !by_subsequence_ && info.restart_interval <= 0)
            << "ImageDecoder: row " << i << " of the batch: no restart intervals: the stream has no DRI segment, entropy = GPU needs one";
        restarts = restarts && info.restart_interval > 0;
        h = info.h; w = info.w; channels = info.channels;
      }
      if (i == 0) { first.h = h; first.w = w; first.channels = channels; }
      LOG_IF(FATAL, h != first.h || w != first.w || channels != first.channels)
          << "ImageDecoder: row " << i << " of the batch changes shape inside a batch (" << w << "x" << h << "x" << channels
          << " after " << first.w << "x" << first.h << "x" << first.channels << ")";
    }
    const bool on_gpu = entropy_ == ENTROPY_GPU || (entropy_ == ENTROPY_AUTO && restarts);
    int oh = first.h, ow = first.w;
    LOG_IF(FATAL, st_jpeg_scaled_size(first.h, first.w, scale_, &oh, &ow) != ST_OK) << "ImageDecoder: no frame size at scale 1/" << scale_;
    FrameInfo info(oh, ow, first.channels, FrameType::U8);
    std::vector<Frame*> output_frames = new_frames(core_.device, info, n);
    const size_t out_bytes = info.size(), out_stride = DeviceStage::align(out_bytes);
    u8* dev = nullptr;
    if (STAGED) {
      dev = stage_.reserve(out_stride * n);
      strided_ptrs(dst_, n, dev, out_stride);
    } else {
      output_ptrs(dst_, output_frames);
    }
    // the JPEG rows first in the three arrays, then the PNG rows: each call takes its own run of pointers
    const i32 n_jpeg = n - n_png;
    bufs_.resize(n);
    sizes_.resize(n);
    sub_dst_.resize(n);
    for (i32 i = 0, j = 0, p = n_jpeg; i < n; ++i) {
      const i32 k = is_png_[i] ? p++ : j++;
      bufs_[k] = img_col[i].buffer; sizes_[k] = img_col[i].size; sub_dst_[k] = dst_[i];
    }
    st_ctx* ctx = core_.ctx;
    if (n_jpeg > 0) {
      const int mode = by_subsequence_ ? ST_JPEG_ENTROPY_SUBSEQUENCE : on_gpu ? ST_JPEG_ENTROPY_INTERVAL : ST_JPEG_ENTROPY_HOST;
      const int st = st_jpeg_decode_batch_scaled(ctx, bufs_.data(), sizes_.data(), n_jpeg, first.h, first.w, first.channels, scale_, mode, nullptr, sub_dst_.data());
      LOG_IF(FATAL, st != ST_OK) << "ImageDecoder: " << st_ctx_last_error(ctx);
    }
    if (n_png > 0) {
      const int st = st_png_decode_batch(ctx, bufs_.data() + n_jpeg, sizes_.data() + n_jpeg, n_png, first.h, first.w, first.channels, sub_dst_.data() + n_jpeg);
      LOG_IF(FATAL, st != ST_OK) << "ImageDecoder: " << st_ctx_last_error(ctx);
    }
    core_.sync();
    if (STAGED) stage_.download_frames(output_frames, dev, out_stride, out_bytes);
    for (i32 i = 0; i < n; ++i) insert_frame(output_columns[0], output_frames[i]);
  }

 private:
  KernelCore core_;
  DeviceStage stage_;   // staged: the decoded frames
  int entropy_ = ENTROPY_HOST;
  int scale_ = 1;
  bool by_subsequence_ = false;
  bool png_ = false;        // png = DECODE
  int image_type_ = -1;     // -1: the field is absent
  std::vector<char> is_png_;
  std::vector<uint8_t*> sub_dst_;
  std::vector<const uint8_t*> bufs_;
  std::vector<size_t> sizes_;
  std::vector<uint8_t*> dst_;
};

using ImageDecoderKernelHIP = ImageDecoderKernelHIPImpl<false>;
using ImageDecoderKernelHIPStaged = ImageDecoderKernelHIPImpl<true>;

REGISTER_OP(ImageDecoder).input("img").frame_output("frame").protobuf_name("ImageDecoderArgs");

REGISTER_KERNEL(ImageDecoder, ImageDecoderKernelHIPStaged).device(DeviceType::CPU).batch().num_devices(1);

REGISTER_KERNEL(ImageDecoder, ImageDecoderKernelHIP).device(DeviceType::GPU).batch().num_devices(1);
}  // namespace scanner
