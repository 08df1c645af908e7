/*
 * scannertools_hip.h -- C ABI of libscannertools_hip.so: the MI355X (gfx950) implementation of
 * the arithmetic behind scannertools' Histogram and OpticalFlow ops.
 *
 * This is the boundary between host code (the Scanner kernels in
 * the scannertools_amd/scanner_kernels sources, the Python front-end, bench.py) and the HIP
 * kernels.  Plain pointers and sizes only; no C++ or torch types.  Every entry point
 *   - returns an int status (ST_OK == 0), never throws, never aborts;
 *   - selects the context's device on entry (Scanner calls kernel instances from their own
 *     evaluator threads; cf. set_device() at the top of every method in
 *     scannertools_cpp/imgproc/histogram_kernel_gpu.cpp:21,35 and
 *     optical_flow_kernel_gpu.cpp:18,29,37,41,47);
 *   - never allocates outputs: the caller passes device buffers it owns (Scanner allocates
 *     them with new_block_buffer / new_frames, histogram_kernel_gpu.cpp:38-39,
 *     optical_flow_kernel_gpu.cpp:61-64);
 *   - enqueues work on the context's stream and returns without synchronising, unless
 *     documented otherwise; call st_ctx_sync() before reading results on the host;
 *   - is re-entrant across contexts (one context per kernel instance / thread).
 *
 * "frames_dev" arguments are HOST arrays of DEVICE pointers (one Scanner element buffer per
 * frame); frames are dense interleaved U8 (h, w, 3), RGB order, no row padding -- the layout
 * frame_to_mat()/frame_to_gpu_mat() view in the reference.
 */
#ifndef SCANNERTOOLS_HIP_H_
#define SCANNERTOOLS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST_ABI_VERSION 1

enum st_status {
  ST_OK = 0,
  ST_ERR_INVALID = 1,     /* bad argument (null pointer, non-positive size, bins out of range ...) */
  ST_ERR_HIP = 2,         /* a HIP runtime call failed; see st_ctx_last_error() */
  ST_ERR_OOM = 3,         /* workspace allocation failed */
  ST_ERR_UNSUPPORTED = 4  /* parameter combination the HIP path does not implement */
};

typedef struct st_ctx st_ctx;

int st_abi_version(void);
/* "src=<first 16 hex digits of the sha256 over the library's sources, in the Makefile's order> host=<machine that compiled
 * it> at=<UTC time>": which sources this binary was built from and where (no reference counterpart: build provenance, so
 * that a test run can show it loaded a library compiled on the machine it runs on from the tree it runs in). */
const char* st_build_info(void);
const char* st_status_string(int status);
int st_device_count(int* count);

/* Per-kernel-instance context: owns a stream and lazily-sized scratch (pyramids, polynomial
 * expansions, matrices).  Replaces the per-instance state of the reference GPU wrappers
 * (streams_, planes_, flow_finders_, grayscale_; histogram_kernel_gpu.cpp:71-75,
 * optical_flow_kernel_gpu.cpp:101-107). */
/* ST_ERR_UNSUPPORTED: the device is not a gfx950-class part (the kernels are compiled for gfx950 and sized for its 160 KB
 * of LDS per workgroup); ST_ERR_INVALID: no such device. */
int st_ctx_create(int device_id, st_ctx** out_ctx);
int st_ctx_destroy(st_ctx* ctx);
/* Borrow an external hipStream_t (e.g. torch's current stream).  NULL is the HIP default
 * (null) stream, which is what torch's default stream is.  st_ctx_reset_stream() returns to
 * the context's own non-blocking stream.  Both drain the previously bound stream first. */
int st_ctx_set_stream(st_ctx* ctx, void* hip_stream);
int st_ctx_reset_stream(st_ctx* ctx);
int st_ctx_sync(st_ctx* ctx);
/* Diagnostic: 1 if the context's last st_farneback_pairs call chose its kernels for a GPU shared with other kernel instances of
 * this process (two or more other contexts had an OpticalFlow call in flight -- entered within 50 ms and not yet st_ctx_sync'ed --
 * and the call had at most 4 pairs), else 0.  Scanner runs K instances of a kernel class per GPU (pipeline_instances_per_node,
 * scannertools/tests/test_all.py:45,231); the choice is a scheduling matter only, results are bit-identical.  ST_CONCURRENT=0 / 1
 * (read at st_ctx_create) switches the detection off / forces it. */
int st_ctx_flow_concurrent(st_ctx* ctx);
/* Cap on scratch the context may hold (bytes; 0 = default 64 GiB).  Large pair batches are
 * processed in passes that fit. */
int st_ctx_set_workspace_limit(st_ctx* ctx, size_t bytes);
int st_ctx_release_workspace(st_ctx* ctx);
const char* st_ctx_last_error(const st_ctx* ctx);

/* ---- per-kernel timing (HIP events on the context's stream) --------------------------------
 * When enabled, every launch of the named kernel class is bracketed by hipEventRecord pairs;
 * st_ctx_timing_read() synchronises the stream and returns launches and total milliseconds
 * since the last reset.  Used by bench.py for the live roofline figure. */
enum st_kernel_id {
  ST_K_HIST = 0,
  ST_K_GRAY = 1,
  ST_K_PYR = 2,
  ST_K_POLYEXP = 3,
  ST_K_UPDATE_MATRICES = 4,
  ST_K_BLUR_UPDATE = 5, /* box blur + 2x2 solve (+ fused UpdateMatrices): the dominant kernel */
  ST_K_FLOW_HIST = 6,
  ST_K_DRAW_FLOW = 7,   /* max-reduction + render launches of one st_draw_flow_batch call */
  ST_K_BLUR_OP = 8,     /* the Blur op's box filter (not the Farneback blur, which is ST_K_BLUR_UPDATE) */
  ST_K_RESIZE = 9,
  ST_K_CVT_COLOR = 10,
  ST_K_CPM2_INPUT = 11,
  ST_K_CPM2_LIMBS = 12,
  ST_K_CONV = 13,       /* convolution / pooling launches of the pose network */
  ST_K_CPM2_RESIZE = 14,
  ST_K_CPM2_NMS = 15,      /* the library's non-maximum suppressions: CPM2's peak search and the FacenetOutput launches (decode, sort + greedy NMS, pack) */
  ST_K_FRAME_STATS = 16, /* moments + finishing launches of the frame-statistics ops */
  ST_K_JPEG = 17,        /* inverse DCT + upsample / colour launches of the ImageDecoder op; the ImageEncoder op's launches (four, or five without restart markers); the PNG launches of st_png_decode_batch (unfilter, expand) and of st_png_encode_batch (filter, deflate, layout, pack) */
  ST_K_NET_INPUT = 18,   /* the FacenetInput and CaffeInput launches */
  ST_K_COUNT = 19
};
int st_ctx_timing_enable(st_ctx* ctx, unsigned kernel_mask);
int st_ctx_timing_reset(st_ctx* ctx);
int st_ctx_timing_read(st_ctx* ctx, int kernel_id, int* launches, double* total_ms);

/* ---- Histogram -----------------------------------------------------------------------------
 * Replaces HistogramKernelCPU::execute's per-frame body
 * (scannertools_cpp/imgproc/histogram_kernel_cpu.cpp:25-45: cv::calcHist x3 + convertTo(CV_32S))
 * and the GPU wrapper's cvc::split + cvc::histEven x3 (histogram_kernel_gpu.cpp:48-57) for a
 * whole batch in one call.
 * out_dev: n * 3 * bins int32, frame-major then channel-major (R,G,B) -- element i is the
 * 3*bins*4-byte block the reference hands to insert_element() (histogram_kernel_cpu.cpp:44).
 * bins in [1, 256]; bin(v) = floor(v * bins / 256) (cv::calcHist uniform 8U table); the
 * reference's value is 16 (histogram_kernel_cpu.cpp:8). */
int st_hist_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w,
                       int bins, int32_t* out_dev);
/* Same, frames at base_dev + i * frame_stride_bytes (a contiguous device-resident stream). */
int st_hist_u8c3_strided(st_ctx* ctx, const uint8_t* base_dev, size_t frame_stride_bytes, int n,
                         int h, int w, int bins, int32_t* out_dev);

/* ---- Frame statistics: BrightnessCPP / ContrastCPP / SharpnessCPP and Brightness / Contrast / Sharpness -------------------
 * Replace the per-frame bodies of the legacy op library's BrightnessKernel, ContrastKernel and SharpnessKernel
 * (scannertools/old/cpp_ops/imgproc.cpp:50-79 cv::cvtColor(RGB2YUV) + cv::mean; :81-131 the same + a float32 sum of squared
 * deviations; :133-175 cv::Laplacian(CV_64F) + cv::meanStdDev + cv::pow) and of their Python twins (old/imgproc.py:11-37:
 * np.mean of the Y plane, np.sqrt(np.mean((Y - mean)**2)), cv2.Laplacian(frame, CV_64F).var()) for a whole batch.
 * Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14 (cv::cvtColor COLOR_RGB2YUV); L_c = the reflect-101 4-neighbour Laplacian of
 * channel c, an integer in [-1020, 1020] (the neighbour on an axis of length 1 is the pixel itself).
 * st_frame_moments_u8c3_*: moments_dev receives n records of 8 int64, in the order ST_FM_SY .. ST_FM_Q_B: sum Y, sum Y^2,
 *   sum L_R, sum L_G, sum L_B, sum L_R^2, sum L_G^2, sum L_B^2, exact.  what: ST_FM_LUMA and / or ST_FM_LAPLACIAN, the moments
 *   to compute; the call zeroes all n * 8 values first, so those not asked for are 0.  Frames of up to 2^31 - 1 bytes;
 *   ST_ERR_UNSUPPORTED for the Laplacian of rows wider than 19 786 pixels.
 * st_frame_stats_finish: out_dev[i] = statistic `kind` (ST_FS_*) of record i for frames of h x w pixels: float for the
 *   *_CPP kinds (the 4-byte element the reference's C++ op emits), double for the others (the value the Python op pickles).
 *   Reads the moments the kind needs: SY, QY for brightness and contrast, the Laplacian moments for sharpness.
 *   Formulas: scannertools_amd/csrc/st_framestats.hip, header comment. */
enum st_frame_moment { ST_FM_SY = 0, ST_FM_QY = 1, ST_FM_S_R = 2, ST_FM_S_G = 3, ST_FM_S_B = 4, ST_FM_Q_R = 5, ST_FM_Q_G = 6, ST_FM_Q_B = 7 };
enum st_frame_moment_mask { ST_FM_LUMA = 1, ST_FM_LAPLACIAN = 2 };
enum st_frame_stat_kind {
  ST_FS_BRIGHTNESS_CPP = 0, /* imgproc.cpp:61-75 */
  ST_FS_CONTRAST_CPP = 1,   /* imgproc.cpp:92-126 (see the deviation noted in st_framestats.hip) */
  ST_FS_SHARPNESS_CPP = 2,  /* imgproc.cpp:144-168 */
  ST_FS_BRIGHTNESS = 3,     /* old/imgproc.py:11-17 */
  ST_FS_CONTRAST = 4,       /* old/imgproc.py:20-30 */
  ST_FS_SHARPNESS = 5       /* old/imgproc.py:33-36 */
};
int st_frame_moments_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int what,
                                int64_t* moments_dev);
/* Same, frames at base_dev + i * frame_stride_bytes (a contiguous device-resident stream). */
int st_frame_moments_u8c3_strided(st_ctx* ctx, const uint8_t* base_dev, size_t frame_stride_bytes, int n, int h, int w,
                                  int what, int64_t* moments_dev);
int st_frame_stats_finish(st_ctx* ctx, const int64_t* moments_dev, int n, int h, int w, int kind, void* out_dev);

/* ---- SharpnessBBoxCPP / SharpnessBBox: sharpness of boxes of a frame ---------------------------------------------------------
 * Replace the per-box bodies of the legacy op library's SharpnessBBoxKernel (scannertools/old/cpp_ops/imgproc.cpp:177-234:
 * cv::resize of the box to 200 x 200 at INTER_LINEAR, cv::Laplacian(CV_64F), cv::meanStdDev) and of its Python twin
 * (old/imgproc.py:44-54) for all boxes of all frames of a call, in ONE moments launch (a call with fewer boxes than the GPU has
 * CUs cuts each box into bands of rows and adds a small second launch that sums them): a box is gathered from its frame, resized with
 * the Resize op's arithmetic (the region an image of its own: taps clamp inside it; an exactly 200 x 200 box is copied, an
 * exactly 400 x 400 box is the rounded mean of its 2 x 2 cells) and reduced to its six Laplacian moments without the resized
 * image leaving the chip.
 * boxes_host: m records of 5 int32 {frame index, x1, y1, x2, y2} in HOST memory, coordinates already truncated to pixels; the
 *   region is rows y1 .. y2-1, columns x1 .. x2-1.  Every record is validated before anything is launched: ST_ERR_INVALID
 *   (the message names the box) unless 0 <= frame < n, 0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h.  The records are copied during
 *   the call; any order, any overlap, a frame without a box and a box listed twice are all fine.
 * st_bbox_moments_u8c3_*: moments_dev receives m records of 8 int64 in the ST_FM_* layout of the ST_BBOX_SIDE x ST_BBOX_SIDE
 *   image of box i (SY = QY = 0), exact, so that st_frame_stats_finish(ctx, moments_dev, m, ST_BBOX_SIDE, ST_BBOX_SIDE,
 *   ST_FS_SHARPNESS_CPP or ST_FS_SHARPNESS, out) finishes them.  A box's record does not depend on what else is in the call.
 * st_bbox_sharpness_u8c3_*: the same launch with the finishing formula fused: out_dev[i] = statistic `kind`
 *   (ST_FS_SHARPNESS_CPP: float, ST_FS_SHARPNESS: double) of box i, bit for bit what the two calls above give.
 * Frames of up to 2^31 - 1 bytes at any byte alignment; m = 0 is a successful no-op; m above 2^31 - 1 is ST_ERR_UNSUPPORTED.
 * No host synchronisation (the scratch allocation may grow, as in every entry point). */
#define ST_BBOX_SIDE 200
int st_bbox_moments_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, const int32_t* boxes_host,
                               int64_t m, int64_t* moments_dev);
int st_bbox_moments_u8c3_strided(st_ctx* ctx, const uint8_t* base_dev, size_t frame_stride_bytes, int n, int h, int w,
                                 const int32_t* boxes_host, int64_t m, int64_t* moments_dev);
int st_bbox_sharpness_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, const int32_t* boxes_host,
                                 int64_t m, int kind, void* out_dev);
int st_bbox_sharpness_u8c3_strided(st_ctx* ctx, const uint8_t* base_dev, size_t frame_stride_bytes, int n, int h, int w,
                                   const int32_t* boxes_host, int64_t m, int kind, void* out_dev);

/* ---- ShotBoundaries (device-resident histograms) -------------------------------------------
 * Replaces the body of the ShotBoundaries python op, scannertools/shot_detection.py:12-28, for histograms that are
 * already on the GPU (the op itself stays host code in the reference; with resident frames its 10 000-window loop is
 * two thirds of the Histogram -> ShotBoundaries pipeline).  hist_dev: n * 3 * bins int32 as st_hist_u8c3_* writes
 * them; flags_dev[i] = 1 where frame i opens a shot: diffs[i] - mean(win) > k_std * std(win), win =
 * diffs[max(i - window, 0) : min(i + window, n)], diffs[i] = mean over the channels of the Chebyshev distance between
 * frames i-1 and i (shot_detection.py:14-18, :23-26; the reference's window = 500, k_std = 2.5).  Means and standard
 * deviations are formed in numpy's summation order, so the flags equal the reference's decisions bit for bit.
 * diffs_dev: optional n doubles that receive diffs (null: context scratch). */
int st_shot_boundaries(st_ctx* ctx, const int32_t* hist_dev, int n, int bins, int window, double k_std, uint8_t* flags_dev,
                       double* diffs_dev);

/* ---- OpticalFlow ---------------------------------------------------------------------------
 * Parameters of cv::FarnebackOpticalFlow::create(numLevels, pyrScale, fastPyramids, winSize,
 * numIters, polyN, polySigma, flags); st_fb_params_default() gives the reference's
 * (3, 0.5, false, 15, 3, 5, 1.2, 0) (optical_flow_kernel_cpu.cpp:15-16).  Implemented:
 * flags == 0 (box filter, no initial flow), fast_pyramids == 0, poly_n in {5, 7},
 * odd win_size in 3...63, num_iters >= 1, num_levels >= 0, pyr_scale in (0, 1).  gray_bits
 * selects cv::cvtColor's 8-bit luma table: 15 (OpenCV 4.x) or 14 (OpenCV <= 3.4.2).
 * win_size == 1 is refused (ST_ERR_UNSUPPORTED): at a window radius of 0 the reference's
 * running sums count row 0 and column 0 twice, so every "box sum" it forms is M[y] + M[0]; what
 * it returns there is an artefact of that initialisation, not a flow, and is not reproduced.
 * Two limits on the pyramid, both checked for every level before anything is launched
 * (ST_ERR_UNSUPPORTED, nothing written): the Gaussian of a level, cvRound(5 * sigma) | 1 taps
 * with sigma = (1 / pyr_scale^k - 1) / 2, has at most 31 taps (pyr_scale^k above 0.0735); and a
 * level that is not an exact 2 / 4 / 8 decimation with the reference's 3 / 9 / 19 taps is built
 * in tiles of 8 x 32 pixels whose source rows and columns, Gaussian apron included, must fit
 * 64 KiB of LDS: with s = 1 / pyr_scale^k and r = taps / 2,
 *   rows = ceil(7 s) + 2 r + 4, cols = (ceil(31 s) + 2 r + 4) rounded up to 4, 256 rows + rows cols <= 65536
 * (at 1080p the deepest level that can be built: pyr_scale 0.3: 1, 0.45: 2, 0.5: 3, 0.6: 4,
 * 0.7: 6, 0.75: 8, 0.8: 10; num_levels beyond it is refused where the frame is large enough to
 * reach that level). */
typedef struct st_fb_params {
  int num_levels;
  double pyr_scale;
  int fast_pyramids;
  int win_size;
  int num_iters;
  int poly_n;
  double poly_sigma;
  int flags;
  int gray_bits;
} st_fb_params;
void st_fb_params_default(st_fb_params* p);

/* Replaces OpticalFlowKernelCPU::execute (optical_flow_kernel_cpu.cpp:27-43: cvtColor
 * BGR2GRAY x2 + FarnebackOpticalFlow::calc) for a batch of stencil windows, and the
 * calling convention of OpticalFlowKernelGPU::execute (optical_flow_kernel_gpu.cpp:45-93).
 * pairs: HOST array of n_pairs x 2 indices into frames_dev; flow p goes FROM frame
 * pairs[2p] TO frame pairs[2p+1] (CPU-kernel direction: stencil element 0 -> element 1;
 * the reference GPU wrapper's reversed direction is a defect and is not reproduced).
 * Pairs need not be consecutive; each distinct frame's pyramid and polynomial expansion is
 * computed once per call.  flow_out_dev: HOST array of n_pairs DEVICE pointers, each a dense
 * (h, w, 2) F32 frame (u, v interleaved) as allocated by new_frames(device, FrameInfo(h, w, 2,
 * F32), n) (optical_flow_kernel_gpu.cpp:61-64). */
int st_farneback_pairs(st_ctx* ctx, const uint8_t* const* frames_dev, int n_frames,
                       const int32_t* pairs, int n_pairs, int h, int w, const st_fb_params* params,
                       float* const* flow_out_dev);

/* Number of pyramid levels processed minus one (k runs levels..0) and per-level geometry, as
 * FarnebackOpticalFlowImpl::calc derives them. */
int st_fb_levels(int h, int w, const st_fb_params* params);
int st_fb_level_geom(int h, int w, const st_fb_params* params, int level, int* lh, int* lw,
                     double* sigma, int* ksize);

/* ---- stage-level entry points (parity tests drive each Farneback stage separately) ---------
 * All arrays are dense device arrays.  M fields are planar (5, h, w) F32 (channel c at
 * base + c*h*w); flow fields are (h, w, 2) F32 interleaved.  Polynomial expansions R (r_dev,
 * r0_dev, r1_dev; 5*h*w floats, 16-byte aligned) use the layout the production kernels read:
 * channels 0..3 of OpenCV's interleaved 5-channel R as h*w float4, then channel 4 as h*w
 * floats. */
int st_gray_u8(st_ctx* ctx, const uint8_t* rgb_dev, int h, int w, int gray_bits, uint8_t* gray_dev);
int st_fb_pyr_image(st_ctx* ctx, const uint8_t* gray_dev, int h, int w, const st_fb_params* params,
                    int level, float* img_dev /* (lh, lw) */);
int st_fb_polyexp(st_ctx* ctx, const float* img_dev, int h, int w, int poly_n, double poly_sigma,
                  float* r_dev /* R layout, 5*h*w floats */);
/* M = UpdateMatrices(R0, R1, flow).  If coarse_flow_dev != NULL the flow is first produced as
 * resize(coarse_flow (ch, cw, 2) -> (h, w), INTER_LINEAR) * (1/pyr_scale) (the level
 * transition of calc()); else flow_dev (h, w, 2) is used; if both are NULL the flow is zero. */
int st_fb_update_matrices(st_ctx* ctx, const float* r0_dev, const float* r1_dev, const float* flow_dev,
                          const float* coarse_flow_dev, int ch, int cw, double pyr_scale, int h, int w,
                          float* m_dev /* (5,h,w) */);
/* One FarnebackUpdateFlow_Blur pass: flow_out = solve(box(M)); if update != 0 additionally
 * m_out = UpdateMatrices(R0, R1, flow_out).  m_out must not alias m_in.  block_size: odd, 3...63
 * (1 is refused as win_size 1 is). */
int st_fb_update_flow_blur(st_ctx* ctx, const float* r0_dev, const float* r1_dev, const float* m_in_dev,
                           int h, int w, int block_size, int update, float* flow_out_dev,
                           float* m_out_dev);

/* One whole iteration as the production path runs it (block_size 15 only):
 *   flow_out = solve(box(UpdateMatrices(R0, R1, flow_in)))  without materialising M.
 * flow_in: flow_in_dev (h,w,2), or resize(coarse_flow (ch,cw,2))*(1/pyr_scale), or zero when both
 * are NULL.  Equals st_fb_update_matrices followed by st_fb_update_flow_blur(update = 0). */
int st_fb_flow_iteration(st_ctx* ctx, const float* r0_dev, const float* r1_dev, const float* flow_in_dev,
                         const float* coarse_flow_dev, int ch, int cw, double pyr_scale, int h, int w,
                         int block_size, float* flow_out_dev);

/* ---- Flow consumers ------------------------------------------------
 * FlowHistogram: replaces FlowHistogramKernelCPU::execute's per-frame body
 * (scannertools/old/cpp_ops/flow_histogram_kernel_cpu.cpp:26-57: cv::split, cv::cartToPolar(x, y,
 * mag, deg, true), cv::calcHist on mag over [0,64) and on deg over [0,360), 64 bins each,
 * convertTo(CV_32S)) for a whole batch in one launch.
 * flows: n device pointers to (h, w, 2) float32 flow frames (x then y, the layout OpticalFlow
 * emits), 8-byte aligned.  out_dev: n * 2 * 64 int32, per frame the magnitude row then the angle
 * row -- the 512-byte block the reference hands to insert_element() (:55).  Values outside the
 * ranges (mag >= 64, deg == 360, NaN) are not counted, as in cv::calcHist. */
int st_flow_hist_batch(st_ctx* ctx, const float* const* flows_dev, int n, int h, int w, int32_t* out_dev);
/* Same, flow frames at base_dev + i * frame_stride_bytes. */
int st_flow_hist_strided(st_ctx* ctx, const float* base_dev, size_t frame_stride_bytes, int n, int h,
                         int w, int32_t* out_dev);

/* DrawFlow: replaces draw_flow() of scannertools/vis.py:8-12 for a batch:
 * out = hstack(frame, uint8(min(avg / max(avg), 1) * 255) on 3 channels), avg = (fx + fy) / 2 in
 * float32, max taken over the frame (NaN propagates, as np.max does), numpy's float32 -> uint8
 * cast.  frames: (h, w, 3) uint8; flows: (h, w, 2) float32, 8-byte aligned; out: (h, 2w, 3) uint8. */
int st_draw_flow_batch(st_ctx* ctx, const uint8_t* const* frames_dev, const float* const* flows_dev,
                       int n, int h, int w, uint8_t* const* out_dev);

/* ---- Sibling imgproc ops ---------------------------------------------
 * Blur: replaces BlurKernel::execute (scannertools_cpp/imgproc/blur_kernel_cpu.cpp:50-81), the
 * reference's own box filter: window [-left, +right] around each interior pixel with
 * left = ceil(kernel_size/2.0) - 1, right = kernel_size/2, per channel
 * out = sum / (left + right + 1)^2 in unsigned integer arithmetic; BlurArgs.sigma is ignored, as in
 * the reference.  frames / out: n device pointers to (h, w, 3) uint8; out must not alias its input.
 * Border pixels (which the reference leaves uninitialised) are set to 0.  kernel_size in [1, 31]. */
int st_box_blur_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w,
                           int kernel_size, uint8_t* const* out_dev);

/* Resize: replaces the cv::resize(img, out, Size(out_w, out_h), 0, 0, interpolation) call of
 * ResizeKernel::execute (scannertools_cpp/imgproc/resize_kernel.cpp:68-73) for U8 frames of 1..4
 * channels.  interpolation takes cv::InterpolationFlags values; ST_INTER_LINEAR (the op's default,
 * resize_kernel.cpp:31), ST_INTER_NEAREST, ST_INTER_CUBIC, ST_INTER_AREA and ST_INTER_LANCZOS4 are
 * implemented -- every entry of the reference's table (resize_kernel.cpp:10-17) except the
 * INTER_MAX mask value, which returns ST_ERR_UNSUPPORTED.
 * The target size is the caller's business (ResizeArgs width/height/min/preserve_aspect,
 * resize_kernel.cpp:44-62, is evaluated by the kernel class). */
enum st_interpolation { ST_INTER_NEAREST = 0, ST_INTER_LINEAR = 1, ST_INTER_CUBIC = 2, ST_INTER_AREA = 3, ST_INTER_LANCZOS4 = 4 };
int st_resize_u8_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int channels,
                       int out_h, int out_w, int interpolation, uint8_t* const* out_dev);

/* Montage: replaces the per-frame cv::resize(img, canvas(Rect(tw * x, th * y, tw, th)), Size(tw, th)) calls of
 * MontageKernel::execute (scannertools_cpp/imgproc/montage_kernel_gpu.cpp; MontageArgs{num_frames = 1, target_width = 4,
 * frames_per_row = 6}, scannertools_imgproc.proto).
 * st_montage_geometry: MontageKernel::new_frame_info's geometry for frames of (frame_h, frame_w), evaluated as it does --
 *   target_h = (i32)(target_width / (1.0 * frame_w) * frame_h), montage_w = frames_per_row * target_width,
 *   montage_h = (i64)(ceil(num_frames / (1.0 * frames_per_row)) * target_h).  ST_ERR_INVALID for a non-positive argument,
 *   a target_h below 1, a montage_w beyond int32 or a canvas (montage_h * montage_w * 3 bytes) beyond int64.  Host-only.
 * st_montage_clear: zeroes a (montage_h, montage_w, 3) canvas on the context's stream (MontageKernel::reset).
 * st_montage_u8c3_batch: resizes n dense (h, w, 3) U8 frames into tiles first_slot .. first_slot + n - 1 of a canvas whose
 *   rows are 3 * montage_w bytes apart -- tile s at pixel ((s % frames_per_row) * target_w, (s / frames_per_row) * target_h)
 *   -- in one launch, bit for bit what st_resize_u8_batch(..., ST_INTER_LINEAR, ...) gives for the same sizes (an equal
 *   size is a copy, an exact 2 x 2 decimation the INTER_AREA mean).  Every other byte of the canvas is left as it is; the
 *   caller sizes the canvas for the slots it names. */
int st_montage_geometry(int frame_h, int frame_w, int64_t num_frames, int target_width, int frames_per_row, int* target_h,
                        int64_t* montage_h, int* montage_w);
int st_montage_clear(st_ctx* ctx, uint8_t* montage_dev, int64_t montage_h, int montage_w);
int st_montage_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, uint8_t* montage_dev,
                          int montage_w, int target_w, int target_h, int frames_per_row, int first_slot);

/* ConvertColor: replaces the cv::cvtColor(img, out, code) call of ConvertColorKernel::execute
 * (scannertools_cpp/imgproc/convert_color_kernel.cpp:268-271) for U8 frames.  code takes
 * cv::ColorConversionCodes values; implemented: the ones below (the reference's name table at
 * convert_color_kernel.cpp:10-209 lists many more, which return ST_ERR_UNSUPPORTED).  gray_bits
 * selects the luma table width as in st_fb_params (15: OpenCV 4.x, 14: <= 3.4.2).
 * st_cvt_color_out_channels() gives the channel count of the output frame (-1: unsupported). */
enum st_color_code {
  /* channel layout family: codes 0..3, 5, 9..31 (alpha channel added / dropped / swapped, 16-bit BGR565 / BGR555
   * pixels as 2-channel frames, gray from / to them) */
  ST_COLOR_BGR2BGRA = 0, ST_COLOR_BGRA2BGR = 1, ST_COLOR_BGR2RGBA = 2, ST_COLOR_RGBA2BGR = 3, ST_COLOR_BGRA2RGBA = 5,
  ST_COLOR_GRAY2BGRA = 9, ST_COLOR_BGRA2GRAY = 10, ST_COLOR_RGBA2GRAY = 11,
  ST_COLOR_BGR2BGR565 = 12, ST_COLOR_RGB2BGR565 = 13, ST_COLOR_BGR5652BGR = 14, ST_COLOR_BGR5652RGB = 15,
  ST_COLOR_BGRA2BGR565 = 16, ST_COLOR_RGBA2BGR565 = 17, ST_COLOR_BGR5652BGRA = 18, ST_COLOR_BGR5652RGBA = 19,
  ST_COLOR_GRAY2BGR565 = 20, ST_COLOR_BGR5652GRAY = 21,
  ST_COLOR_BGR2BGR555 = 22, ST_COLOR_RGB2BGR555 = 23, ST_COLOR_BGR5552BGR = 24, ST_COLOR_BGR5552RGB = 25,
  ST_COLOR_BGRA2BGR555 = 26, ST_COLOR_RGBA2BGR555 = 27, ST_COLOR_BGR5552BGRA = 28, ST_COLOR_BGR5552RGBA = 29,
  ST_COLOR_GRAY2BGR555 = 30, ST_COLOR_BGR5552GRAY = 31,
  ST_COLOR_BGR2RGB = 4, ST_COLOR_RGB2BGR = 4,
  ST_COLOR_BGR2GRAY = 6, ST_COLOR_RGB2GRAY = 7,
  ST_COLOR_GRAY2BGR = 8, ST_COLOR_GRAY2RGB = 8,
  ST_COLOR_BGR2XYZ = 32, ST_COLOR_RGB2XYZ = 33, ST_COLOR_XYZ2BGR = 34, ST_COLOR_XYZ2RGB = 35,
  ST_COLOR_BGR2YCrCb = 36, ST_COLOR_RGB2YCrCb = 37, ST_COLOR_YCrCb2BGR = 38, ST_COLOR_YCrCb2RGB = 39,
  ST_COLOR_BGR2HSV = 40, ST_COLOR_RGB2HSV = 41, ST_COLOR_HSV2BGR = 54, ST_COLOR_HSV2RGB = 55,
  ST_COLOR_BGR2HSV_FULL = 66, ST_COLOR_RGB2HSV_FULL = 67, ST_COLOR_HSV2BGR_FULL = 70, ST_COLOR_HSV2RGB_FULL = 71,
  ST_COLOR_BGR2HLS = 52, ST_COLOR_RGB2HLS = 53, ST_COLOR_HLS2BGR = 60, ST_COLOR_HLS2RGB = 61,
  ST_COLOR_BGR2HLS_FULL = 68, ST_COLOR_RGB2HLS_FULL = 69, ST_COLOR_HLS2BGR_FULL = 72, ST_COLOR_HLS2RGB_FULL = 73,
  ST_COLOR_BGR2YUV = 82, ST_COLOR_RGB2YUV = 83, ST_COLOR_YUV2BGR = 84, ST_COLOR_YUV2RGB = 85
};
int st_cvt_color_out_channels(int code, int in_channels);
/* Output shape of a conversion: most codes keep (h, w) and change the channel count (st_cvt_color_out_channels);
 * the YUV 4:2:0 sources (cv::cvtColor codes 90..106: NV12, NV21, YV12, IYUV / I420 -- a (3H/2, W) single-channel frame, what a
 * video decoder hands out) produce (H, W, 3 | 4 | 1); the packed 4:2:2 sources (107..124: UYVY, YUY2, YVYU; (H, W, 2))
 * produce (H, W, 3 | 4 | 1).  Returns 0, or -1 when the code does not apply to such a frame.  The output-shape probe of
 * ConvertColorKernel::execute (convert_color_kernel.cpp:252-277). */
int st_cvt_color_out_shape(int code, int in_h, int in_w, int in_channels, int* out_h, int* out_w, int* out_channels);
int st_cvt_color_u8_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int channels,
                          int code, int gray_bits, uint8_t* const* out_dev);

/* ---- Pose path (scannertools_caffe) ------------------------------------
 * Geometry of the CPM2 network input for a frame of (h, w) at `scale`, as CPM2InputKernel::new_frame_info
 * and CPM2OutputKernel::new_frame_info derive it (scannertools_caffe_cpp/cpm2_input_kernel_gpu.cpp:44-55,
 * cpm2_output_kernel_cpu.cpp:123-137): resize = (int)(size * scale) in float, padded up to a multiple of 8.
 * Host-only (no context). */
int st_cpm2_geometry(int h, int w, float scale, int* resize_h, int* resize_w, int* net_h, int* net_w);

/* The float scale for which the rule above resizes a frame of height h to EXACTLY target_h rows: (int)(h * scale)
 * == target_h.  (float)target_h / h can fall one row short under the truncation -- 368.f / 1080 gives 367 -- which
 * would add a padded row and shift every normalised y coordinate of the OpenPose op, whose network input height is a
 * given (op::Wrapper netInputSize = (-1, 368), scannertools_caffe_cpp/openpose_kernel.cpp:99).  Host-only. */
int st_cpm2_scale_for_height(int h, int target_h, float* scale);

/* CPM2Input: replaces the per-frame body of CPM2InputKernel::execute
 * (cpm2_input_kernel_gpu.cpp:104-140: cvtColor RGB2BGR, resize INTER_CUBIC, copyMakeBorder with 128,
 * convertTo(F32, 1/256, -0.5), split, three plane copies, cudaMemcpy2DAsync) for a whole batch in one
 * launch.  frames: n device pointers to (h, w, 3) uint8 RGB frames; out: n device pointers to dense
 * planar (3, net_h, net_w) float32 frames (planes B, G, R), the FrameInfo(3, net_h, net_w, F32) frame the
 * reference hands to insert_frame (:96-103).  Arithmetic: OpenCV's CPU functions of the same names (the
 * reference file calls their cv::cuda twins, whose bicubic is a different filter; see st_pose.hip). */
int st_cpm2_input_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, float scale,
                        float* const* out_dev);

/* CPM2Output, candidate scoring: replaces the pair loop of CPM2OutputKernel::connect_limbs_coco
 * (cpm2_output_kernel_cpu.cpp:424-487) for all 19 limbs of the COCO_18 model and a batch of frames.
 * heatmaps: n device pointers to (57, net_h, net_w) float32 maps ("cpm2_resized_map"); peaks: n device
 * pointers to (18, max_peaks + 1, 3) float32 joint candidates ("cpm2_joints": row 0 of a part = [count,
 * -, -], rows 1.. = (x, y, score)).  scores_dev: n * 19 * max_peaks * max_peaks float32; entry
 * [f][k][i-1][j-1] is the mean part-affinity score sum/count of candidate pair (i, j) of limb k when
 * more than min_above of the 10 samples exceed inter_threshold, else -1 (the reference's values:
 * inter_threshold 0.05, min_above 9, max_peaks 64; :795-801). */
int st_cpm2_limb_scores(st_ctx* ctx, const float* const* heatmaps_dev, const float* const* peaks_dev, int n,
                        int net_h, int net_w, int max_peaks, float inter_threshold, int min_above,
                        float* scores_dev);

/* Convolution stack of the pose network (what the Caffe forward pass behind the reference's CPM2 op
 * computes, scannertools_caffe_cpp/cpm2_kernel.cpp:8-52 / caffe_kernel.cpp; layer list: profiles/NOTES.md, Part II section 9).
 * float32 throughout, as in the reference.  Activations are NHWC float32 device arrays whose channel count
 * (x_stride / y_stride floats per pixel) is a multiple of 4; a call reads cin channels from channel
 * x_offset on and writes cout channels from channel y_offset on, so concatenations need no copy.
 * st_conv2d_nhwc_f32: stride-1 "same" convolution (odd square kernel <= 7) + bias (+ ReLU).  cin must be a
 * multiple of 16 (pad channels zero).  w_dev: [cout_pad][kh][kw][cin] with cout_pad a multiple of 64 >= cout
 * (extra rows zero), bias_dev: [cout_pad]. */
int st_conv2d_nhwc_f32(st_ctx* ctx, const float* x_dev, int n, int h, int w, int cin, int x_stride, int x_offset,
                       const float* w_dev, const float* bias_dev, int kh, int kw, int cout, int cout_pad, int relu,
                       float* y_dev, int y_stride, int y_offset);
/* The same convolution with the weights ALSO in the spatial-tile kernel's operand order (wt_dev: st_conv_f32_tile_bytes(...)
 * bytes filled once by st_conv_pack_weights_f32_tile from the same float32 tensor; the size is 0 and wt_dev may be null for
 * layers the tile kernel does not take -- anything but 3x3 / 7x7 with cout_pad a multiple of 128).  The library picks the
 * kernel per call (tile shape by map size, tile or per-tap kernel by launch size; ST_CONV_TILE=0 / 1 at st_ctx_create forces
 * the per-tap / the tile kernel).  Both accumulate every output as the same k-ordered float32 fmaf chain (16-channel slices
 * outer, taps inner, channels ascending), so the choice -- and with it the batch size -- never changes a bit.
 * st_conv2d_nhwc_f32 = this with wt_dev null. */
long long st_conv_f32_tile_bytes(int cout_pad, int kh, int kw, int cin);
int st_conv_pack_weights_f32_tile(st_ctx* ctx, const float* w_dev, int cout_pad, int kh, int kw, int cin, void* out_dev);
int st_conv2d_nhwc_f32_tiled(st_ctx* ctx, const float* x_dev, int n, int h, int w, int cin, int x_stride, int x_offset,
                             const float* w_dev, const void* wt_dev, const float* bias_dev, int kh, int kw, int cout, int cout_pad,
                             int relu, float* y_dev, int y_stride, int y_offset);
/* TWO convolutions of the same geometry (n, h, w, cin, kernel, cout_pad, relu) on different operands -- the two branches of a
 * stage of the pose network -- in one launch where the spatial-tile kernel runs (at the reference's five frames per call a
 * 7x7 layer alone leaves a third of the CUs idle), else one after the other.  The result is exactly what the two single
 * calls give.  w: the float32 tensor (f32) / the packed buffer (bf16x3); w_tile: f32 tile-order copy or null (bf16x3: unused). */
typedef struct st_conv_operands {
  const float* x; int x_stride, x_offset;
  const void* w; const void* w_tile;
  const float* bias; int cout;
  float* y; int y_stride, y_offset;
} st_conv_operands;
int st_conv2d_nhwc_f32_pair(st_ctx* ctx, int n, int h, int w, int cin, int kh, int kw, int cout_pad, int relu,
                            const st_conv_operands* a, const st_conv_operands* b);
int st_conv2d_nhwc_bf16x3_pair(st_ctx* ctx, int n, int h, int w, int cin, int kh, int kw, int cout_pad, int relu,
                               const st_conv_operands* a, const st_conv_operands* b);
/* 2x2 max pooling, stride 2: (n, h, w, c) -> (n, h/2, w/2, c), c a multiple of 4. */
/* The same convolution on the bf16 matrix pipe at float32-grade accuracy ("bf16x3": every operand split into three
 * bf16 terms, the six significant products accumulated in float32; 2.67 x the float32 matrix rate on CDNA4, results
 * within one float32 rounding per product of st_conv2d_nhwc_f32's, not bit-identical to it).  Opt-in replacement for
 * the same Caffe layers (cpm2_kernel.cpp:8-52).  Activations and outputs as above; w3_dev: the layer's weights
 * rearranged ONCE by st_conv_pack_weights_bf16x3 from the [cout_pad][kh][kw][cin] float32 tensor into a 16-byte
 * aligned buffer of st_conv_bf16x3_packed_bytes(...) bytes (6 bytes per weight; twice that for 3x3 / 7x7 layers with
 * cout_pad a multiple of 128, which also get the operand-order copy the spatial-tile kernel reads -- the library picks
 * the kernel per call; both kernels add the same products in the same order, so the result does not depend on the choice). */
long long st_conv_bf16x3_packed_bytes(int cout_pad, int kh, int kw, int cin);
/* out_bytes: the size of the buffer behind out_dev; less than st_conv_bf16x3_packed_bytes(...) is ST_ERR_INVALID (nothing is
 * written).  st_conv_pack_weights_bf16x3 is the same call without the check: the caller vouches for the size. */
int st_conv_pack_weights_bf16x3_n(st_ctx* ctx, const float* w_dev, int cout_pad, int kh, int kw, int cin, void* out_dev,
                                  size_t out_bytes);
int st_conv_pack_weights_bf16x3(st_ctx* ctx, const float* w_dev, int cout_pad, int kh, int kw, int cin, void* out_dev);
int st_conv2d_nhwc_bf16x3(st_ctx* ctx, const float* x_dev, int n, int h, int w, int cin, int x_stride, int x_offset,
                          const void* w3_dev, const float* bias_dev, int kh, int kw, int cout, int cout_pad, int relu,
                          float* y_dev, int y_stride, int y_offset);

int st_maxpool2_nhwc_f32(st_ctx* ctx, const float* x_dev, int n, int h, int w, int c, int x_stride, float* y_dev,
                         int y_stride);
/* planar (n, c, h, w) -> NHWC (n, h, w, y_stride) with zero pad channels: CPM2Input's frame as the first
 * layer's operand. */
int st_planar_to_nhwc_f32(st_ctx* ctx, const float* x_dev, int n, int c, int h, int w, float* y_dev, int y_stride);

/* The two layers between the network and CPM2Output, which the reference configures in
 * CPM2Kernel::net_config (scannertools_caffe_cpp/cpm2_kernel.cpp:13-29: the Caffe fork's ImResizeLayer "resize"
 * with start scale 1 / target = network input size, and its "nms" layer) and whose outputs are the op's columns
 * cpm2_resized_map and cpm2_joints (cpm2_kernel.cpp:46-49).  The layers' sources are not in the reference tree:
 * behaviour restated from the published fork ([EXT], unpinned; csrc/st_pose.hip says what exactly).
 * st_cpm2_resize_maps: src (n, src_h, src_w, src_stride) channel-last float32 maps -> n planar (nmaps, dst_h,
 * dst_w) frames (out_dev: host array of n device pointers); output plane c reads source channel chan_map[c]
 * (host array; NULL = identity); bicubic (Catmull-Rom), one scale. */
int st_cpm2_resize_maps(st_ctx* ctx, const float* src_dev, int n, int src_h, int src_w, int src_stride,
                        const int* chan_map, int nmaps, int dst_h, int dst_w, float* const* out_dev);
/* Several network scales merged (OpenPoseArgs.pose_num_scales / pose_scale_gap, openpose_kernel.cpp:96-112; the `num`
 * loop of the fork's resize kernel): source s = (n, src_h[s], src_w[s], src_stride) maps of which eff_h[s] x eff_w[s]
 * source pixels (float) correspond to the whole output; per output pixel the bicubic interpolants of the scales are
 * summed in order and divided by `scales` (<= 8).  One scale with eff = its map size is st_cpm2_resize_maps, bit for bit. */
int st_cpm2_resize_merge_maps(st_ctx* ctx, const float* const* src_dev, const int* src_h, const int* src_w, const float* eff_h,
                              const float* eff_w, int scales, int n, int src_stride, const int* chan_map, int nmaps, int dst_h,
                              int dst_w, float* const* out_dev);
/* st_cpm2_nms: peaks of the first `parts` planes of n (>= parts, h, w) maps: strict 8-neighbour maxima above
 * `threshold`, interior pixels only, raster order, at most max_peaks per part.  joints_dev: n device pointers to
 * (parts, max_peaks + 1, 3) float32: row 0 = [count, 0, 0], row i = (x, y, score) -- the layout
 * cpm2_output_kernel_cpu.cpp:481-499 reads. */
int st_cpm2_nms(st_ctx* ctx, const float* const* maps_dev, int n, int h, int w, int parts, int max_peaks, float threshold,
                float* const* joints_dev);

/* ---- Network inputs (scannertools_caffe): FacenetInput and CaffeInput ----------------------------------
 * Geometry of the Facenet network input for a frame of (h, w) at `scale`, as FacenetInputKernelCPU::new_frame_info derives
 * it (scannertools_caffe_cpp/facenet_input_kernel_cpu.cpp:21-29): floor(float(size) * scale) in float32, rounded up to a
 * multiple of 8.  Host-only (no context).  ST_ERR_INVALID for scale <= 0 or a size below one pixel. */
int st_facenet_geometry(int h, int w, float scale, int* net_h, int* net_w);

/* FacenetInput: replaces the per-frame body of FacenetInputKernelCPU::execute (facenet_input_kernel_cpu.cpp:81-117:
 * cv::resize INTER_LINEAR to (net_w, net_h), convertTo(CV_32FC3), subtract the mean_colors Scalar, split, three
 * transposes, three plane copies, a row-wise memcpy) for a whole batch in one launch.  frames: n device pointers to
 * (h, w, 3) uint8 RGB frames; mean: mean_colors[0..2], subtracted from channels R, G, B in float32; out: n device pointers
 * to dense float32 frames of FrameInfo(3, net_w, net_h, F32) (:75): element [c][x][y] = float(resized[y][x][c]) - mean[c],
 * every plane transposed, channels in frame order.  The resize is the Resize op's INTER_LINEAR (cv::resize for 8-bit
 * data: 11-bit fixed point, the exact 2 x 2 mean at a precise 2:1 ratio, a copy at equal size); parity is with this CPU
 * kernel, not with facenet_input_kernel_gpu.cpp, whose cv::cuda::resize interpolates in float. */
int st_facenet_input_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, float scale,
                           const float* mean, float* const* out_dev);

/* One axis of CaffeInput's box filter (caffe_input_transformer_base.h:51-70, kernel_box :10-13), n_in source samples ->
 * n_out outputs, every operation an IEEE float32 operation: scale = float(n_out) / float(n_in), ks = 0.5f / scale and per
 * output x: src = (float(x) + 0.5f) / scale, begin[x] = int(src - ks + 0.5f); tap k of [0, int(2.0f * ks + 1.0f)) is a
 * member when fabsf((float(k + begin) - src) * scale) <= 0.5f.  first[x]: the first member's k (-1: none), count[x]: the
 * number of members; member k reads source index min(begin + k, n_in - 1) with weight 1.0f / float(count).  Host only (no
 * context, no GPU); the arrays hold n_out entries each and are always filled.  ST_ERR_UNSUPPORTED when some window is
 * empty (the reference divides 0 by 0 there: non-integer enlargements) or its members are not contiguous;
 * ST_ERR_INVALID for sizes outside 1 .. 2^24 or a null array. */
int st_caffe_input_axis(int n_in, int n_out, int* begin, int* first, int* count);

/* CaffeInput: replaces CaffeInputKernel::transform_halide (caffe_input_kernel.cpp:75-138; the pipeline is
 * caffe_input_transformer_base.h:43-105) for a whole batch in one launch.  frames: n device pointers to (h, w, 3) uint8
 * RGB frames; out: n device pointers to dense planar (3, net_h, net_w) float32 frames, the FrameInfo(3, net_h, net_w,
 * F32) of :186.  Horizontal pass first: per source row, channel and output column the sum over the window's members of
 * weight * float(pixel), accumulated in member order, multiply and add rounded separately; the vertical pass is the same
 * sum over those rows; then clamp to [0, 255].  Output plane c = (clamped value of input channel 2 - c) - mean_bgr[c]
 * (mean_colors in B, G, R order, :129-130), divided by 255.0f when `normalize`.  The window tables come from
 * st_caffe_input_axis, computed on the host once per geometry and kept in the context.  A geometry that function refuses
 * is ST_ERR_UNSUPPORTED here, before anything is launched or written (known deviation: the reference produces NaN). */
int st_caffe_input_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int net_h, int net_w,
                         const float* mean_bgr, int normalize, float* const* out_dev);

/* ---- FacenetOutput (scannertools_caffe): detector maps to NMS-filtered face boxes ------------------------
 * Replaces the per-frame body of FacenetOutputKernel::execute (scannertools_caffe_cpp/facenet_output_kernel_cpu.cpp:72-163)
 * for a whole batch.  maps_dev: n device pointers (4-byte aligned) to the Facenet op's float32 maps of 125 * G values,
 * G = grid_w * grid_h, grid = ceil(net / 8) of st_facenet_geometry(h, w, scale): 25 * G confidences conf[t][xi][yi], then
 * 100 * G adjustments adj[k][t][xi][yi] (k = dcx, dcy, dcw, dch).  templates: the 25 x 4 floats of the templates file.
 * Candidates are numbered t over the valid templates ({4..11, 18..24}; {4..11} when scale > 1), then xi, then yi.  Per
 * candidate, every operation an IEEE float32 operation rounded on its own unless said otherwise:
 *   e = float32(exp(float64(-c))); score = float32(1.0 / (1.0 + float64(e))); dropped when float64(score) < float64(threshold);
 *   x = float(8 xi - 1), y = float(8 yi - 1); tw = (T[t][2] - T[t][0]) + 1, th = (T[t][3] - T[t][1]) + 1;
 *   x += tw * dcx; y += th * dcy; bw = tw * float32(exp(float64(dcw))); bh = th * float32(exp(float64(dch)));
 *   each of x, y, bw, bh: (v / float(net_dim)) * float(frame_dim); dropped on bw < 0, bh < 0 or a NaN among the four;
 *   x1 = (x - bw / 2) / w, y1 = (y - bh / 2) / h, x2 = (x + bw / 2) / w, y2 = (y + bh / 2) / h.  Nothing is clamped.
 * The survivors of a frame then go through the greedy suppression of st_bbox_nms_f32 with `overlap` and `offset`.
 * counts_host[i]: the boxes frame i keeps.  The rows [x1, y1, x2, y2, score] of all frames, frame after frame, each frame's
 * in kept order (descending score), stay in a buffer of the context until its next st_facenet_output_batch call;
 * st_facenet_output_fetch copies them.  One device-to-host copy here (the counts), one in the fetch, whatever n is; the
 * call returns with the stream synchronised.  n = 0 is a successful no-op.  ST_ERR_INVALID: n < 0, a null argument or
 * row, a geometry st_facenet_geometry refuses, a threshold, overlap or offset that is not finite.  Exponentials are
 * evaluated in float64 on the device and rounded: the correctly rounded float32 value except where the float64 result lies
 * within its own error of a rounding boundary (known deviation from the reference's expf: DESIGN.md section 4.15). */
int st_facenet_output_batch(st_ctx* ctx, const float* const* maps_dev, int n, int h, int w, float scale, const float* templates,
                            float threshold, float overlap, float offset, int32_t* counts_host);
/* The rows of the context's last st_facenet_output_batch call: rows_host receives 5 floats per kept box; capacity_rows
 * must be at least the sum of that call's counts (ST_ERR_INVALID otherwise, nothing copied). */
int st_facenet_output_fetch(st_ctx* ctx, float* rows_host, int64_t capacity_rows);

/* Greedy non-maximum suppression (Scanner's best_nms, [EXT] restated: DESIGN.md section 4.15) of n independent sets of
 * boxes.  rows_dev: device float32 rows [x1, y1, x2, y2, score], set after set; counts_host[i]: the rows of set i.
 * Boxes are visited by descending score (as unsigned bit patterns, so a NaN score goes first), equal scores by ascending
 * row index.  A visited box that is still valid is kept; it then invalidates every still-valid box i, itself included,
 * unless ov(i) < overlap, with
 *   ov(i) = max(0, (min(x2c, x2i) - max(x1c, x1i)) + o) * max(0, (min(y2c, y2i) - max(y1c, y1i)) + o)
 *           / (((x2i - x1i) + o) * ((y2i - y1i) + o))
 * in float32, min(a, b) = b < a ? b : a and max(a, b) = a < b ? b : a (std::min / std::max: a NaN in b is ignored, in a
 * kept), 0 / 0 = NaN is not below any overlap.  kept_dev: device int32, one slot per input row; the first
 * kept_counts_host[i] slots of set i's range receive the kept boxes' row indices within the set, in kept order.  One
 * workgroup per set sorts in LDS up to 6144 boxes and in global scratch beyond; the result does not depend on the path.
 * The call returns with the stream synchronised (one device-to-host copy).  ST_ERR_INVALID: n < 0, a null argument, a
 * negative count, an overlap or offset that is not finite; ST_ERR_UNSUPPORTED: more than 2^31 - 1 rows in all. */
int st_bbox_nms_f32(st_ctx* ctx, const float* rows_dev, const int32_t* counts_host, int n, float overlap, float offset,
                    int32_t* kept_dev, int32_t* kept_counts_host);

/* ---- Generic Caffe networks (scannertools_caffe: the Caffe and Facenet ops) ---------------------------
 * The layers of a Caffe forward pass (scannertools_caffe_cpp/caffe_kernel.cpp:382) beyond the stride-1 "same" convolutions
 * above.  Layer rules restated from Caffe's public sources ([EXT], unpinned).  Activations are NHWC
 * float32; a call reads c channels from channel x_offset on (x_stride floats per pixel) and writes c channels from y_offset
 * on.  No other channel is read or written: the zero pad channels of a buffer stay zero and never take part.  No result
 * depends on the batch size n: every output element is accumulated in an order fixed by the layer.
 *
 * InnerProduct: y[m][j] = sum_k x[m][k] * W[j][k] (+ bias[j]) (+ ReLU), m < n, j < nout, on v_mfma_f32_32x32x2_f32.  k must be
 * a multiple of 8 (the NHWC-padded length of the bottom blob; W holds zero columns for pad channels).  wp_dev: W rearranged
 * ONCE by st_inner_product_pack_weights from the row-major [nout][k] float32 tensor into a 16-byte aligned buffer of
 * st_inner_product_packed_bytes(k, nout) bytes.  The weights are streamed once per 32 rows of x; the sum over k is cut into
 * chunks of 512 whose partial sums are added in ascending order.  bias_dev may be null.  Row m of y starts at y_dev + m *
 * y_stride; columns >= nout are not written. */
long long st_inner_product_packed_bytes(int k, int nout);
int st_inner_product_pack_weights(st_ctx* ctx, const float* w_dev, int k, int nout, void* out_dev);
int st_inner_product_f32(st_ctx* ctx, const float* x_dev, int n, int k, int x_stride, const void* wp_dev, const float* bias_dev,
                         int nout, int relu, float* y_dev, int y_stride);
/* Output sizes of one axis, host only: Convolution floor((size + 2 pad - k) / stride) + 1; Pooling ceil((size + 2 pad - k) /
 * stride) + 1, less one when pad > 0 and the last window would start in the padding.  0 for arguments Caffe refuses. */
int st_conv_out_size(int size, int k, int stride, int pad);
int st_pool_out_size(int size, int k, int stride, int pad);
/* Convolution of any square kernel, stride, pad and group (+ bias, may be null) (+ ReLU): the correctness path for the
 * geometries st_conv2d_nhwc_f32 does not take.  w_dev: [cout][k][k][cin / group]; each output is one fmaf chain over (ky, kx,
 * channel). */
int st_conv2d_general_nhwc_f32(st_ctx* ctx, const float* x_dev, int n, int h, int w, int cin, int x_stride, int x_offset,
                               const float* w_dev, const float* bias_dev, int k, int stride, int pad, int group, int cout,
                               int relu, float* y_dev, int y_stride, int y_offset);
/* Pooling: window [o * stride - pad, min(o * stride - pad + k, size + pad)) per axis, clipped to the map; ST_POOL_MAX over the
 * clipped window, ST_POOL_AVE its sum divided by the UNCLIPPED window's size.  global: one window, the whole map (k, stride,
 * pad ignored). */
enum { ST_POOL_MAX = 0, ST_POOL_AVE = 1 };
int st_pool_nhwc_f32(st_ctx* ctx, const float* x_dev, int n, int h, int w, int c, int x_stride, int x_offset, int method, int k,
                     int stride, int pad, int global, float* y_dev, int y_stride, int y_offset);
/* LRN across channels: x * (k + alpha / local_size * sum x^2)^-beta over channels c - (local_size - 1) / 2 .. c + (local_size
 * - 1) / 2 clipped to [0, c); local_size odd.  pixels = n * h * w. */
int st_lrn_nhwc_f32(st_ctx* ctx, const float* x_dev, long long pixels, int c, int x_stride, int x_offset, int local_size,
                    float alpha, float beta, float k, float* y_dev, int y_stride, int y_offset);
/* Softmax over the c channels of every pixel, the maximum subtracted first. */
int st_softmax_nhwc_f32(st_ctx* ctx, const float* x_dev, long long pixels, int c, int x_stride, int x_offset, float* y_dev,
                        int y_stride, int y_offset);
/* A channel slice copied between two NHWC buffers (Concat where the producers cannot write their slices themselves), with
 * max(x, 0) on the way when `relu` (a ReLU that could not be fused into its producer; x and y may be the same slice). */
int st_copy_channels_nhwc_f32(st_ctx* ctx, const float* x_dev, long long pixels, int c, int x_stride, int x_offset, int relu,
                              float* y_dev, int y_stride, int y_offset);
/* NHWC (n, h, w, x_stride) -> n dense planar (c, h, w) frames, the blob as Caffe lays it out (out_dev: host array of n device
 * pointers). */
int st_nhwc_to_planar_f32(st_ctx* ctx, const float* x_dev, int n, int h, int w, int c, int x_stride, int x_offset,
                          float* const* out_dev);

/* ---- ImageDecoder: baseline JPEG ------------------------------------------------------------
 * Replaces the reference's ImageDecoder kernels (scannertools_cpp/imgproc/image_decoder_kernel_cpu.cpp: cv::imdecode(
 * IMREAD_UNCHANGED) + BGR->RGB on a thread pool; image_decoder_kernel_gpu.cpp: cv::cudacodec, JPEG only).  Entropy decoding
 * runs on host threads, dequantisation / inverse DCT / chroma upsampling / colour conversion in HIP kernels; the result is
 * bit-exact to libjpeg(-turbo) at its defaults (JDCT_ISLOW, fancy upsampling, RGB output), which is what cv::imdecode calls.
 * Supported: SOF0 (baseline sequential Huffman, 8-bit samples, 8-bit quantisation tables), one scan, with 1 component or with
 * 3 YCbCr components at luma sampling 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and chroma 1x1; restart intervals, APPn / COM
 * segments and fill bytes are handled, EXIF orientation is not applied (IMREAD_UNCHANGED does not).  ST_ERR_UNSUPPORTED:
 * progressive, extended, lossless, hierarchical and arithmetic-coded streams, other precisions, 16-bit quantisation tables,
 * 4 components, an Adobe transform other than YCbCr, any other sampling, several scans.  ST_ERR_INVALID: anything malformed,
 * truncated or not a JPEG.  Known deviation on corrupt input only: samples are clamped to 0..255 where libjpeg's range table
 * wraps (dequantised coefficients no encoder produces). */
typedef struct st_jpeg_info {
  int h, w, channels;   /* channels: 1 or 3 = the decoded frame's (h, w, channels) */
  int h_samp, v_samp;   /* luma sampling factors: 1,1 (4:4:4 and one-component streams), 2,1 (4:2:2), 2,2 (4:2:0) */
  int restart_interval; /* MCUs between RSTn markers; 0: none */
  char message[160];    /* what is wrong with the stream when the status is not ST_OK; empty otherwise */
} st_jpeg_info;
/* Host only (no context, no GPU): parses the markers up to the scan.  Re-entrant. */
int st_jpeg_probe(const uint8_t* buf, size_t size, st_jpeg_info* info);
/* Host only: stage 1 alone (marker parser + Huffman decoder), for tests and tools.  coef receives int16 coefficients as
 * stored in the stream (not dequantised), 64 per 8 x 8 block in natural (row-major) order; the blocks of component 0 first,
 * then component 1, then 2, each component's blocks in raster order of its block-padded plane: ceil(w / (8 H)) H_c blocks
 * per row and ceil(h / (8 V)) V_c block rows, (H, V) the luma sampling and (H_c, V_c) the component's (a one-component
 * stream: ceil(w / 8) x ceil(h / 8)).  cap: the number of int16 behind coef; too few is ST_ERR_INVALID with nothing decoded.
 * quant (may be null): channels x 64 uint16, each component's quantisation table in natural order.  info (may be null)
 * receives the probe's fields and the message. */
int st_jpeg_coefficients(const uint8_t* buf, size_t size, int16_t* coef, size_t cap, uint16_t* quant, st_jpeg_info* info);
/* n streams in HOST memory -> n dense (h, w, channels) uint8 frames in DEVICE memory (out_dev: host array of n device
 * pointers), R, G, B order (the reference's BGR->RGB after imdecode) or one channel.  Every stream is probed first: one that
 * is refused, malformed, or of another shape than (h, w, channels) fails the call -- the message names the stream -- before
 * anything is launched or written.  Then the streams are entropy-decoded on min(n, ST_JPEG_THREADS) host threads (read at
 * each call; default min(16, hardware threads)) into page-locked memory, in sub-batches that alternate between two slots:
 * each sub-batch's coefficients are copied and its two kernels enqueued on the context's stream while the next one is being
 * decoded.  The only host synchronisation is the wait for a slot's previous copy before the slot is refilled.  Subsampling
 * may differ between the streams of a call.  A stream whose entropy-coded data turns out to be corrupt or truncated also
 * fails the call with ST_ERR_INVALID; the frames of its sub-batch and of later ones are then not written, those of
 * sub-batches already enqueued are (a call of at most ST_JPEG_THREADS streams is one sub-batch: nothing is written). */
int st_jpeg_decode_batch(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                         uint8_t* const* out_dev);
/* Host only, re-entrant: the restart intervals of a stream that has a DRI segment, for tests and tools.  An interval is an
 * independently decodable piece of the scan: byte-aligned, DC predictors reset.  *count receives ceil(MCUs / restart_interval);
 * table (may be null: the count alone) receives `count` (begin, end) pairs of byte offsets into buf: interval k's first
 * entropy-coded byte, and the 0xFF of the marker that ends it (after any fill bytes; the end of the buffer where the stream
 * stops without one).  cap: the number of pairs behind table; too few is ST_ERR_INVALID.  The scan is walked once for 0xFF
 * bytes: FF00 and FFFF are data and fill, RSTn must be RST(k mod 8) after interval k, any other marker ends the scan, and
 * what follows the last interval the frame needs is ignored.  ST_ERR_UNSUPPORTED: no DRI segment, or a stream of 4 GiB or
 * more; ST_ERR_INVALID: fewer intervals than the frame needs, a marker out of sequence, and whatever st_jpeg_probe reports.
 * info (may be null) receives the probe's fields and the message. */
int st_jpeg_restart_intervals(const uint8_t* buf, size_t size, uint32_t* table, size_t cap, size_t* count, st_jpeg_info* info);
/* Host only, re-entrant: st_jpeg_coefficients' contract and output layout, computed the way the device computes it: the
 * intervals are scanned as st_jpeg_restart_intervals does and each one is decoded on its own by the bounded core the kernel
 * of st_jpeg_decode_batch_gpu runs (st_jpeg_entropy.h).  The CPU twin of that kernel.  A corrupt interval is ST_ERR_INVALID,
 * the message naming the interval and the cause; a stream without restart intervals is ST_ERR_UNSUPPORTED. */
int st_jpeg_coefficients_by_interval(const uint8_t* buf, size_t size, int16_t* coef, size_t cap, uint16_t* quant, st_jpeg_info* info);
/* st_jpeg_decode_batch with the entropy decoding on the device too, for streams that have restart intervals (every stream
 * st_jpeg_encode_batch writes; Pillow's restart_marker_rows / restart_marker_blocks; libjpeg's -restart).  Same arguments,
 * same frames byte for byte.  Every stream is probed first with the same refusals and messages; a stream without a DRI
 * segment fails the call with ST_ERR_UNSUPPORTED naming it.  The intervals are then scanned on min(n, ST_JPEG_THREADS) host
 * threads, and any scan error fails the call before anything is launched or written.  Per sub-batch ONE copy from page-locked
 * memory carries the Huffman tables (per frame, as its scan selects them), the interval table, the entropy-coded bytes of
 * every stream (16-byte aligned, padded by 16) and the frame headers; k_jpeg_entropy_dec (one lane per restart interval,
 * each lane zeroing its blocks before it fills them) writes the coefficients into device memory where the inverse DCT reads
 * them.  A sub-batch holds at most 2 GiB of coefficients (unless one frame has more).  After a sub-batch's entropy launch
 * the call waits for its status word -- one host wait per sub-batch -- and launches the inverse DCT and colour kernels only
 * when it is clean: a corrupt interval fails the call with ST_ERR_INVALID, the message naming the lowest (stream, interval)
 * that failed and the cause; the frames of that sub-batch and of later ones are not written. */
int st_jpeg_decode_batch_gpu(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                             uint8_t* const* out_dev);

/* ---- Huffman decoding by subsequence: streams with or without restart intervals ----
 * A SEGMENT is a byte range that is decoded from a known state: a restart interval, or the whole scan of a stream without a
 * DRI segment.  A segment is cut into subsequences of subseq_bytes raw bytes; each is decoded on its own from a guessed state,
 * then again from the exit state of the one before it, round after round, until a round changes no exit state: every
 * subsequence has then verified that it entered where its predecessor left, and the chain is the sequential decoder's.  Only
 * then are coefficients written.  max_rounds caps the rounds; a segment that has not converged by then is decoded by the
 * interval decoder in one piece.  0 in either field, or a null pointer, means the library's default (128 bytes, 64 rounds);
 * subseq_bytes must be a multiple of 8 in 8..4096, max_rounds must not be negative. */
typedef struct st_jpeg_split_opts { int subseq_bytes; int max_rounds; } st_jpeg_split_opts;
/* Host only, re-entrant: the segment table of any baseline stream this library decodes, in st_jpeg_restart_intervals' terms
 * (count, cap, (begin, end) pairs, info).  With a DRI segment it is that function's table; without one it is ONE segment from
 * the first entropy-coded byte to the first marker that is neither FF00 nor a fill byte (the end of the buffer where there is
 * none).  Refusals and messages are st_jpeg_probe's. */
int st_jpeg_scan_segments(const uint8_t* buf, size_t size, uint32_t* table, size_t cap, size_t* count, st_jpeg_info* info);
/* Host only, re-entrant: st_jpeg_coefficients' contract and output layout, computed by the iteration above with the bounded
 * core the kernels of st_jpeg_decode_batch_gpu_split run (st_jpeg_entropy.h): their CPU twin.  *rounds (may be null) receives
 * the rounds that changed an exit state, the most over the segments, or max_rounds when a segment fell back to the interval
 * decoder.  A corrupt segment is ST_ERR_INVALID, the message naming the segment and the cause. */
int st_jpeg_coefficients_by_subsequence(const uint8_t* buf, size_t size, const st_jpeg_split_opts* opts, int16_t* coef, size_t cap,
                                        uint16_t* quant, st_jpeg_info* info, int* rounds);
/* st_jpeg_decode_batch with the entropy decoding on the device by subsequence: same arguments, same frames byte for byte, for
 * every stream st_jpeg_decode_batch accepts, with or without restart intervals, mixed in one call.  The upload is
 * st_jpeg_decode_batch_gpu's (one copy per sub-batch) with a prefix table of subsequence counts per frame.  Per sub-batch:
 * round launches (one lane per subsequence, up to 16 rounds per launch inside a workgroup, a count of changed exit states per
 * launch), a segmented scan of block counts and DC sums, a launch that zeroes the coefficients, the write launch, and the
 * interval decoder for segments that did not converge within max_rounds launches; then the inverse DCT and colour kernels.
 * The host waits once per group of round launches (three, then two at a time) and once for the status word: two waits for a
 * sub-batch that converges within two launches.  A corrupt segment fails the call with ST_ERR_INVALID, the message naming the
 * lowest (stream, segment) -- "restart interval k of n", or "the scan" -- and the cause; the frames of that sub-batch and
 * of later ones are not written. */
int st_jpeg_decode_batch_gpu_split(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                                   uint8_t* const* out_dev, const st_jpeg_split_opts* opts);
/* The rounds st_jpeg_decode_batch_gpu_split's last call on this context took: round launches, the most over its sub-batches. */
int st_jpeg_split_last_rounds(st_ctx* ctx);

/* ---- ImageDecoder at a reduced scale: 1/2, 1/4, 1/8 ----
 * libjpeg's scaled decoding (scale_num / scale_denom = 1 / d), bit-exact with libjpeg-turbo: what cv::imdecode returns for
 * IMREAD_REDUCED_COLOR_2 / _4 / _8 (IMREAD_REDUCED_GRAYSCALE_* for a one-component stream) and Pillow after Image.draft().
 * Every coefficient is still entropy-decoded; each component's blocks go through an inverse DCT of S = 1, 2, 4 or 8 samples
 * a side instead of 8, and the frame written is (ceil(h / d), ceil(w / d), channels). */
/* Host only: the size of an (h, w) frame decoded at 1 / scale_denom.  ST_ERR_INVALID: a denominator other than 1, 2, 4 or 8, a
 * size outside 1..65 535, a null pointer. */
int st_jpeg_scaled_size(int h, int w, int scale_denom, int* oh, int* ow);
/* Host only, re-entrant: per component (entries behind `channels` are 0) the inverse DCT size S libjpeg's rule gives it at
 * this scale -- from 8 / d, doubled while the component's remaining upsampling factor stays whole both ways: 4:2:0 chroma gets
 * twice the luma's size and is never upsampled, 4:2:2 chroma the luma's and is still upsampled 2:1 horizontally -- and the
 * extent dw x dh of its reduced plane in samples.  Refusals and messages are st_jpeg_probe's; a bad denominator or a null
 * array is ST_ERR_INVALID.  info may be null. */
int st_jpeg_scaled_geometry(const uint8_t* buf, size_t size, int scale_denom, int S[3], int dw[3], int dh[3], st_jpeg_info* info);
/* Where st_jpeg_decode_batch_scaled decodes the Huffman codes: what st_jpeg_decode_batch, st_jpeg_decode_batch_gpu and
 * st_jpeg_decode_batch_gpu_split do. */
enum { ST_JPEG_ENTROPY_HOST = 0, ST_JPEG_ENTROPY_INTERVAL = 1, ST_JPEG_ENTROPY_SUBSEQUENCE = 2 };
/* The call `entropy` names, writing the frames at 1 / scale_denom: h and w are the streams' own size, out_dev holds n device
 * pointers to (ceil(h / d), ceil(w / d), channels) frames; opts is read for ST_JPEG_ENTROPY_SUBSEQUENCE only.  Refusals,
 * messages, sub-batches, status words and the order of errors are those of the call it stands for, and with scale_denom = 1 it
 * is that call.  A denominator other than 1, 2, 4 or 8, or an unknown `entropy`, is ST_ERR_INVALID naming the value before
 * anything is launched or written. */
int st_jpeg_decode_batch_scaled(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                                int scale_denom, int entropy, const st_jpeg_split_opts* opts, uint8_t* const* out_dev);

/* ---- ImageEncoder: baseline JPEG ------------------------------------------------------------
 * The counterpart of the ImageDecoder block (Scanner's stdlib ImageEncoder wraps cv::imencode on the host; it is not part of
 * the reference tree).  Resident (h, w, 3) uint8 frames in R, G, B order become baseline JPEG streams; colour conversion,
 * chroma downsampling, forward DCT, quantisation AND the Huffman coding run in HIP kernels, so only the compressed streams
 * cross to the host.  A stream is, byte for byte, what libjpeg(-turbo) writes for the same picture at the same quality and
 * sampling with JDCT_ISLOW, the standard (Annex K) Huffman tables and one restart interval per MCU row (Pillow:
 * save(quality=q, subsampling=s, restart_marker_rows=1)): SOI, JFIF APP0, DQT luma, DQT chroma, SOF0, four DHT, DRI (= MCUs
 * per row), SOS, the scan with RST0..7 cycling between MCU rows, EOI.  Three YCbCr components, one interleaved scan, luma
 * sampling h_samp x v_samp = 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0), chroma 1x1.  DESIGN.md section 4.16 restates the
 * arithmetic.  Optimised Huffman tables are opt-in (st_jpeg_encode_batch_opt below).  Not written: grayscale or 4-channel frames, progressive
 * streams, EXIF / ICC.
 *
 * Host only (no context, no GPU), re-entrant: */
/* The quantisation tables of `quality` (1..100) in natural (row-major) order: the Annex K tables scaled as libjpeg's
 * jpeg_set_quality with force_baseline does.  ST_ERR_INVALID: quality out of range, a null pointer. */
int st_jpeg_quant_tables(int quality, uint16_t luma[64], uint16_t chroma[64]);
/* The stream's bytes from SOI up to and including SOS (629 for every stream this encoder writes) into buf[0, cap); *size (may
 * be null) receives their number whenever the other arguments are valid.  ST_ERR_INVALID: quality outside 1..100, h or w
 * outside 1..65535, buf null or cap too small; ST_ERR_UNSUPPORTED: another sampling. */
int st_jpeg_encode_header(int h, int w, int quality, int h_samp, int v_samp, uint8_t* buf, size_t cap, size_t* size);
/* An upper bound of a stream's bytes whatever the picture and quality: the header, 416 bytes per coded 8 x 8 block (padding
 * blocks included: 1660 bits of codes at most, every byte stuffed), the RST markers and EOI.  -1 for arguments
 * st_jpeg_encode_header refuses. */
long long st_jpeg_encode_bound(int h, int w, int h_samp, int v_samp);
/* frames_dev: host array of n device pointers to dense (h, w, 3) uint8 frames, any alignment.  Enqueues the encoder's four
 * launches on the context's stream and returns without waiting (it waits only where its buffers have to grow, or for the upload
 * of new tables when h, w, quality or sampling differ from the last call's); the streams stay in a buffer of the context until its next
 * st_jpeg_encode_batch call, st_jpeg_encode_fetch copies them.  Refused before anything is launched, the message naming the
 * cause: ST_ERR_INVALID for n < 0, quality outside 1..100, h or w outside 1..65535, a null table or frame pointer;
 * ST_ERR_UNSUPPORTED for a sampling other than 1x1, 2x1, 2x2 and for more than 2^31 - 1 MCU rows in all.  n = 0 is a successful
 * no-op.  Device memory of a call: 128 bytes of coefficients and 2 x 416 bytes of stream space per coded block. */
int st_jpeg_encode_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int quality, int h_samp, int v_samp);
/* The streams of the context's last st_jpeg_encode_batch call.  sizes[i] receives stream i's bytes; bufs_host: n host buffers of
 * `capacity` bytes each, or null to learn the sizes alone.  One wait for the kernels, with the copy of the stream offsets;
 * then all streams come in ONE device-to-host copy of exactly their bytes and are handed out on the host.  ST_ERR_INVALID: no
 * call to fetch from, sizes null, a null buffer, a stream longer than capacity (sizes is filled in all the same, nothing is
 * copied). */
int st_jpeg_encode_fetch(st_ctx* ctx, uint8_t* const* bufs_host, size_t* sizes, size_t capacity);
/* Where the stream has restart markers.  ROW: one restart interval per MCU row, everything said above; what
 * st_jpeg_encode_header and st_jpeg_encode_batch write.  NONE: no DRI segment and no RSTn markers, the stream libjpeg writes
 * with restart_interval = 0, its default and that of cv::imencode, Pillow (save(quality=q, subsampling=s)) and cjpeg: the 623
 * header bytes (the 629 without the DRI segment), ONE scan whose DC predictors carry over from MCU row to MCU row, whose last
 * byte is padded with 1-bits and in which every 0xFF byte -- also one made of the bits of two MCU rows -- is followed by 0x00,
 * then EOI.  Everything before the entropy coder is the same.  DESIGN.md section 4.16b. */
enum { ST_JPEG_RESTART_ROW = 0, ST_JPEG_RESTART_NONE = 1 };
/* st_jpeg_encode_header for either mode (ROW: the same bytes).  ST_ERR_INVALID also for any other `restart`. */
int st_jpeg_encode_header_rst(int h, int w, int quality, int h_samp, int v_samp, int restart, uint8_t* buf, size_t cap, size_t* size);
/* st_jpeg_encode_batch for either mode (ROW: the same launches, bytes and messages).  NONE enqueues five launches -- transform,
 * entropy coding of each MCU row into its slot unpadded and unstuffed, a count of the 0xFF bytes each row owns once the rows are
 * joined bit by bit, the layout, the pack that shifts, joins, stuffs and writes them -- and like ROW has no workgroup wait for
 * another.  Any other `restart` is ST_ERR_INVALID, the message naming the value, before anything is launched or uploaded.
 * st_jpeg_encode_fetch and st_jpeg_encode_bound serve both modes (the bound covers the shorter stream); the device memory per
 * coded block is the same. */
int st_jpeg_encode_batch_rst(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int quality, int h_samp, int v_samp,
                             int restart);

/* ---- ImageEncoder with optimised Huffman tables ----
 * libjpeg's optimize_coding (Pillow: optimize=True; cjpeg -optimize): each frame's four Huffman tables are built from the
 * frame's own symbol counts, on the device, and the stream is byte for byte what libjpeg-turbo writes at JDCT_ISLOW with
 * optimize_coding = TRUE at the same quality, sampling and restart mode.  Only the four DHT segments and the scan coded with
 * them differ from the streams above.
 *
 * Host only, re-entrant: jpeg_gen_optimal_table.  freq: the counts of symbols 0 .. 255 (the reserved pseudo-symbol is added
 * inside); bits[k]: the codes of k + 1 bits; vals: the *nvals symbols that have a code, by code length, then by value.
 * ST_ERR_INVALID: a null pointer.  ST_ERR_UNSUPPORTED: a code would have more than 32 bits before the limiting to 16 (counts that
 * grow like Fibonacci numbers over 34 symbols or more), where libjpeg stops with JERR_HUFF_CLEN_OVERFLOW; bits and vals then
 * hold a valid table of 9- and 10-bit codes, which is what the device path encodes such a frame with. */
int st_jpeg_optimal_table(const uint64_t freq[256], uint8_t bits[16], uint8_t vals[256], int* nvals);
/* Host only: the DHT segment (marker included, 21 + nvals bytes) of the table st_jpeg_optimal_table builds from freq, as table
 * `table` = 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma (the order of the segments in the stream); *size (may be null) receives
 * the bytes whenever freq and table are valid; codes (may be null): 16 (DC) or 256 (AC) words (code length << 16) | code by
 * symbol, 0 for a symbol without a code.  ST_ERR_INVALID: a null freq, another table, buf null or cap too small. */
int st_jpeg_optimal_dht(const uint64_t freq[256], int table, uint8_t* buf, size_t cap, size_t* size, uint32_t* codes);
/* Host only: the 4 x 256 symbol counts (tables in the order above) of an (h, w, 3) frame's coefficients in st_jpeg_coefficients'
 * layout, `cap` int16 behind coef: what jchuff's htest_one_block counts -- the DC category of each block's difference to its
 * component's previous block, 0xF0 per run of 16 zeros, (run << 4) | size per non-zero coefficient, 0x00 where a block ends in
 * zeros --, the DC predictors reset at each MCU row for ST_JPEG_RESTART_ROW and kept for ST_JPEG_RESTART_NONE.  The CPU twin of
 * k_jpeg_sym_stats.  Refusals as st_jpeg_encode_header_rst; too few coefficients or a null pointer is ST_ERR_INVALID. */
int st_jpeg_symbol_stats(const int16_t* coef, size_t cap, int h, int w, int h_samp, int v_samp, int restart, uint64_t freq[1024]);
/* st_jpeg_encode_bound for streams written with optimize = 1: 418 bytes per coded block (any table of codes up to 16 bits: 1665
 * bits at most, every byte stuffed); the header is never longer than the 629 bytes (at most 12 DC and 162 AC symbols occur). */
long long st_jpeg_encode_bound_opt(int h, int w, int h_samp, int v_samp);
/* st_jpeg_encode_batch_rst with `optimize`.  0: that call exactly -- the same launches, bytes and messages.  1: two launches
 * more between the transform and the entropy coder -- k_jpeg_sym_stats counts each frame's symbols into 4 x 256 64-bit counters
 * (zeroed by the call), k_jpeg_opt_tables builds each frame's tables, code words and header -- six launches for
 * ST_JPEG_RESTART_ROW and seven for ST_JPEG_RESTART_NONE, with no host wait between them.  Any other `optimize` is
 * ST_ERR_INVALID, the message naming the value, before anything is launched or uploaded.  st_jpeg_encode_fetch serves the call.
 * Device memory: 128 bytes of coefficients and 2 x 418 bytes of stream space per coded block, 11 KiB per frame. */
int st_jpeg_encode_batch_opt(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int quality, int h_samp, int v_samp,
                             int restart, int optimize);
/* The symbol counts of the context's last st_jpeg_encode_batch_opt(optimize = 1) call, for tests and tools: n x 1024 counters
 * (st_jpeg_symbol_stats' layout per frame) into freq[0, cap).  One wait for the kernels.  ST_ERR_INVALID: no such call to fetch
 * from, freq null, cap < n x 1024. */
int st_jpeg_encode_fetch_stats(st_ctx* ctx, uint64_t* freq, size_t cap);

/* ---- ImageDecoder: PNG (opt-in, ImageDecoderArgs.png = DECODE) ----------------------------------
 * cv::imdecode(IMREAD_UNCHANGED) reads PNG as readily as JPEG (image_decoder_kernel_cpu.cpp).  Inflate is serial per stream and
 * runs on host threads with the library's own inflater (no zlib, no libpng); undoing the row filters and expanding palette
 * indices, sub-byte samples, gray+alpha and colour-key transparency run in HIP kernels.  Decoded: colour type 0 at bit depth
 * 1 / 2 / 4 / 8 -> 1 channel (depth 1 / 2 / 4 scaled by 255 / 85 / 17, tRNS ignored); 2 at 8 -> R, G, B, with tRNS R, G, B, A
 * (A = 0 where the pixel equals the key, else 255); 3 at 1 / 2 / 4 / 8 -> R, G, B, with tRNS R, G, B, A (entries past tRNS
 * have A = 255; an index past the palette is opaque black); 4 at 8 -> g, g, g, a; 6 at 8 -> R, G, B, A.  That restates
 * OpenCV's PNG reader followed by the reference's BGR(A) -> RGB(A) swap (unpinned: DESIGN.md 4.17).  ST_ERR_UNSUPPORTED:
 * 16-bit samples, Adam7 interlace; of an APNG only the default image is decoded.  ST_ERR_INVALID: anything malformed. */
typedef struct st_png_info {
  int h, w, channels;            /* of the decoded frame */
  int color_type, bit_depth, interlace;
  int palette_entries, trns_entries;   /* 0: no such chunk */
  char message[160];             /* why a stream is refused; empty on ST_OK */
} st_png_info;
/* Host only, re-entrant: reads the signature and the chunks up to the first IDAT (so that `channels` is known), CRCs checked. */
int st_png_probe(const uint8_t* buf, size_t size, st_png_info* info);
/* Host only, re-entrant, for tests and tools: inflates one zlib stream (RFC 1950 / 1951) into dst[0, cap) and never past it;
 * *produced (may be null) receives the bytes written.  ST_ERR_INVALID with the cause in message (may be null): a bad zlib
 * header, block type 3, stored LEN / NLEN mismatch, over-subscribed or incomplete code lengths, invalid length or distance
 * symbols, a distance before the start of the output, truncated input, more output than cap, Adler-32 mismatch. */
int st_zlib_inflate(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* produced, char* message, size_t message_len);
/* Host only, re-entrant: stage 1 alone -- the whole container is parsed and checked, the IDAT chunks are joined and inflated
 * into raw[0, cap): h x (1 + rowbytes) bytes, every row its filter type and its still-filtered bytes.  cap too small, an
 * inflated length other than exactly that, or a filter type above 4 is ST_ERR_INVALID.  The twin of st_jpeg_coefficients. */
int st_png_filtered(const uint8_t* buf, size_t size, uint8_t* raw, size_t cap, st_png_info* info);
/* Host only, re-entrant: the whole decode in plain C++, the way the device computes it: frame[0, cap) receives the
 * (h, w, channels) frame.  The CPU twin of k_png_unfilter + k_png_expand. */
int st_png_decode_host(const uint8_t* buf, size_t size, uint8_t* frame, size_t cap, st_png_info* info);
/* st_jpeg_decode_batch's contract for PNG streams: every stream is probed and its container checked first (all but the CRCs of
 * the IDAT chunks, which belong to the data), and one that is refused, malformed or of another decoded shape than
 * (h, w, channels) fails the call naming it before anything is launched or written.  Then the streams are inflated on min(n, ST_PNG_THREADS) host threads (default and clamping as ST_JPEG_THREADS)
 * into page-locked memory in sub-batches that alternate between two slots; each sub-batch is copied and its launches
 * (k_png_unfilter: one workgroup per frame; k_png_expand where a frame needs it) enqueued on the context's stream while the
 * next is inflated; the only host wait is the one for a slot's previous copy.  Streams of different colour types and depths
 * may share a call when they decode to the same shape.  A stream whose data turns out corrupt (an IDAT CRC, the zlib stream, the
 * inflated length, a filter type) fails the call under
 * st_jpeg_decode_batch's rule: later sub-batches are not written, enqueued ones are.  out_dev: n device pointers to
 * (h, w, channels) frames at any byte address.  Timed under ST_K_JPEG. */
int st_png_decode_batch(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                        uint8_t* const* out_dev);

/* ---- ImageEncoder: PNG (opt-in, ImageEncoderArgs.format = PNG) -----------------------------------
 * Lossless streams of (h, w, c) uint8 frames, c = 1 (gray), 3 (R, G, B) or 4 (R, G, B, A): colour types 0, 2, 6 at bit depth
 * 8, not interlaced, no ancillary chunks.  Rows are filtered on the device (k_png_filter), the filtered bytes are cut into
 * pieces of 32 768 that are deflated independently (k_png_deflate: runs as distance-1 matches, one dynamic-Huffman block per
 * piece, stored where that is not shorter), every piece is one IDAT chunk, and a last IDAT carries the final empty block and
 * the Adler-32.  The bytes are defined by tests/ref_png_encode_np.py; any PNG reader decodes them. */
enum { ST_PNG_FILTER_NONE = 0, ST_PNG_FILTER_SUB = 1, ST_PNG_FILTER_UP = 2, ST_PNG_FILTER_AVERAGE = 3, ST_PNG_FILTER_PAETH = 4,
       ST_PNG_FILTER_ADAPTIVE = 5 };   /* ADAPTIVE: per row the type with the least sum of min(b, 256 - b), ties to the lowest */
/* Host only.  ST_OK, or ST_ERR_INVALID with the refusal's words in msg (may be null): c outside {1, 3, 4}, a size outside
 * 1..65535, a filter outside the enum. */
int st_png_encode_check(int h, int w, int c, int filter, char* msg, size_t msg_len);
/* Host only.  No stream of an (h, w, c) frame is longer: every piece stored.  -1 for what st_png_encode_check refuses. */
long long st_png_encode_bound(int h, int w, int c);
/* Host only, re-entrant: the stream of one dense host frame in plain C++, byte for byte what st_png_encode_batch writes.  *size
 * receives its bytes; buf may be null for the size alone, else cap must hold it (ST_ERR_INVALID). */
int st_png_encode_host(const uint8_t* frame, int h, int w, int c, int filter, uint8_t* buf, size_t cap, size_t* size);
/* Host only, for tests: the encoder's length-limited code construction on any histogram.  counts[symbols] (2 <= symbols <= 286,
 * their sum below 2^32), limit 1..15 with 2^limit >= symbols -> lengths[symbols], 0 for a symbol without a code.  The code is
 * complete; with fewer than two counted symbols the lowest-numbered others receive a code too. */
int st_png_huff_limited(const uint32_t* counts, int symbols, int limit, uint8_t* lengths);
/* n device frames (h, w, c), dense, at any byte address -> n streams kept on the device until the context's next
 * st_png_encode_batch call; st_png_encode_fetch copies them.  Refused before anything is launched, written or uploaded, with
 * the context's previous streams still fetchable: n < 1, what st_png_encode_check refuses, a null table or frame, more than
 * 2^31 - 1 rows or pieces in the call.  Four launches -- filter, deflate, layout, pack --, timed under ST_K_JPEG. */
int st_png_encode_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int c, int filter);
/* The streams of the context's last st_png_encode_batch call, with st_jpeg_encode_fetch's contract: sizes[i] receives stream
 * i's bytes; bufs_host may be null for the sizes alone, else n host buffers of `capacity` bytes each.  One copy of the packed
 * streams; the host does not touch their bytes otherwise. */
int st_png_encode_fetch(st_ctx* ctx, uint8_t* const* bufs_host, size_t* sizes, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* SCANNERTOOLS_HIP_H_ */
