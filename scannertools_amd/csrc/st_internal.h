// Internal declarations shared by the translation units of libscannertools_hip.so.
#ifndef ST_INTERNAL_H_
#define ST_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "scannertools_hip.h"

#define ST_EXPORT extern "C" __attribute__((visibility("default")))

struct st_timing_slot {
  std::vector<hipEvent_t> starts, stops;  // pooled events, one pair per recorded launch
  size_t used = 0;
  int launches = 0;
  double total_ms = 0.0;
};

struct st_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // flow-iteration kernel choice for small launches (ST_ITER_TILE, read when the context is created):
  // -1 by total size (default), 0 never the tile kernel, 1 always.  The two kernels agree bit for
  // bit, so this is a scheduling switch only.
  int tile_mode = -1;
  bool poly_u8 = true;     // level-0 expansion straight from the gray frames (k_polyexp_u8), level 0 left out of the pyramid pass; ST_POLY_U8=0: float source
  bool fold_gray = false;  // ST_PYR_FOLD_GRAY=1: luma conversion inside the one-pass pyramid (slower; A/B switch)
  // role-split kernels (scheduling switches like tile_mode, read when the context is created; results do not depend on them):
  // ST_ITER_ROLES / ST_PYR_ROLES: -1 by launch size (default), 0 never, 1 always; ST_ROLES_NCW: 0 = by cost, 4 or 5 column waves
  int roles_mode = -1, roles_ncw = 0, pyr_roles = -1;
  bool pyr_roles_rgb = true;  // ST_PYR_ROLES_RGB=0: large calls run the separate luma pass (k_gray4) ahead of the role-split pyramid instead of its RGB-source instance
  int conv_tile = -1;   // ST_CONV_TILE: 0 = bf16x3 convolutions always on the per-tap kernel (st_conv.hip)
  // Concurrent kernel instances (Scanner's pipeline_instances_per_node: K contexts of one process on one GPU, each call followed
  // by st_ctx_sync).  flow_busy: an OpticalFlow call of this context has been enqueued and not yet synchronised; flow_enter_ns:
  // when (steady clock).  st_flow_call_begins() reads the other contexts' to pick kernels that share the chip (st_context.hip).
  std::atomic<bool> flow_busy{false};
  std::atomic<long long> flow_enter_ns{0};
  bool flow_concurrent = false;   // decided at the entry of the current st_farneback_pairs call
  int concurrency_mode = -1;      // ST_CONCURRENT: -1 detect (default), 0 never assume, 1 always assume other instances
  // bump-allocated scratch
  void* ws = nullptr;
  size_t ws_bytes = 0;
  size_t ws_limit = (size_t)64 << 30;
  size_t ws_off = 0;
  // small device table for pointer arrays
  unsigned timing_mask = 0;
  st_timing_slot timing[ST_K_COUNT];
  std::string last_error;
  int num_cus = 256;
  struct st_jpeg_state* jpeg = nullptr;   // page-locked slots of st_jpeg_decode_batch (st_jpeg.hip), made at its first call
  struct st_netin_state* netin = nullptr; // per-geometry tables of the FacenetInput / CaffeInput entry points (st_netinput.hip)
  struct st_detect_state* detect = nullptr; // the kept rows of the last st_facenet_output_batch call (st_detect.hip)
  struct st_png_state* png = nullptr;     // page-locked slots of st_png_decode_batch (st_png.hip), made at its first call
  struct st_jpeg_enc_state* jpeg_enc = nullptr; // tables and the packed streams of the last st_jpeg_encode_batch call (st_jpeg_enc.hip)
  struct st_png_enc_state* png_enc = nullptr;   // the packed streams of the last st_png_encode_batch call (st_png_enc.hip)
};
void st_jpeg_release(st_ctx* ctx);   // frees ctx->jpeg (st_ctx_destroy)
struct StJpegEntArgs;
// enqueues k_jpeg_entropy_dec (st_jpeg_entropy.hip) for one sub-batch of st_jpeg_decode_batch_gpu; max_groups: the most
// groups of 64 restart intervals any of its frames has
int st_jpeg_entropy_launch(st_ctx* ctx, const StJpegEntArgs& a, unsigned max_groups);
struct StJsqArgs;
// st_jpeg_subseq.hip, for one sub-batch of st_jpeg_decode_batch_gpu_split.  max_groups: the most groups of 64 subsequences any of
// its frames has; max_segments: the most segments.  A round launch (k_jsq_round) reads the exit states of array par ^ 1 and
// writes array par, and adds the exits it changed to *changed (device memory); `first`: no state exists yet.  The finishing
// launches: k_jsq_scan over array par, k_jsq_zero over coef_bytes of coefficients, k_jsq_write, k_jsq_fallback.
int st_jsq_round_launch(st_ctx* ctx, const StJsqArgs& a, unsigned max_groups, bool first, int par, unsigned* changed);
int st_jsq_finish_launch(st_ctx* ctx, const StJsqArgs& a, unsigned max_groups, unsigned max_segments, int par, size_t coef_bytes);
void st_png_release(st_ctx* ctx);    // frees ctx->png (st_ctx_destroy)
void st_jpeg_enc_release(st_ctx* ctx); // frees ctx->jpeg_enc (st_ctx_destroy)
void st_png_enc_release(st_ctx* ctx);  // frees ctx->png_enc (st_ctx_destroy)
void st_netin_release(st_ctx* ctx);  // frees ctx->netin (st_ctx_destroy)
void st_detect_release(st_ctx* ctx); // frees ctx->detect (st_ctx_destroy)

int st_set_error(st_ctx* ctx, int status, const char* fmt, ...);

#define ST_HIP(ctx, expr)                                                                   \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return st_set_error((ctx), ST_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                \
                          hipGetErrorString(_e), __FILE__, __LINE__);                       \
  } while (0)

#define ST_TRY(expr)              \
  do {                            \
    int _s = (expr);              \
    if (_s != ST_OK) return _s;   \
  } while (0)

// Enter an API call: null check + select device.
int st_enter(st_ctx* ctx);

// The checks a batch decoder begins with (codec: "jpeg" or "png"; channels_ok: bit c set where c channels can be asked
// for).  The caller then returns ST_OK itself when n is 0.
inline int st_decode_args(st_ctx* ctx, const char* codec, int n, int h, int w, int channels, unsigned channels_ok, const void* bufs_host,
                          const void* sizes, const void* out_dev) {
  if (n < 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535 || channels < 0 || channels > 31 || !(channels_ok >> channels & 1))
    return st_set_error(ctx, ST_ERR_INVALID, "%s: bad arguments (n=%d h=%d w=%d channels=%d)", codec, n, h, w, channels);
  if (n > 0 && (!bufs_host || !sizes || !out_dev)) return st_set_error(ctx, ST_ERR_INVALID, "%s: null argument", codec);
  return ST_OK;
}
constexpr const char* kStNoOutputFrame = "%s: stream %d has no output frame";   // (codec, stream), ST_ERR_INVALID

// Grows a page-locked buffer to `bytes` (its contents are not kept); oom_fmt words the failure and may print the size (%zu).
inline int st_pinned_grow(st_ctx* ctx, void** p, size_t* cap, size_t bytes, const char* oom_fmt) {
  if (bytes <= *cap) return ST_OK;
  if (*p) ST_HIP(ctx, hipHostFree(*p));
  *p = nullptr;
  *cap = 0;
  if (hipHostMalloc(p, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return st_set_error(ctx, ST_ERR_OOM, oom_fmt, bytes);
  }
  *cap = bytes;
  return ST_OK;
}

// The two page-locked upload slots of a pipelined decoder (st_host_pipeline.h): sub-batch k is filled into slot k & 1 and
// copied to the device from there.
struct st_pinned_slots {
  void* pin[2] = {nullptr, nullptr};
  size_t cap[2] = {0, 0};
  hipEvent_t copied[2] = {nullptr, nullptr};   // the slot's last copy has left host memory
  bool busy[2] = {false, false};               // a copy was enqueued that `copied` has not been waited for since
  uint8_t* at(int s) const { return static_cast<uint8_t*>(pin[s]); }
};
// A slot is refilled only after its previous copy (of this call or an earlier one) has read it.
inline int st_slot_release(st_ctx* ctx, st_pinned_slots* sl, int s) {
  if (sl->busy[s]) ST_HIP(ctx, hipEventSynchronize(sl->copied[s]));
  sl->busy[s] = false;
  return ST_OK;
}
// The first `count` slots ready to be filled with up to `bytes`.
inline int st_slots_prepare(st_ctx* ctx, st_pinned_slots* sl, int count, size_t bytes, const char* oom_fmt) {
  for (int s = 0; s < count; ++s) {
    if (!sl->copied[s]) ST_HIP(ctx, hipEventCreateWithFlags(&sl->copied[s], hipEventDisableTiming));
    ST_TRY(st_slot_release(ctx, sl, s));
    ST_TRY(st_pinned_grow(ctx, &sl->pin[s], &sl->cap[s], bytes, oom_fmt));
  }
  return ST_OK;
}
// enqueues the copy of a filled slot
inline int st_slot_upload(st_ctx* ctx, st_pinned_slots* sl, int s, void* dst_dev, size_t bytes) {
  ST_HIP(ctx, hipMemcpyAsync(dst_dev, sl->pin[s], bytes, hipMemcpyHostToDevice, ctx->stream));
  ST_HIP(ctx, hipEventRecord(sl->copied[s], ctx->stream));
  sl->busy[s] = true;
  return ST_OK;
}
inline void st_slots_free(st_pinned_slots* sl) {
  for (int s = 0; s < 2; ++s) {
    if (sl->copied[s]) (void)hipEventDestroy(sl->copied[s]);
    if (sl->pin[s]) (void)hipHostFree(sl->pin[s]);
  }
}

// Marks `ctx` as having an OpticalFlow call in flight and says whether TWO OR MORE other contexts of this process have one in
// flight on the same device (entered within the last 50 ms and not synchronised since): then a small launch should not take a
// whole CU per workgroup.  A scheduling decision only -- the kernels it chooses between agree bit for bit.
bool st_flow_call_begins(st_ctx* ctx);

// Scratch: reset at the start of a call, then bump-allocate (256-B aligned).  Grows the
// backing allocation when needed (synchronising the stream first).
int st_ws_reserve(st_ctx* ctx, size_t total_bytes);
void st_ws_reset(st_ctx* ctx);
void* st_ws_alloc(st_ctx* ctx, size_t bytes);  // nullptr if the reservation is exhausted
inline size_t st_align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// ---- The host-side frame of a batched entry point: row checks, pointer tables, launch cuts.
// A kernel that takes its frame index from gridDim.y or gridDim.z serves at most this many frames per launch.
constexpr int kStMaxGridFrames = 65535;

// Cuts a call of n frames into launches: body(f0, nf) -> status for frames f0 .. f0 + nf - 1, nf <= kStMaxGridFrames;
// stops at the first status that is not ST_OK and returns it.
template <class Body>
inline int st_for_launches(int n, Body&& body) {
  for (int f0 = 0; f0 < n; f0 += kStMaxGridFrames) ST_TRY(body(f0, n - f0 < kStMaxGridFrames ? n - f0 : kStMaxGridFrames));
  return ST_OK;
}

// Refuses the lowest row i at which one of the host tables a, b, c (b and c may be absent) holds a null pointer, or, with
// no_alias, at which a[i] == b[i]: ST_ERR_INVALID, with `fmt` taking the row index.
template <class A, class B = void, class C = void>
inline int st_check_rows(st_ctx* ctx, const char* fmt, int n, bool no_alias, A* const* a, B* const* b = nullptr, C* const* c = nullptr) {
  for (int i = 0; i < n; ++i)
    if (!a[i] || (b && !b[i]) || (c && !c[i]) || (no_alias && (const void*)a[i] == (const void*)b[i]))
      return st_set_error(ctx, ST_ERR_INVALID, fmt, i);
  return ST_OK;
}

// Device copies of one to three host tables of n pointers each: reserves the tables' workspace plus `extra` bytes (which
// the caller allocates afterwards), then per (host table, device table out) pair allocates and enqueues the copy on ctx->stream.
inline int st_upload_table(st_ctx*, size_t) { return ST_OK; }
template <class D, class... Rest>
inline int st_upload_table(st_ctx* ctx, size_t bytes, const void* host, D** dev, Rest... rest) {
  if (!(*dev = (D*)st_ws_alloc(ctx, bytes))) return st_set_error(ctx, ST_ERR_OOM, "pointer table: workspace exhausted");
  ST_HIP(ctx, hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return st_upload_table(ctx, bytes, rest...);
}
template <class... Pairs>
inline int st_upload_tables(st_ctx* ctx, int n, size_t extra, Pairs... pairs) {
  const size_t bytes = sizeof(void*) * (size_t)n;
  ST_TRY(st_ws_reserve(ctx, sizeof...(Pairs) / 2 * st_align_up(bytes) + extra));
  return st_upload_table(ctx, bytes, pairs...);
}

// Timing brackets for kernel class `id` (no-ops unless enabled in timing_mask).
int st_time_begin(st_ctx* ctx, int id);
int st_time_end(st_ctx* ctx, int id);
int st_time_dispatch(st_ctx* ctx, int id, hipEvent_t* start, hipEvent_t* stop);   // events for hipExtLaunchKernelGGL (st_context.hip)

// A bracket is closed only if it was opened: when st_time_begin fails (event creation / record) the
// launch simply goes untimed; the failure stays in last_error and the slot's counters are untouched.
struct st_timed {
  st_ctx* ctx;
  int id;
  bool open;
  st_timed(st_ctx* c, int k) : ctx(c), id(k), open(st_time_begin(c, k) == ST_OK) {}
  ~st_timed() { if (open) (void)st_time_end(ctx, id); }
};

// A pointer read from a device-side pointer table (Scanner hands every frame as its own buffer) has no provable
// address space, so loads and stores through it compile to flat_* instructions: those also count on lgkmcnt (an LDS
// wait then waits for them too) and take a 64-bit address in VGPRs.  Everything this library is handed lives in
// global memory; the round trip through address space 1 tells the compiler so (global_* instructions, SGPR base).
#ifdef __HIPCC__
template <class T>
__device__ __forceinline__ T* st_gl(T* p) {
  return (T*)((__attribute__((address_space(1))) T*)(uintptr_t)p);
}
#endif

// ---- cv::resize's INTER_LINEAR arithmetic for 8-bit data, shared by the Resize / Montage kernels (st_imgproc.hip) and the
// SharpnessBBox kernel (st_framestats.hip), so that a box resized inside the statistics kernel cannot drift from the op.
enum { RS_NEAREST = 0, RS_LINEAR = 1, RS_AREA2 = 2, RS_COPY = 3, RS_CUBIC = 4, RS_AREA_INT = 5, RS_AREA = 6, RS_LINEAR_AREA = 7, RS_LANCZOS4 = 8 };

// cv::resize's scale factors for (h, w) -> (out_h, out_w), computed on the host, and the path INTER_LINEAR takes: an equal
// size is a copy (RS_COPY), an exact 2 x 2 decimation the mean of four (RS_AREA2, INTER_AREA's fast path), else RS_LINEAR
struct st_rs_scales {
  double scale_x, scale_y, inv_scale_x, inv_scale_y;
  int iscale_x, iscale_y;
  bool area_fast;   // both ratios are integers
};
st_rs_scales st_rs_plan_scales(int h, int w, int out_h, int out_w);
inline int st_rs_linear_mode(int h, int w, int out_h, int out_w, const st_rs_scales& s) {
  if (h == out_h && w == out_w) return RS_COPY;
  if (s.area_fast && s.iscale_x == 2 && s.iscale_y == 2) return RS_AREA2;
  return RS_LINEAR;
}

#ifdef __HIPCC__
// (coordinates and taps are __host__ __device__: st_netinput.hip tabulates them on the host with the same code)
// saturate_cast<short>(float): cvRound = round half to even, then saturation
__host__ __device__ __forceinline__ int rs_coef(float v) {
  const float r = rintf(v);
  return r < -32768.f ? -32768 : (r > 32767.f ? 32767 : (int)r);
}

// INTER_LINEAR's source coordinate of destination index d: the first tap's index and the fraction towards the second
__host__ __device__ __forceinline__ float rs_linear_coord(int d, double scale, int* s) {
  const float f = (float)((d + 0.5) * scale - 0.5);
  *s = (int)floorf(f);
  return f - *s;
}

// Horizontal taps of one destination column: the column is clamped into the row (a single tap * 2048 at the right edge),
// 11-bit weights.  sx: the first tap's column; two: a second tap exists at sx + 1.
struct RsTapX { int sx, a0, a1; bool two; };
__host__ __device__ __forceinline__ RsTapX rs_linear_tap_x(int sx, float fx, int sw) {
  RsTapX t;
  if (sx < 0) { fx = 0; sx = 0; }
  if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
  t.a0 = rs_coef((1.f - fx) * 2048); t.a1 = rs_coef(fx * 2048);
  t.two = sx + 1 < sw;
  t.sx = sx;
  return t;
}
// Vertical taps of one destination row: both rows clamped into the image
struct RsTapY { int y0, y1, b0, b1; };
__host__ __device__ __forceinline__ RsTapY rs_linear_tap_y(int sy, float fy, int sh) {
  RsTapY t;
  t.b0 = rs_coef((1.f - fy) * 2048); t.b1 = rs_coef(fy * 2048);
  t.y0 = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy);
  t.y1 = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
  return t;
}
// HResizeLinear for one channel of one row (v0, v1: the two taps' bytes) and VResizeLinear<uchar> of the two row values
__device__ __forceinline__ int rs_linear_h(int v0, int v1, int a0, int a1, bool two) { return two ? v0 * a0 + v1 * a1 : v0 * 2048; }
__device__ __forceinline__ int rs_linear_v(int r0, int r1, int b0, int b1) { return (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2; }

// One output pixel of the 3-channel INTER_LINEAR kernels: the two source pixels of a row are 6 contiguous bytes at R + sxo,
// read as two unaligned dwords when `wide` (8 bytes from sxo stay inside the row), bytewise otherwise.  The three output
// bytes go into bytes 3p .. 3p + 2 of out[0..2] (which the caller zeroed).
__device__ __forceinline__ void rs_linear_px_c3(const uint8_t* __restrict__ R0, const uint8_t* __restrict__ R1, int sxo, int a0, int a1, bool two,
                                                bool wide, int b0, int b1, int p, unsigned* out) {
  typedef unsigned u32u __attribute__((aligned(1)));
  int t0[6], t1[6];
  if (wide) {
    const unsigned l0 = *reinterpret_cast<const u32u*>(R0 + sxo), h0 = *reinterpret_cast<const u32u*>(R0 + sxo + 4);
    const unsigned l1 = *reinterpret_cast<const u32u*>(R1 + sxo), h1 = *reinterpret_cast<const u32u*>(R1 + sxo + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) { t0[k] = (l0 >> (8 * k)) & 0xff; t1[k] = (l1 >> (8 * k)) & 0xff; }
    t0[4] = h0 & 0xff; t0[5] = (h0 >> 8) & 0xff; t1[4] = h1 & 0xff; t1[5] = (h1 >> 8) & 0xff;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) { t0[k] = R0[sxo + k]; t1[k] = R1[sxo + k]; }
#pragma unroll
    for (int k = 3; k < 6; ++k) { t0[k] = two ? R0[sxo + k] : 0; t1[k] = two ? R1[sxo + k] : 0; }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int r0 = rs_linear_h(t0[c], t0[3 + c], a0, a1, two);
    const int r1 = rs_linear_h(t1[c], t1[3 + c], a0, a1, two);
    const unsigned v = (unsigned)rs_linear_v(r0, r1, b0, b1) & 0xffu;
    out[(3 * p + c) >> 2] |= v << (8 * ((3 * p + c) & 3));
  }
}

// The exact 2 x 2 decimation of four output pixels of a 3-channel image: 24 contiguous source bytes in each of two rows
// (six unaligned dword loads per row), (v00 + v01 + v10 + v11 + 2) >> 2, twelve output bytes in out[0..2].
__device__ __forceinline__ void rs_area2_4px_c3(const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, unsigned* out) {
  typedef unsigned u32u __attribute__((aligned(1)));
  unsigned w0[6], w1[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) { w0[k] = reinterpret_cast<const u32u*>(S0)[k]; w1[k] = reinterpret_cast<const u32u*>(S1)[k]; }
  out[0] = out[1] = out[2] = 0u;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int i0 = 6 * p + c, i1 = 6 * p + 3 + c;  // bytes of the two source columns
      const unsigned v = (((w0[i0 >> 2] >> (8 * (i0 & 3))) & 0xffu) + ((w0[i1 >> 2] >> (8 * (i1 & 3))) & 0xffu) +
                          ((w1[i0 >> 2] >> (8 * (i0 & 3))) & 0xffu) + ((w1[i1 >> 2] >> (8 * (i1 & 3))) & 0xffu) + 2u) >> 2;
      out[(3 * p + c) >> 2] |= v << (8 * ((3 * p + c) & 3));
    }
}
#endif

#endif  // ST_INTERNAL_H_
