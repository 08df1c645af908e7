// Context, error reporting, scratch arena and per-kernel event timing for libscannertools_hip.so.
#include <cstring>
#include <vector>
#include <mutex>
#include <chrono>
#include <cstdlib>

#include "st_internal.h"

int st_set_error(st_ctx* ctx, int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->last_error = buf;
  return status;
}

int st_enter(st_ctx* ctx) {
  if (!ctx) return ST_ERR_INVALID;
  ST_HIP(ctx, hipSetDevice(ctx->device));
  return ST_OK;
}

// ---- registry of live contexts (for the concurrency-aware kernel choice) --------------------------------------------------
namespace {
// never destroyed: a context released from a static destructor of the host program must still find the registry
struct CtxRegistry { std::mutex mu; std::vector<st_ctx*> live; };
CtxRegistry& registry() { static CtxRegistry* r = new CtxRegistry; return *r; }
long long now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
void reg_add(st_ctx* c) { CtxRegistry& r = registry(); std::lock_guard<std::mutex> lk(r.mu); r.live.push_back(c); }
void reg_remove(st_ctx* c) {
  CtxRegistry& r = registry();
  std::lock_guard<std::mutex> lk(r.mu);
  for (size_t i = 0; i < r.live.size(); ++i)
    if (r.live[i] == c) { r.live.erase(r.live.begin() + i); break; }
}
}  // namespace

bool st_flow_call_begins(st_ctx* ctx) {
  const long long t = now_ns();
  ctx->flow_enter_ns.store(t, std::memory_order_relaxed);
  ctx->flow_busy.store(true, std::memory_order_release);
  if (ctx->concurrency_mode >= 0) return ctx->concurrency_mode != 0;
  constexpr long long kWindowNs = 50LL * 1000 * 1000;   // a call that began longer ago and was never synchronised is stale
  // TWO other instances in flight: with one, the two calls overlap on the GPU only part of the time (each instance spends a
  // third of its cycle on the host between its synchronisation and its next call) and the lone-instance choice wins
  // (2 instances x 2 pairs per call, a sync per call: 5 440 frames/s against 4 990 with the shared-chip choice)
  int others = 0;
  CtxRegistry& r = registry();
  std::lock_guard<std::mutex> lk(r.mu);
  for (st_ctx* o : r.live)
    if (o != ctx && o->device == ctx->device && o->flow_busy.load(std::memory_order_acquire) &&
        t - o->flow_enter_ns.load(std::memory_order_relaxed) < kWindowNs)
      ++others;
  return others >= 2;
}

ST_EXPORT int st_abi_version(void) { return ST_ABI_VERSION; }

#ifndef ST_SRC_HASH
#define ST_SRC_HASH "unknown"
#endif
#ifndef ST_BUILD_HOST
#define ST_BUILD_HOST "unknown"
#endif
#ifndef ST_BUILD_TIME
#define ST_BUILD_TIME "unknown"
#endif
ST_EXPORT const char* st_build_info(void) { return "src=" ST_SRC_HASH " host=" ST_BUILD_HOST " at=" ST_BUILD_TIME; }

ST_EXPORT const char* st_status_string(int status) {
  switch (status) {
    case ST_OK: return "ok";
    case ST_ERR_INVALID: return "invalid argument";
    case ST_ERR_HIP: return "HIP runtime error";
    case ST_ERR_OOM: return "out of device memory";
    case ST_ERR_UNSUPPORTED: return "unsupported parameters";
    default: return "unknown status";
  }
}

ST_EXPORT int st_device_count(int* count) {
  if (!count) return ST_ERR_INVALID;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return ST_ERR_HIP; }
  *count = n;
  return ST_OK;
}

static constexpr size_t kMinLdsBytes = 160 * 1024;  // gfx950

ST_EXPORT int st_ctx_create(int device_id, st_ctx** out_ctx) {
  if (!out_ctx) return ST_ERR_INVALID;
  *out_ctx = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) return ST_ERR_INVALID;
  if (hipSetDevice(device_id) != hipSuccess) return ST_ERR_HIP;
  st_ctx* c = new (std::nothrow) st_ctx();
  if (!c) return ST_ERR_OOM;
  c->device = device_id;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return ST_ERR_HIP;
  }
  c->stream = c->own_stream;
  if (const char* e = getenv("ST_ITER_TILE")) c->tile_mode = atoi(e);
  c->fold_gray = getenv("ST_PYR_FOLD_GRAY") != nullptr;
  if (const char* e = getenv("ST_POLY_U8")) c->poly_u8 = atoi(e) != 0;
  if (const char* e = getenv("ST_ITER_ROLES")) c->roles_mode = atoi(e);
  if (const char* e = getenv("ST_ROLES_NCW")) c->roles_ncw = atoi(e);
  if (const char* e = getenv("ST_PYR_ROLES")) c->pyr_roles = atoi(e);
  if (const char* e = getenv("ST_PYR_ROLES_RGB")) c->pyr_roles_rgb = atoi(e) != 0;
  if (const char* e = getenv("ST_CONV_TILE")) c->conv_tile = atoi(e);
  if (const char* e = getenv("ST_CONCURRENT")) c->concurrency_mode = atoi(e);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
    c->num_cus = prop.multiProcessorCount;
    // The library is compiled for gfx950 and its kernels are sized for that chip's 160 KB of LDS per workgroup (the Histogram
    // counters take 96 KB, the role-split flow iteration 129 / 158 KB, the convolution tiles up to 104 KB): a device with less
    // is refused here, once, instead of failing at some later launch.
    // ... and the code object holds gfx950 code only: another architecture (even one with as much LDS) has no kernel to run
    if (prop.sharedMemPerBlock < kMinLdsBytes || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      (void)hipStreamDestroy(c->own_stream);
      delete c;
      return ST_ERR_UNSUPPORTED;
    }
  }
  reg_add(c);
  *out_ctx = c;
  return ST_OK;
}

ST_EXPORT int st_ctx_destroy(st_ctx* ctx) {
  if (!ctx) return ST_ERR_INVALID;
  reg_remove(ctx);
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& t : ctx->timing) {
    for (auto e : t.starts) (void)hipEventDestroy(e);
    for (auto e : t.stops) (void)hipEventDestroy(e);
  }
  if (ctx->ws) (void)hipFree(ctx->ws);
  st_jpeg_release(ctx);
  st_png_release(ctx);
  st_jpeg_enc_release(ctx);
  st_png_enc_release(ctx);
  st_netin_release(ctx);
  st_detect_release(ctx);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
  return ST_OK;
}

ST_EXPORT int st_ctx_set_stream(st_ctx* ctx, void* hip_stream) {
  ST_TRY(st_enter(ctx));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->flow_busy.store(false, std::memory_order_release);
  ctx->stream = (hipStream_t)hip_stream;
  return ST_OK;
}

ST_EXPORT int st_ctx_reset_stream(st_ctx* ctx) {
  ST_TRY(st_enter(ctx));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->flow_busy.store(false, std::memory_order_release);
  ctx->stream = ctx->own_stream;
  return ST_OK;
}

ST_EXPORT int st_ctx_sync(st_ctx* ctx) {
  ST_TRY(st_enter(ctx));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->flow_busy.store(false, std::memory_order_release);   // nothing of this context is in flight any more
  return ST_OK;
}

ST_EXPORT int st_ctx_flow_concurrent(st_ctx* ctx) { return ctx && ctx->flow_concurrent ? 1 : 0; }

ST_EXPORT int st_ctx_set_workspace_limit(st_ctx* ctx, size_t bytes) {
  if (!ctx) return ST_ERR_INVALID;
  ctx->ws_limit = bytes ? bytes : ((size_t)64 << 30);
  return ST_OK;
}

ST_EXPORT int st_ctx_release_workspace(st_ctx* ctx) {
  ST_TRY(st_enter(ctx));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->ws) ST_HIP(ctx, hipFree(ctx->ws));
  ctx->ws = nullptr;
  ctx->ws_bytes = 0;
  ctx->ws_off = 0;
  return ST_OK;
}

ST_EXPORT const char* st_ctx_last_error(const st_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int st_ws_reserve(st_ctx* ctx, size_t total_bytes) {
  ctx->ws_off = 0;
  if (total_bytes <= ctx->ws_bytes) return ST_OK;
  if (total_bytes > ctx->ws_limit)
    return st_set_error(ctx, ST_ERR_OOM, "workspace request %zu exceeds limit %zu", total_bytes, ctx->ws_limit);
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->ws) ST_HIP(ctx, hipFree(ctx->ws));
  ctx->ws = nullptr;
  ctx->ws_bytes = 0;
  size_t want = total_bytes + total_bytes / 8;  // slack against regrowth
  if (want > ctx->ws_limit) want = total_bytes;
  hipError_t e = hipMalloc(&ctx->ws, want);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    want = total_bytes;
    e = hipMalloc(&ctx->ws, want);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ctx->ws = nullptr;
    return st_set_error(ctx, ST_ERR_OOM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
  }
  ctx->ws_bytes = want;
  return ST_OK;
}

void st_ws_reset(st_ctx* ctx) { ctx->ws_off = 0; }

void* st_ws_alloc(st_ctx* ctx, size_t bytes) {
  size_t off = st_align_up(ctx->ws_off);
  if (off + bytes > ctx->ws_bytes) return nullptr;
  ctx->ws_off = off + bytes;
  return (char*)ctx->ws + off;
}

ST_EXPORT int st_ctx_timing_enable(st_ctx* ctx, unsigned kernel_mask) {
  if (!ctx) return ST_ERR_INVALID;
  ctx->timing_mask = kernel_mask;
  return ST_OK;
}

static int timing_fold(st_ctx* ctx, st_timing_slot& t) {
  for (size_t i = 0; i < t.used; ++i) {
    float ms = 0.f;
    ST_HIP(ctx, hipEventElapsedTime(&ms, t.starts[i], t.stops[i]));
    t.total_ms += ms;
  }
  t.used = 0;
  return ST_OK;
}

ST_EXPORT int st_ctx_timing_reset(st_ctx* ctx) {
  ST_TRY(st_enter(ctx));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (auto& t : ctx->timing) {
    t.used = 0;
    t.launches = 0;
    t.total_ms = 0.0;
  }
  return ST_OK;
}

ST_EXPORT int st_ctx_timing_read(st_ctx* ctx, int kernel_id, int* launches, double* total_ms) {
  ST_TRY(st_enter(ctx));
  if (kernel_id < 0 || kernel_id >= ST_K_COUNT) return ST_ERR_INVALID;
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  st_timing_slot& t = ctx->timing[kernel_id];
  ST_TRY(timing_fold(ctx, t));
  if (launches) *launches = t.launches;
  if (total_ms) *total_ms = t.total_ms;
  return ST_OK;
}

int st_time_begin(st_ctx* ctx, int id) {
  if (!(ctx->timing_mask & (1u << id))) return ST_OK;
  st_timing_slot& t = ctx->timing[id];
  if (t.used == t.starts.size()) {
    if (t.used >= 4096) {  // fold to bound the pool
      ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
      ST_TRY(timing_fold(ctx, t));
    } else {
      hipEvent_t a, b;
      ST_HIP(ctx, hipEventCreate(&a));
      if (hipEventCreate(&b) != hipSuccess) {
        (void)hipEventDestroy(a);
        return st_set_error(ctx, ST_ERR_HIP, "timing: hipEventCreate failed");
      }
      t.starts.push_back(a);
      t.stops.push_back(b);
    }
  }
  ST_HIP(ctx, hipEventRecord(t.starts[t.used], ctx->stream));
  return ST_OK;
}

// Events for ONE dispatch, to be handed to hipExtLaunchKernelGGL: the runtime then takes both timestamps from the dispatch's
// own completion signal (what a kernel trace reports) instead of from marker packets before and after it, which read 5-6 us
// more than the kernel runs and cost the stream as much.  Null events (timing off) make that launch an ordinary one.
int st_time_dispatch(st_ctx* ctx, int id, hipEvent_t* start, hipEvent_t* stop) {
  *start = *stop = nullptr;
  if (!(ctx->timing_mask & (1u << id))) return ST_OK;
  st_timing_slot& t = ctx->timing[id];
  if (t.used == t.starts.size()) {
    if (t.used >= 4096) {
      ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
      ST_TRY(timing_fold(ctx, t));
    } else {
      hipEvent_t a, b;
      ST_HIP(ctx, hipEventCreate(&a));
      if (hipEventCreate(&b) != hipSuccess) {
        (void)hipEventDestroy(a);
        return st_set_error(ctx, ST_ERR_HIP, "timing: hipEventCreate failed");
      }
      t.starts.push_back(a);
      t.stops.push_back(b);
    }
  }
  *start = t.starts[t.used];
  *stop = t.stops[t.used];
  t.used++;
  t.launches++;
  return ST_OK;
}

int st_time_end(st_ctx* ctx, int id) {
  if (!(ctx->timing_mask & (1u << id))) return ST_OK;
  st_timing_slot& t = ctx->timing[id];
  if (t.used >= t.stops.size()) return st_set_error(ctx, ST_ERR_INVALID, "timing: bracket closed without an open one");
  ST_HIP(ctx, hipEventRecord(t.stops[t.used], ctx->stream));
  t.used++;
  t.launches++;
  return ST_OK;
}
