// What every Scanner kernel class of this directory shares: the choice of the GPU, the C-ABI context and the result that
// validate() reports (KernelCore), the check on C-ABI status codes (ST_CHECK), and the tables an execute() builds from
// its columns.  stage.h holds the host <-> device copies.  Skeleton of a kernel class, registered twice
// (STAGED: DeviceType::CPU, host frames staged through the GPU; otherwise DeviceType::GPU, device-resident frames):
//
//   template <bool STAGED> class FooKernelHIPImpl : public BatchedKernel, public VideoKernel {
//    public:
//     FooKernelHIPImpl(const KernelConfig& config) : BatchedKernel(config), core_(config, STAGED), stage_(core_.gpu) {
//       if (!parse_foo_args(config.args, &args_)) RESULT_ERROR(&core_.valid, "Could not parse FooArgs");
//       else core_.open("FooKernelHIP");  // last: the DeviceType::GPU check of the non-staged class, then the context
//     }
//     void validate(Result* result) override { core_.validate(result); }
//     void execute(const BatchedElements& in, BatchedElements& out) override {
//       ... check_frame(core_.device, in[0][0]); check_batch_shape(in[0], frame_info_, "Foo");
//       ... STAGED: stage_.reserve / upload_frames / strided_ptrs, else input_ptrs / output_ptrs
//       ST_CHECK(core_.ctx, st_foo_batch(core_.ctx, ...)); core_.sync(); ... STAGED: stage_.download_frames
//     }
//    private:
//     KernelCore core_;   // after an UploadPipeline it is bound to (the context goes first), before what needs core_.gpu
//     DeviceStage stage_;
//   };
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "scanner/api/kernel.h"
#include "scanner/util/hip.h"
#include "scannertools_hip.h"
#include "stage.h"

namespace scanner {

// `call`, a C-ABI call on `ctx`, must return ST_OK: otherwise fatal with the entry point's name and the context's last error
#define ST_CHECK(ctx, call) ::scanner::st_check((ctx), (call), #call)
inline void st_check(st_ctx* ctx, int st, const char* call) {
  if (st != ST_OK) LOG(FATAL) << std::string(call, strcspn(call, "(")) << ": " << st_ctx_last_error(ctx);
}
inline void st_sync(st_ctx* ctx) { ST_CHECK(ctx, st_ctx_sync(ctx)); }

class KernelCore {
 public:
  // staged: the class is registered on DeviceType::CPU and works on the GPU that backs such kernels
  KernelCore(const KernelConfig& config, bool staged)
    : device(config.devices[0]), gpu(staged ? staging_device_id() : config.devices[0].id), staged_(staged) {}
  ~KernelCore() { close(&ctx); }
  KernelCore(const KernelCore&) = delete;
  KernelCore& operator=(const KernelCore&) = delete;

  // The end of a constructor whose own checks have passed: a non-staged class runs on DeviceType::GPU only; then the context.
  bool open(const char* class_name) {
    if (!staged_ && device.type != DeviceType::GPU) {
      RESULT_ERROR(&valid, "%s runs on DeviceType::GPU only", class_name);
      return false;
    }
    return open(&ctx);
  }
  // one more context on the same GPU, for a class that keeps several; close() is its counterpart
  bool open(st_ctx** c) {
    const int st = st_ctx_create(gpu, c);
    if (st != ST_OK) RESULT_ERROR(&valid, "st_ctx_create(%d) failed: %s (no CPU fallback exists)", gpu, st_status_string(st));
    return st == ST_OK;
  }
  void close(st_ctx** c) {
    if (*c) st_ctx_destroy(*c);
    *c = nullptr;
  }
  // the context's work goes to the pipeline's compute stream
  bool bind(UploadPipeline* pipe) {
    const bool ok = pipe->init(gpu) && st_ctx_set_stream(ctx, pipe->compute_stream()) == ST_OK;
    if (!ok) RESULT_ERROR(&valid, "cannot create the upload pipeline on device %d", gpu);
    return ok;
  }
  void sync() { st_sync(ctx); }
  void validate(Result* result) const {
    result->set_msg(valid.msg());
    result->set_success(valid.success());
  }

  const DeviceHandle device;  // where Scanner keeps this kernel's frames
  const int gpu;              // where it computes
  Result valid;
  st_ctx* ctx = nullptr;

 private:
  const bool staged_;
};

// every frame of the column has the shape `info`
inline void check_batch_shape(const Elements& col, const FrameInfo& info, const char* op) {
  for (size_t i = 0; i < col.size(); ++i)
    LOG_IF(FATAL, col[i].as_const_frame()->as_frame_info() != info) << op << ": frame " << i << " changes shape inside a batch";
}

// pointer tables of an execute(): n blocks `stride` apart, the frames of an input column, newly allocated output frames
template <typename T>
void strided_ptrs(std::vector<T*>& v, i32 n, u8* base, size_t stride) {
  v.resize(n);
  for (i32 i = 0; i < n; ++i) v[i] = (T*)(base + stride * i);
}
template <typename T>
void input_ptrs(std::vector<const T*>& v, const Elements& col) {
  v.resize(col.size());
  for (size_t i = 0; i < col.size(); ++i) v[i] = (const T*)col[i].as_const_frame()->data;
}
template <typename T>
void output_ptrs(std::vector<T*>& v, const std::vector<Frame*>& frames) {
  v.resize(frames.size());
  for (size_t i = 0; i < frames.size(); ++i) v[i] = (T*)frames[i]->data;
}

// Copies n blocks of `bytes` between host[i] and dev[i]; a run of blocks adjacent on both sides is one hipMemcpyAsync
// (a PCIe copy of one 6 MB frame carries ~0.2 ms of fixed cost, a third of its duration).
template <typename H, typename D>
void copy_runs(hipMemcpyKind kind, H* const* host, D* const* dev, size_t n, size_t bytes, hipStream_t stream) {
  for (size_t i = 0; i < n;) {
    size_t j = i + 1;
    while (j < n && (const u8*)host[j] == (const u8*)host[j - 1] + bytes && (const u8*)dev[j] == (const u8*)dev[j - 1] + bytes) ++j;
    if (kind == hipMemcpyHostToDevice) HIP_CHECK(hipMemcpyAsync((void*)dev[i], host[i], bytes * (j - i), kind, stream));
    else HIP_CHECK(hipMemcpyAsync((void*)host[i], dev[i], bytes * (j - i), kind, stream));
    i = j;
  }
}

// Rows [r0, r0 + nb) of a column of 2-element stencils: the distinct frames (by buffer address) in order of first use,
// and per row the (from, to) indices into them -- a frame shared between windows is listed, and later processed, once.
inline void pair_table(const std::vector<Elements>& col, i32 r0, i32 nb, std::vector<const u8*>* frames, std::vector<int32_t>* pairs) {
  frames->clear();
  pairs->clear();
  std::unordered_map<const u8*, i32> slot;
  for (i32 i = r0; i < r0 + nb; ++i)
    for (i32 s = 0; s < 2; ++s) {
      const u8* d = col[i][s].as_const_frame()->data;
      auto it = slot.find(d);
      if (it == slot.end()) {
        it = slot.emplace(d, (i32)frames->size()).first;
        frames->push_back(d);
      }
      pairs->push_back(it->second);
    }
}

// integer from the environment, at least `min`; *was_set: whether the variable exists
inline int env_int(const char* name, int dflt, int min, bool* was_set = nullptr) {
  const char* e = getenv(name);
  if (was_set) *was_set = e != nullptr;
  return std::max(min, e ? atoi(e) : dflt);
}

}  // namespace scanner
