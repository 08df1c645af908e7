// Caffe op for Scanner on MI355X: frames -> CaffeInput -> Caffe -> features or class scores.
//
// Drop-in for the reference's op (/root/reference/scannertools_caffe/scannertools_caffe_cpp/caffe_kernel_cpu.cpp:5-8,
// caffe_kernel_gpu.cpp): frame_input("caffe_frame") -> frame_output("caffe_output"), protobuf_name("CaffeArgs"), registered on
// DeviceType::GPU and, staged through the GPU, on DeviceType::CPU, both batched.  The kernel class is caffe_kernel_hip.h, the
// forward pass caffe_net.h.
#include "caffe_kernel_hip.h"

// The planner without a GPU: the number of launches-carrying layers executed for an input of (c, h, w) -- 0 for c, h or w takes
// the description's own -- from the description's first input blob to `output_blob`, with the output blob's (C, H, W) in
// out_shape; -1 with the reason in `err`.  With `caffemodel` the weights of every Convolution / InnerProduct on the path must be
// in the file with the right element counts.
extern "C" __attribute__((visibility("default"))) int scannertools_caffe_plan_net(const char* prototxt, const char* caffemodel, int c, int h, int w,
                                                                                  const char* output_blob, int* out_shape, char* err, size_t err_len) {
  std::string msg;
  int steps = -1;
  try {
    namespace cn = scanner::caffe_net;
    scanner::caffe_files::Blobs weights;
    std::vector<cn::Layer> layers;
    cn::Plan plan;
    if (!prototxt || !output_blob) {
      msg = "null argument";
    } else if ((!caffemodel || scanner::caffe_files::read_caffemodel(caffemodel, &weights, &msg)) && cn::parse_layers(prototxt, &layers, &msg)) {
      std::string input;
      for (auto& l : layers)
        if (input.empty() && l.kind == cn::kInput && l.num_output != -1 && !l.tops.empty()) input = l.tops[0];
      if (input.empty()) msg = "malformed description: no input blob";
      else if (cn::make_plan(prototxt, caffemodel ? &weights : nullptr, c, h, w, input, output_blob, true, &plan, &msg)) {
        steps = (int)plan.steps.size();
        if (out_shape) { out_shape[0] = plan.out_shape.c; out_shape[1] = plan.out_shape.h; out_shape[2] = plan.out_shape.w; }
      }
    }
  } catch (const std::exception& e) {
    msg = e.what();
    steps = -1;
  }
  if (err && err_len) { strncpy(err, msg.c_str(), err_len - 1); err[err_len - 1] = 0; }
  return steps;
}

// Measurement (scripts/bench_caffe_net.py): the forward pass of `n` random frames of the description's own input size on `device`,
// `reps` times after one warm-up, timed by the library's ST_K_CONV events.  total_ms[reps]: the kernel time of each whole pass
// (input and output layout copies included); step_ms[steps]: per launch-carrying layer the median over the passes, from passes that
// synchronise after every layer; step_names: the layers' names, newline-separated.  Returns the number of steps, -1 with `err`.
extern "C" __attribute__((visibility("default"))) int scannertools_caffe_time_net(const char* prototxt, const char* caffemodel, const char* output_blob,
                                                                                  int device, int n, int reps, double* total_ms, double* step_ms,
                                                                                  int max_steps, char* step_names, size_t names_len, char* err,
                                                                                  size_t err_len) {
  namespace cn = scanner::caffe_net;
  std::string msg;
  int steps = -1;
  st_ctx* ctx = nullptr;
  float* in = nullptr;
  float* out = nullptr;
  try {
    std::vector<cn::Layer> layers;
    std::string input;
    cn::Net net;
    if (!prototxt || !caffemodel || !output_blob || n <= 0 || reps <= 0 || !total_ms) msg = "bad arguments";
    else if (hipSetDevice(device) != hipSuccess || st_ctx_create(device, &ctx) != ST_OK) msg = "cannot open device " + std::to_string(device);
    else if (cn::parse_layers(prototxt, &layers, &msg)) {
      for (auto& l : layers)
        if (input.empty() && l.kind == cn::kInput && l.num_output != -1 && !l.tops.empty()) input = l.tops[0];
      if (net.load(prototxt, caffemodel, input, output_blob, &msg) && net.prepare(ctx, 0, 0, 0, &msg)) {
        const cn::Shape is = net.plan().in_shape, os = net.plan().out_shape;
        const size_t in_f = (size_t)is.c * is.h * is.w, out_f = (size_t)os.c * os.h * os.w;
        std::vector<float> host(in_f * n);
        unsigned state = 12345u;
        for (auto& v : host) { state = state * 1664525u + 1013904223u; v = (float)(state >> 8) / 16777216.f * 200.f - 100.f; }
        if (hipMalloc(&in, host.size() * 4) != hipSuccess || hipMalloc(&out, out_f * n * 4) != hipSuccess ||
            hipMemcpy(in, host.data(), host.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
          msg = "out of device memory";
        } else {
          std::vector<const float*> src(n);
          std::vector<float*> dst(n);
          for (int i = 0; i < n; ++i) { src[i] = in + in_f * i; dst[i] = out + out_f * i; }
          bool ok = net.forward(ctx, src.data(), n, dst.data(), &msg) && st_ctx_sync(ctx) == ST_OK;
          ok = ok && st_ctx_timing_enable(ctx, 1u << ST_K_CONV) == ST_OK;
          for (int r = 0; r < reps && ok; ++r) {
            int launches = 0;
            ok = st_ctx_timing_reset(ctx) == ST_OK && net.forward(ctx, src.data(), n, dst.data(), &msg) &&
                 st_ctx_timing_read(ctx, ST_K_CONV, &launches, &total_ms[r]) == ST_OK;
          }
          const size_t ns = net.plan().steps.size();
          std::vector<std::vector<double>> per(ns);
          for (int r = 0; r < reps && ok && step_ms; ++r) {
            std::vector<double> one;
            ok = net.forward(ctx, src.data(), n, dst.data(), &msg, &one) && one.size() == ns;
            for (size_t i = 0; i < ns && ok; ++i) per[i].push_back(one[i]);
          }
          if (ok) {
            steps = (int)ns;
            std::string names;
            for (size_t i = 0; i < ns; ++i) {
              if (step_ms && (int)i < max_steps) {
                std::sort(per[i].begin(), per[i].end());
                step_ms[i] = per[i][per[i].size() / 2];
              }
              names += net.plan().layers[net.plan().steps[i].layer].name + "\n";
            }
            if (step_names && names_len) { strncpy(step_names, names.c_str(), names_len - 1); step_names[names_len - 1] = 0; }
          } else if (msg.empty()) {
            msg = st_ctx_last_error(ctx);
          }
        }
      }
      net.release();   // on its device, before the context goes
    }
  } catch (const std::exception& e) {
    msg = e.what();
    steps = -1;
  }
  if (in) (void)hipFree(in);
  if (out) (void)hipFree(out);
  if (ctx) st_ctx_destroy(ctx);
  if (err && err_len) { strncpy(err, msg.c_str(), err_len - 1); err[err_len - 1] = 0; }
  return steps;
}

namespace scanner {
using CaffeKernelHIP = CaffeKernelHIPImpl<false, false>;
using CaffeKernelHIPStaged = CaffeKernelHIPImpl<true, false>;

REGISTER_OP(Caffe).frame_input("caffe_frame").frame_output("caffe_output").protobuf_name("CaffeArgs");

REGISTER_KERNEL(Caffe, CaffeKernelHIPStaged).device(DeviceType::CPU).num_devices(1).batch();
REGISTER_KERNEL(Caffe, CaffeKernelHIP).device(DeviceType::GPU).num_devices(1).batch();
}
