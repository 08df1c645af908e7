// A convolution's weights in the forms the MFMA kernels of st_conv.hip read, for both networks (pose_net.h, caffe_net.h): the
// host packing of a caffemodel's [cout][cin][k][k] blob and bias into zero-padded [cout_pad][k][k][cin_pad] + [cout_pad], the
// upload, the spatial-tile and bf16-triple forms packed on the device from it, and the owner of the device pointers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <vector>

#include "scannertools_hip.h"

namespace scanner {
namespace net_weights {

// Device copies of one layer's weights; frees what it holds.  Held in place (a std::map's node), never copied.
struct DeviceWeights {
  float* w = nullptr;   // [cout_pad][k][k][cin_pad] for the MFMA kernels; the layout of the layer's kernel otherwise
  float* b = nullptr;
  void* wt = nullptr;   // float32 weights in the spatial-tile kernel's operand order (eligible geometries only)
  void* w3 = nullptr;   // the same weights as bf16 triples (bf16x3 arithmetic only)
  int cin_pad = 0, cout_pad = 0;

  DeviceWeights() = default;
  DeviceWeights(const DeviceWeights&) = delete;
  DeviceWeights& operator=(const DeviceWeights&) = delete;
  ~DeviceWeights() { release(); }
  void release() {
    void** all[] = {(void**)&w, (void**)&b, &wt, &w3};
    for (void** p : all) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
    cin_pad = cout_pad = 0;
  }
};

inline bool to_device(const std::vector<float>& host, float** dev) {
  return hipMalloc(dev, std::max<size_t>(host.size(), 4) * 4) == hipSuccess &&
         (host.empty() || hipMemcpy(*dev, host.data(), host.size() * 4, hipMemcpyHostToDevice) == hipSuccess);
}

// w [cout][cin][k][k] and bias [cout] (null: no bias term) -> d.w, d.b on the current device, output channels padded to a
// multiple of 64 and input channels to cin_pad with zeros.  chan (null: the identity): file channel -> buffer channel.
// False when the device is out of memory; what was allocated stays with d.
inline bool upload_mfma(const float* w, const float* bias, int cout, int cin, int k, int cin_pad, const int* chan, DeviceWeights* d) {
  const int cop = (cout + 63) / 64 * 64, kk = k * k;
  std::vector<float> wp((size_t)cop * kk * cin_pad, 0.f), bp(cop, 0.f);
  for (int o = 0; o < cout; ++o) {
    if (bias) bp[o] = bias[o];
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < kk; ++t) wp[((size_t)o * kk + t) * cin_pad + (chan ? chan[c] : c)] = w[((size_t)o * cin + c) * kk + t];
  }
  d->cin_pad = cin_pad; d->cout_pad = cop;
  return to_device(wp, &d->w) && to_device(bp, &d->b);
}

// d.wt from d.w where the spatial-tile kernel takes this geometry (d.wt stays null where it does not).  ST_ERR_OOM: no device memory.
inline int pack_tile(st_ctx* ctx, int k, DeviceWeights* d) {
  const long long nb = st_conv_f32_tile_bytes(d->cout_pad, k, k, d->cin_pad);
  if (nb <= 0) return ST_OK;
  void* wt = nullptr;
  if (hipMalloc(&wt, (size_t)nb) != hipSuccess) return ST_ERR_OOM;
  const int st = st_conv_pack_weights_f32_tile(ctx, d->w, d->cout_pad, k, k, d->cin_pad, wt);
  if (st != ST_OK) {  // an unpacked buffer must never be mistaken for packed weights by the next call
    (void)hipFree(wt);
    return st;
  }
  d->wt = wt;
  return ST_OK;
}

// d.w3 from d.w.  ST_ERR_OOM: no device memory.
inline int pack_bf16x3(st_ctx* ctx, int k, DeviceWeights* d) {
  void* w3 = nullptr;
  const size_t bytes = (size_t)st_conv_bf16x3_packed_bytes(d->cout_pad, k, k, d->cin_pad);
  if (hipMalloc(&w3, bytes) != hipSuccess) return ST_ERR_OOM;
  const int st = st_conv_pack_weights_bf16x3_n(ctx, d->w, d->cout_pad, k, k, d->cin_pad, w3, bytes);
  if (st != ST_OK) {
    (void)hipFree(w3);
    return st;
  }
  d->w3 = w3;
  return ST_OK;
}

}  // namespace net_weights
}  // namespace scanner
