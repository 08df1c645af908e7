// Layers of a generic Caffe network beyond the stride-1 "same" convolutions of st_conv.hip: InnerProduct on the float32 matrix
// instruction, a direct convolution for every other geometry, Pooling, LRN, Softmax, and the copies between the NHWC activation
// layout and Caffe's planar blobs.  Layer rules: DESIGN.md section 4.14 ([EXT] Caffe's public sources, unpinned).
// Layout: activations are NHWC float32 with a channel stride that is a multiple of 4; a call reads c channels from channel
// x_offset on and writes c channels from y_offset on.  Channels outside those ranges (the zero pad channels of a buffer, the
// other slices of a Concat) are neither read nor written.  Every output element is computed by ONE thread (or one wave, with a
// fixed reduction tree) in an order that depends on the layer alone, so no result depends on the batch size.
#include "st_internal.h"

#include <cfloat>

namespace {

long long grid_for(long long total) {
  long long bx = (total + 255) / 256;
  return bx > 65536 ? 65536 : (bx < 1 ? 1 : bx);
}

// ---- InnerProduct ------------------------------------------------------------------------------------------------------
// y[m][j] = sum_k x[m][k] * W[j][k] (+ bias) for up to 32 rows per launch: a skinny product bound by streaming W.  One wave
// owns 32 output columns and IP_KC values of k; v_mfma_f32_32x32x2_f32 takes the rows as M (rows past n are zero) and 2 k per
// instruction.  The packed weights hold, per column tile and per 8 k, one float4 per lane: lane (j = l & 31, half = l >> 5)
// reads W[tile * 32 + j][8 b + 4 half + 0..3], so a wave's load is one contiguous KiB and W is read exactly once per launch.
// The partial sums of the K chunks go to the workspace and are added in chunk order by k_ip_reduce: chunk size and order are
// fixed by K, never by n.
constexpr int IP_KC = 512;
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct IpArgs {
  const float* x; const float4* wp; float* part;
  int rows, k, xs, nchunks, np;
};

__global__ __launch_bounds__(256) void k_ip_partial(IpArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x, chunk = blockIdx.y * 4 + wave;
  if (chunk >= a.nchunks) return;
  const int m = lane & 31, half = lane >> 5;
  const int k0 = chunk * IP_KC;
  const int nb = ((a.k - k0 < IP_KC ? a.k - k0 : IP_KC)) / 8;
  const float4* wp = a.wp + ((size_t)tile * (a.k / 8) + k0 / 8) * 64 + lane;
  const bool live = m < a.rows;
  const float* xr = a.x + (size_t)(live ? m : 0) * a.xs + k0 + 4 * half;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  int b = 0;
  for (; b + 4 <= nb; b += 4) {   // four KiB of weights in flight per wave before the first of 16 matrix instructions
    float4 wv[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      wv[u] = wp[(size_t)(b + u) * 64];
      xv[u] = *reinterpret_cast<const float4*>(xr + 8 * (b + u));
      if (!live) xv[u] = zero;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u].x, wv[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u].y, wv[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u].z, wv[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u].w, wv[u].w, acc, 0, 0, 0);
    }
  }
  for (; b < nb; ++b) {
    const float4 wv = wp[(size_t)b * 64];
    float4 xv = *reinterpret_cast<const float4*>(xr + 8 * b);
    if (!live) xv = make_float4(0.f, 0.f, 0.f, 0.f);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv.x, wv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv.y, wv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv.z, wv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv.w, wv.w, acc, 0, 0, 0);
  }
  float* p = a.part + (size_t)chunk * 32 * a.np + tile * 32 + m;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
    if (row < a.rows) p[(size_t)row * a.np] = acc[r];
  }
}

struct IpReduceArgs {
  const float* part; const float* bias; float* y;
  int rows, nout, np, nchunks, ys, relu;
};

__global__ __launch_bounds__(256) void k_ip_reduce(IpReduceArgs a) {
  const long long total = (long long)a.rows * a.nout;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int j = (int)(i % a.nout), m = (int)(i / a.nout);
    const float* p = a.part + (size_t)m * a.np + j;
    float s = p[0];
    for (int c = 1; c < a.nchunks; ++c) s += p[(size_t)c * 32 * a.np];
    if (a.bias) s += a.bias[j];
    if (a.relu && !(s > 0.f)) s = 0.f;
    a.y[(size_t)m * a.ys + j] = s;
  }
}

__global__ __launch_bounds__(256) void k_ip_pack(const float* __restrict__ w, int k, int nout, long long total, float* __restrict__ out) {
  const int kb8 = k / 8;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
    const long long rest = i >> 8;
    const int b = (int)(rest % kb8);
    const long long tile = rest / kb8;
    const long long col = tile * 32 + (lane & 31);
    out[i] = col < nout ? w[col * k + 8 * b + 4 * (lane >> 5) + j] : 0.f;
  }
}

// ---- direct convolution ------------------------------------------------------------------------------------------------
// One thread per output element; the sum runs over (ky, kx, input channel of the group) in that order as one fmaf chain.
// w: [cout][kh][kw][cin / group].
struct GConvArgs {
  const float* x; const float* w; const float* bias; float* y;
  int n, h, wd, cin, xs, xoff, k, stride, pad, group, cout, oh, ow, ys, yoff, relu;
};

__global__ __launch_bounds__(256) void k_conv_general(GConvArgs a) {
  const long long total = (long long)a.n * a.oh * a.ow * a.cout;
  const int cg = a.cin / a.group, og = a.cout / a.group;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int o = (int)(i % a.cout);
    long long px = i / a.cout;
    const int ox = (int)(px % a.ow);
    px /= a.ow;
    const int oy = (int)(px % a.oh), f = (int)(px / a.oh);
    const int c0 = (o / og) * cg;
    const float* wr = a.w + (size_t)o * a.k * a.k * cg;
    float s = 0.f;
    for (int ky = 0; ky < a.k; ++ky) {
      const int iy = oy * a.stride - a.pad + ky;
      if (iy < 0 || iy >= a.h) continue;
      for (int kx = 0; kx < a.k; ++kx) {
        const int ix = ox * a.stride - a.pad + kx;
        if (ix < 0 || ix >= a.wd) continue;
        const float* xp = a.x + ((size_t)((size_t)f * a.h + iy) * a.wd + ix) * a.xs + a.xoff + c0;
        const float* wp = wr + (size_t)(ky * a.k + kx) * cg;
        for (int c = 0; c < cg; ++c) s = fmaf(xp[c], wp[c], s);
      }
    }
    if (a.bias) s += a.bias[o];
    if (a.relu && !(s > 0.f)) s = 0.f;
    a.y[((size_t)((size_t)f * a.oh + oy) * a.ow + ox) * a.ys + a.yoff + o] = s;
  }
}

// ---- Pooling -----------------------------------------------------------------------------------------------------------
// Caffe's windows: [o * s - p, min(o * s - p + k, H + p)) clipped to the map; MAX over the clipped window, AVE the clipped
// window's sum divided by the UNCLIPPED window's size.
struct PoolNNArgs {
  const float* x; float* y;
  int n, h, wd, c, xs, xoff, k, stride, pad, oh, ow, ys, yoff, ave;
};

__global__ __launch_bounds__(256) void k_pool(PoolNNArgs a) {
  const long long total = (long long)a.n * a.oh * a.ow * a.c;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % a.c);
    long long px = i / a.c;
    const int ox = (int)(px % a.ow);
    px /= a.ow;
    const int oy = (int)(px % a.oh), f = (int)(px / a.oh);
    int y0 = oy * a.stride - a.pad, x0 = ox * a.stride - a.pad;
    int y1 = y0 + a.k < a.h + a.pad ? y0 + a.k : a.h + a.pad, x1 = x0 + a.k < a.wd + a.pad ? x0 + a.k : a.wd + a.pad;
    const int size = (y1 - y0) * (x1 - x0);
    y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0;
    y1 = y1 > a.h ? a.h : y1; x1 = x1 > a.wd ? a.wd : x1;
    float r = a.ave ? 0.f : -FLT_MAX;
    for (int yy = y0; yy < y1; ++yy)
      for (int xx = x0; xx < x1; ++xx) {
        const float v = a.x[((size_t)((size_t)f * a.h + yy) * a.wd + xx) * a.xs + a.xoff + c];
        if (a.ave) r += v;
        else r = v > r ? v : r;
      }
    if (a.ave) r = r / (float)size;
    a.y[((size_t)((size_t)f * a.oh + oy) * a.ow + ox) * a.ys + a.yoff + c] = r;
  }
}

// ---- LRN across channels -----------------------------------------------------------------------------------------------
struct LrnArgs {
  const float* x; float* y;
  long long pixels;
  int c, xs, xoff, ys, yoff, size;
  float alpha, beta, k;
};

__global__ __launch_bounds__(256) void k_lrn(LrnArgs a) {
  const long long total = a.pixels * a.c;
  const int half = (a.size - 1) / 2;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % a.c);
    const long long px = i / a.c;
    const float* xp = a.x + (size_t)px * a.xs + a.xoff;
    const int lo = c - half < 0 ? 0 : c - half, hi = c + half > a.c - 1 ? a.c - 1 : c + half;
    float s = 0.f;
    for (int j = lo; j <= hi; ++j) s = fmaf(xp[j], xp[j], s);
    const float scale = a.k + (a.alpha / (float)a.size) * s;
    a.y[(size_t)px * a.ys + a.yoff + c] = xp[c] * powf(scale, -a.beta);
  }
}

// ---- Softmax over channels: one wave per pixel, a fixed butterfly for the maximum and the sum ---------------------------
struct SoftmaxArgs {
  const float* x; float* y;
  long long pixels;
  int c, xs, xoff, ys, yoff;
};

__global__ __launch_bounds__(256) void k_softmax(SoftmaxArgs a) {
  const int lane = threadIdx.x & 63;
  for (long long px = blockIdx.x * 4LL + (threadIdx.x >> 6); px < a.pixels; px += (long long)gridDim.x * 4) {
    const float* xp = a.x + (size_t)px * a.xs + a.xoff;
    float* yp = a.y + (size_t)px * a.ys + a.yoff;
    float m = -FLT_MAX;
    for (int c = lane; c < a.c; c += 64) m = xp[c] > m ? xp[c] : m;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const float o = __shfl_xor(m, d, 64);
      m = o > m ? o : m;
    }
    float s = 0.f;
    for (int c = lane; c < a.c; c += 64) s += expf(xp[c] - m);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    for (int c = lane; c < a.c; c += 64) yp[c] = expf(xp[c] - m) / s;
  }
}

// ---- layout copies -----------------------------------------------------------------------------------------------------
struct CopyArgs {
  const float* x; float* y;
  long long pixels;
  int c, xs, xoff, ys, yoff, relu;
};

__global__ __launch_bounds__(256) void k_copy_channels(CopyArgs a) {
  const long long total = a.pixels * a.c;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % a.c);
    const long long px = i / a.c;
    float v = a.x[(size_t)px * a.xs + a.xoff + c];
    if (a.relu && !(v > 0.f)) v = 0.f;
    a.y[(size_t)px * a.ys + a.yoff + c] = v;
  }
}

struct PlanarOutArgs {
  const float* x; float* const* out;
  long long hw;
  int n, c, xs, xoff;
};

__global__ __launch_bounds__(256) void k_nhwc_to_planar(PlanarOutArgs a) {
  const long long per = a.hw * a.c, total = per * a.n;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int f = (int)(i / per);
    const long long r = i - (long long)f * per;
    const int c = (int)(r / a.hw);
    const long long p = r - (long long)c * a.hw;
    st_gl(a.out[f])[r] = a.x[((size_t)f * a.hw + p) * a.xs + a.xoff + c];
  }
}

bool slice_ok(int c, int stride, int offset) { return c > 0 && offset >= 0 && stride > 0 && offset + c <= stride; }

}  // namespace

ST_EXPORT long long st_inner_product_packed_bytes(int k, int nout) {
  if (k <= 0 || k % 8 || nout <= 0) return 0;
  return (long long)((nout + 31) / 32) * 32 * k * 4;
}

ST_EXPORT int st_inner_product_pack_weights(st_ctx* ctx, const float* w_dev, int k, int nout, void* out_dev) {
  ST_TRY(st_enter(ctx));
  if (!w_dev || !out_dev || k <= 0 || k % 8 || nout <= 0 || ((uintptr_t)out_dev & 15))
    return st_set_error(ctx, ST_ERR_INVALID, "inner_product pack: bad arguments (k a multiple of 8, 16-byte aligned output)");
  const long long total = (long long)((nout + 31) / 32) * 32 * k;
  hipLaunchKernelGGL(k_ip_pack, dim3((unsigned)grid_for(total)), dim3(256), 0, ctx->stream, w_dev, k, nout, total, (float*)out_dev);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}

ST_EXPORT int st_inner_product_f32(st_ctx* ctx, const float* x_dev, int n, int k, int x_stride, const void* wp_dev, const float* bias_dev,
                                   int nout, int relu, float* y_dev, int y_stride) {
  ST_TRY(st_enter(ctx));
  if (!x_dev || !wp_dev || !y_dev || n <= 0 || k <= 0 || k % 8 || nout <= 0 || x_stride < k || x_stride % 4 || y_stride < nout ||
      ((uintptr_t)x_dev & 15) || ((uintptr_t)wp_dev & 15))
    return st_set_error(ctx, ST_ERR_INVALID, "inner_product: bad arguments (k a multiple of 8 <= x_stride, x_stride a multiple of 4, nout <= y_stride, 16-byte aligned x and weights)");
  const int ntiles = (nout + 31) / 32, np = ntiles * 32, nchunks = (k + IP_KC - 1) / IP_KC;
  if ((nchunks + 3) / 4 > 65535) return st_set_error(ctx, ST_ERR_UNSUPPORTED, "inner_product: k too large");
  ST_TRY(st_ws_reserve(ctx, (size_t)nchunks * 32 * np * 4));
  float* part = (float*)st_ws_alloc(ctx, (size_t)nchunks * 32 * np * 4);
  if (!part) return st_set_error(ctx, ST_ERR_OOM, "inner_product: workspace exhausted");
  for (int r0 = 0; r0 < n; r0 += 32) {
    const int rows = n - r0 < 32 ? n - r0 : 32;
    IpArgs a;
    a.x = x_dev + (size_t)r0 * x_stride; a.wp = (const float4*)wp_dev; a.part = part;
    a.rows = rows; a.k = k; a.xs = x_stride; a.nchunks = nchunks; a.np = np;
    IpReduceArgs r;
    r.part = part; r.bias = bias_dev; r.y = y_dev + (size_t)r0 * y_stride;
    r.rows = rows; r.nout = nout; r.np = np; r.nchunks = nchunks; r.ys = y_stride; r.relu = relu ? 1 : 0;
    st_timed t(ctx, ST_K_CONV);
    hipLaunchKernelGGL(k_ip_partial, dim3(ntiles, (nchunks + 3) / 4), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_ip_reduce, dim3((unsigned)grid_for((long long)rows * nout)), dim3(256), 0, ctx->stream, r);
    ST_HIP(ctx, hipGetLastError());
  }
  return ST_OK;
}

ST_EXPORT int st_conv_out_size(int size, int k, int stride, int pad) {
  if (size <= 0 || k <= 0 || stride <= 0 || pad < 0 || size + 2 * pad < k) return 0;
  return (size + 2 * pad - k) / stride + 1;
}

ST_EXPORT int st_pool_out_size(int size, int k, int stride, int pad) {
  if (size <= 0 || k <= 0 || stride <= 0 || pad < 0 || pad >= k || size + 2 * pad < k) return 0;
  int out = (size + 2 * pad - k + stride - 1) / stride + 1;
  if (pad > 0 && (out - 1) * stride >= size + pad) --out;
  return out;
}

ST_EXPORT int st_conv2d_general_nhwc_f32(st_ctx* ctx, const float* x_dev, int n, int h, int w, int cin, int x_stride, int x_offset,
                                         const float* w_dev, const float* bias_dev, int k, int stride, int pad, int group, int cout,
                                         int relu, float* y_dev, int y_stride, int y_offset) {
  ST_TRY(st_enter(ctx));
  const int oh = st_conv_out_size(h, k, stride, pad), ow = st_conv_out_size(w, k, stride, pad);
  if (!x_dev || !w_dev || !y_dev || n <= 0 || group <= 0 || !slice_ok(cin, x_stride, x_offset) || !slice_ok(cout, y_stride, y_offset) ||
      cin % group || cout % group || oh <= 0 || ow <= 0)
    return st_set_error(ctx, ST_ERR_INVALID, "conv2d_general: bad arguments (%dx%d map, kernel %d stride %d pad %d group %d, %d -> %d channels)", h, w, k,
                        stride, pad, group, cin, cout);
  GConvArgs a;
  a.x = x_dev; a.w = w_dev; a.bias = bias_dev; a.y = y_dev;
  a.n = n; a.h = h; a.wd = w; a.cin = cin; a.xs = x_stride; a.xoff = x_offset; a.k = k; a.stride = stride; a.pad = pad; a.group = group;
  a.cout = cout; a.oh = oh; a.ow = ow; a.ys = y_stride; a.yoff = y_offset; a.relu = relu ? 1 : 0;
  st_timed t(ctx, ST_K_CONV);
  hipLaunchKernelGGL(k_conv_general, dim3((unsigned)grid_for((long long)n * oh * ow * cout)), dim3(256), 0, ctx->stream, a);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}

ST_EXPORT int st_pool_nhwc_f32(st_ctx* ctx, const float* x_dev, int n, int h, int w, int c, int x_stride, int x_offset, int method, int k,
                               int stride, int pad, int global, float* y_dev, int y_stride, int y_offset) {
  ST_TRY(st_enter(ctx));
  int oh = 1, ow = 1;
  if (global) {
    // Caffe's global pooling: the kernel is the map, stride 1, no padding.  The one window is [0, max side) on both axes,
    // clipped to the map BEFORE its size is taken (pad 0), so the AVE divisor is h * w whatever the map's shape.
    pad = 0; stride = 1; k = h > w ? h : w;
  } else {
    oh = st_pool_out_size(h, k, stride, pad); ow = st_pool_out_size(w, k, stride, pad);
  }
  if (!x_dev || !y_dev || n <= 0 || h <= 0 || w <= 0 || !slice_ok(c, x_stride, x_offset) || !slice_ok(c, y_stride, y_offset) ||
      (method != ST_POOL_MAX && method != ST_POOL_AVE) || oh <= 0 || ow <= 0)
    return st_set_error(ctx, ST_ERR_INVALID, "pool: bad arguments (%dx%d map, kernel %d stride %d pad %d)", h, w, k, stride, pad);
  PoolNNArgs a;
  a.x = x_dev; a.y = y_dev; a.n = n; a.h = h; a.wd = w; a.c = c; a.xs = x_stride; a.xoff = x_offset;
  a.k = k; a.stride = stride; a.pad = pad; a.oh = oh; a.ow = ow; a.ys = y_stride; a.yoff = y_offset;
  a.ave = method == ST_POOL_AVE;
  st_timed t(ctx, ST_K_CONV);
  hipLaunchKernelGGL(k_pool, dim3((unsigned)grid_for((long long)n * oh * ow * c)), dim3(256), 0, ctx->stream, a);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}

ST_EXPORT int st_lrn_nhwc_f32(st_ctx* ctx, const float* x_dev, long long pixels, int c, int x_stride, int x_offset, int local_size,
                              float alpha, float beta, float k, float* y_dev, int y_stride, int y_offset) {
  ST_TRY(st_enter(ctx));
  if (!x_dev || !y_dev || pixels <= 0 || !slice_ok(c, x_stride, x_offset) || !slice_ok(c, y_stride, y_offset) || local_size <= 0 ||
      !(local_size & 1))
    return st_set_error(ctx, ST_ERR_INVALID, "lrn: bad arguments (an odd local_size)");
  LrnArgs a;
  a.x = x_dev; a.y = y_dev; a.pixels = pixels; a.c = c; a.xs = x_stride; a.xoff = x_offset; a.ys = y_stride; a.yoff = y_offset;
  a.size = local_size; a.alpha = alpha; a.beta = beta; a.k = k;
  st_timed t(ctx, ST_K_CONV);
  hipLaunchKernelGGL(k_lrn, dim3((unsigned)grid_for(pixels * c)), dim3(256), 0, ctx->stream, a);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}

ST_EXPORT int st_softmax_nhwc_f32(st_ctx* ctx, const float* x_dev, long long pixels, int c, int x_stride, int x_offset, float* y_dev,
                                  int y_stride, int y_offset) {
  ST_TRY(st_enter(ctx));
  if (!x_dev || !y_dev || pixels <= 0 || !slice_ok(c, x_stride, x_offset) || !slice_ok(c, y_stride, y_offset))
    return st_set_error(ctx, ST_ERR_INVALID, "softmax: bad arguments");
  SoftmaxArgs a;
  a.x = x_dev; a.y = y_dev; a.pixels = pixels; a.c = c; a.xs = x_stride; a.xoff = x_offset; a.ys = y_stride; a.yoff = y_offset;
  long long bx = (pixels + 3) / 4;
  if (bx > 65536) bx = 65536;
  st_timed t(ctx, ST_K_CONV);
  hipLaunchKernelGGL(k_softmax, dim3((unsigned)bx), dim3(256), 0, ctx->stream, a);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}

ST_EXPORT int st_copy_channels_nhwc_f32(st_ctx* ctx, const float* x_dev, long long pixels, int c, int x_stride, int x_offset, int relu,
                                        float* y_dev, int y_stride, int y_offset) {
  ST_TRY(st_enter(ctx));
  if (!x_dev || !y_dev || pixels <= 0 || !slice_ok(c, x_stride, x_offset) || !slice_ok(c, y_stride, y_offset))
    return st_set_error(ctx, ST_ERR_INVALID, "copy_channels: bad arguments");
  CopyArgs a;
  a.x = x_dev; a.y = y_dev; a.pixels = pixels; a.c = c; a.xs = x_stride; a.xoff = x_offset; a.ys = y_stride; a.yoff = y_offset; a.relu = relu ? 1 : 0;
  st_timed t(ctx, ST_K_CONV);
  hipLaunchKernelGGL(k_copy_channels, dim3((unsigned)grid_for(pixels * c)), dim3(256), 0, ctx->stream, a);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}

ST_EXPORT int st_nhwc_to_planar_f32(st_ctx* ctx, const float* x_dev, int n, int h, int w, int c, int x_stride, int x_offset,
                                    float* const* out_dev) {
  ST_TRY(st_enter(ctx));
  if (!x_dev || !out_dev || n <= 0 || h <= 0 || w <= 0 || !slice_ok(c, x_stride, x_offset))
    return st_set_error(ctx, ST_ERR_INVALID, "nhwc_to_planar: bad arguments");
  ST_TRY(st_check_rows(ctx, "nhwc_to_planar: row %d is null", n, false, out_dev));
  float** d_out;
  ST_TRY(st_upload_tables(ctx, n, 0, out_dev, &d_out));
  PlanarOutArgs a;
  a.x = x_dev; a.out = d_out; a.hw = (long long)h * w; a.n = n; a.c = c; a.xs = x_stride; a.xoff = x_offset;
  st_timed t(ctx, ST_K_CONV);
  hipLaunchKernelGGL(k_nhwc_to_planar, dim3((unsigned)grid_for(a.hw * c * n)), dim3(256), 0, ctx->stream, a);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}
