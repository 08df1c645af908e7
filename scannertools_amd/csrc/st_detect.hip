// FacenetOutput of scannertools_caffe for gfx950: the Facenet detector's maps become NMS-filtered face boxes.
//
//   FacenetOutput  scannertools_caffe/scannertools_caffe_cpp/facenet_output_kernel_cpu.cpp:72-163
//                  per frame a triple loop over (valid template, xi, yi) that pushes boxes into a vector, then Scanner's
//                  best_nms(boxes, 0.1) on the host.  Here, for a whole batch:
//     k_fo_decode  one thread per (frame, valid template, cell): sigmoid and threshold on the confidence plane; a
//                  survivor reads its four adjustments, forms the box, and appends the key (score bits, candidate
//                  index) through the frame's counter.  Append order is arbitrary: the sort below is total.
//     k_nms        one workgroup per frame: bitonic sort of the keys (score descending, index ascending), the boxes in
//                  sorted order, then the greedy loop -- find the first box that is still valid, keep it, all threads apply
//                  its suppression.  Keys and boxes live in LDS up to NMS_LDS_CAP boxes and in global scratch beyond; it is
//                  the same code on two pointers, and no survivor is ever dropped for space.
//     k_fo_pack    the kept candidates' rows [x1, y1, x2, y2, score], all frames packed, for one copy to the host.
//   st_bbox_nms_f32 is k_nms alone on rows the caller supplies.
//
// Arithmetic (include/scannertools_hip.h): float32, every operation rounded on its own (the file is
// compiled with -ffp-contract=off).  Exponentials are taken in float64 and rounded to float32; divisions are done in float64
// and rounded, which is the correctly rounded float32 quotient (53 >= 2 * 24 + 2 bits); a compiler may only replace that
// by a float32 division that rounds correctly too.
#include <cmath>
#include <cstring>
#include <vector>

#include "st_internal.h"

struct st_detect_state {
  float* rows = nullptr;      // the kept rows of the last st_facenet_output_batch call
  size_t rows_cap = 0;        // rows the buffer holds
  long long total = -1;       // rows of the last call; -1: none yet
};

void st_detect_release(st_ctx* ctx) {
  if (!ctx->detect) return;
  if (ctx->detect->rows) (void)hipFree(ctx->detect->rows);
  delete ctx->detect;
  ctx->detect = nullptr;
}

namespace {

typedef unsigned long long u64;

constexpr int NMS_THREADS = 1024;
constexpr int NMS_LDS_CAP = 6144;                  // boxes a workgroup sorts in LDS: 24 B each, 144 KB of the 160 KB
constexpr size_t NMS_LDS_BYTES = (size_t)NMS_LDS_CAP * (sizeof(u64) + sizeof(float4));

// the correctly rounded float32 quotient
__device__ __forceinline__ float fo_div(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float fo_exp(float v) { return (float)exp((double)v); }

// Sort key: ascending order of the key is descending order of the score's bit pattern, then ascending index.  Scores are
// never negative, so for everything but a NaN the bit pattern orders as the value does.
__device__ __forceinline__ u64 nms_key(float score, unsigned idx) { return ((u64)(~__float_as_uint(score)) << 32) | idx; }

struct FoGeom {
  int G, gh;                 // cells of a plane, cells along yi (the fast axis)
  int nvalid;
  int valid[15];             // the valid templates, in loop order
  float T[100];              // templates file
  float net_w, net_h, fw, fh;
  double thr;
};

// facenet_output_kernel_cpu.cpp:95: the sigmoid; false when the candidate falls to the threshold (:97)
__device__ __forceinline__ bool fo_score(float c, double thr, float* score) {
  const float e = fo_exp(-c);
  const float s = (float)(1.0 / (1.0 + (double)e));
  *score = s;
  return !((double)s < thr);
}

// :99-141: the box of candidate (t, xi, yi), g = xi * gh + yi; false when it is dropped (:131-133)
__device__ __forceinline__ bool fo_box(const float* __restrict__ map, const FoGeom& k, int t, int xi, int yi, int g, float4* box) {
  const float* adj = map + (size_t)25 * k.G;
  const float dcx = adj[(size_t)(0 * 25 + t) * k.G + g], dcy = adj[(size_t)(1 * 25 + t) * k.G + g];
  const float dcw = adj[(size_t)(2 * 25 + t) * k.G + g], dch = adj[(size_t)(3 * 25 + t) * k.G + g];
  float x = (float)(xi * 8 - 1), y = (float)(yi * 8 - 1);
  const float tw = (k.T[4 * t + 2] - k.T[4 * t + 0]) + 1.0f, th = (k.T[4 * t + 3] - k.T[4 * t + 1]) + 1.0f;
  x = x + tw * dcx;
  y = y + th * dcy;
  float bw = tw * fo_exp(dcw), bh = th * fo_exp(dch);
  x = fo_div(x, k.net_w) * k.fw;
  y = fo_div(y, k.net_h) * k.fh;
  bw = fo_div(bw, k.net_w) * k.fw;
  bh = fo_div(bh, k.net_h) * k.fh;
  if (bw < 0.0f || bh < 0.0f || bw != bw || bh != bh || x != x || y != y) return false;
  const float hw = bw * 0.5f, hh = bh * 0.5f;   // a division by 2 is exact
  *box = make_float4(fo_div(x - hw, k.fw), fo_div(y - hh, k.fh), fo_div(x + hw, k.fw), fo_div(y + hh, k.fh));
  return true;
}

struct FoDecodeK {
  const float* const* maps;   // n maps
  u64* keys;                  // n * stride
  unsigned* count;            // n, zeroed
  long long stride;           // candidates of a frame
  FoGeom g;
};

// grid (ceil(G / 256), valid templates, frames)
__global__ __launch_bounds__(256) void k_fo_decode(FoDecodeK a) {
  const int g = blockIdx.x * 256 + threadIdx.x, tv = blockIdx.y, f = blockIdx.z;
  const int t = a.g.valid[tv];
  bool keep = false;
  float score = 0.f;
  if (g < a.g.G) {
    const float* __restrict__ map = st_gl(a.maps[f]);
    keep = fo_score(map[(size_t)t * a.g.G + g], a.g.thr, &score);
    if (keep) {
      float4 box;
      keep = fo_box(map, a.g, t, g / a.g.gh, g % a.g.gh, g, &box);
    }
  }
  // one atomic per wave: its survivors take consecutive slots (their order among themselves does not matter)
  const u64 mask = __ballot(keep);
  if (mask == 0) return;
  const int lane = __lane_id(), leader = __ffsll((long long)mask) - 1;
  unsigned base = 0;
  if (lane == leader) base = atomicAdd(&a.count[f], (unsigned)__popcll(mask));
  base = __shfl(base, leader);
  if (keep) {
    const unsigned slot = base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));   // < stride: a candidate appends once
    a.keys[(size_t)f * a.stride + slot] = nms_key(score, (unsigned)(tv * a.g.G + g));
  }
}

// ---- the suppression ----------------------------------------------------------------------------------
__device__ __forceinline__ float nms_min(float a, float b) { return b < a ? b : a; }   // std::min
__device__ __forceinline__ float nms_max(float a, float b) { return a < b ? b : a; }   // std::max

// the overlap of box b with the kept box c, over b's own area
__device__ __forceinline__ float nms_ov(const float4 c, const float4 b, float o) {
  const float iw = nms_max(0.0f, (nms_min(c.z, b.z) - nms_max(c.x, b.x)) + o);
  const float ih = nms_max(0.0f, (nms_min(c.w, b.w) - nms_max(c.y, b.y)) + o);
  const float num = iw * ih;
  const float den = ((b.z - b.x) + o) * ((b.w - b.y) + o);
  return fo_div(num, den);
}

struct NmsK {
  const unsigned* count;      // boxes per set
  const long long* first;     // a set's first slot in keys / boxes / kept (and, for rows, its first row)
  u64* keys;                  // facenet: the decode kernel's keys; rows: scratch
  float4* boxes;              // scratch for the sets that do not fit LDS
  int* kept;                  // out: kept indices (candidate index / row index within the set), in kept order
  int* kept_count;            // out
  const float* rows;          // rows mode: [x1, y1, x2, y2, score] per box; null in facenet mode
  const float* const* maps;   // facenet mode
  float overlap, offset;
  FoGeom g;                   // facenet mode
};

// One workgroup per set.  K[j]: before the greedy loop the sort key; in it, low word = the box's index, high word = 1 while
// the box is valid.  B[j]: the box at sorted position j.
__global__ __launch_bounds__(NMS_THREADS) void k_nms(NmsK a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int s_found;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int m = (int)a.count[f];
  const long long first = a.first[f];
  const bool in_lds = m <= NMS_LDS_CAP;
  u64* K = in_lds ? reinterpret_cast<u64*>(lds + sizeof(float4) * NMS_LDS_CAP) : a.keys + first;
  float4* B = in_lds ? reinterpret_cast<float4*>(lds) : a.boxes + first;
  const float* __restrict__ map = a.rows ? nullptr : st_gl(a.maps[f]);
  const float* __restrict__ rows = a.rows ? a.rows + 5 * first : nullptr;
  // the keys
  if (rows) {
    for (int i = tid; i < m; i += NMS_THREADS) K[i] = nms_key(rows[5 * (size_t)i + 4], (unsigned)i);
  } else if (in_lds) {
    for (int i = tid; i < m; i += NMS_THREADS) K[i] = a.keys[first + i];
  }
  __syncthreads();
  // Bitonic sort as a network whose comparators all put the smaller key at the lower index (the first step of a merge
  // mirrors, i ^ (k - 1)): slots m .. 2^p - 1 then behave as +infinity that never moves, so any m is sorted as it is.
  for (unsigned k = 2; (k >> 1) < (unsigned)m; k <<= 1) {
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      const unsigned flip = j == (k >> 1) ? k - 1 : j;
      for (unsigned i = tid; i < (unsigned)m; i += NMS_THREADS) {
        const unsigned l = i ^ flip;
        if (l > i && l < (unsigned)m) {
          const u64 x = K[i], y = K[l];
          if (y < x) { K[i] = y; K[l] = x; }
        }
      }
      __syncthreads();
    }
  }
  // the boxes, in sorted order
  for (int j = tid; j < m; j += NMS_THREADS) {
    const unsigned idx = (unsigned)K[j];
    float4 box;
    if (rows) {
      const float* r = rows + 5 * (size_t)idx;
      box = make_float4(r[0], r[1], r[2], r[3]);
    } else {
      const int tv = (int)(idx / (unsigned)a.g.G), g = (int)(idx % (unsigned)a.g.G);
      (void)fo_box(map, a.g, a.g.valid[tv], g / a.g.gh, g % a.g.gh, g, &box);   // true: the decode kernel let it through
    }
    B[j] = box;
    K[j] = (u64)idx | (1ull << 32);
  }
  if (tid == 0) s_found = 0x7fffffff;
  __syncthreads();
  int* kept = a.kept + first;
  int nk = 0, cur = 0;   // uniform across the workgroup
  while (cur < m) {
    const int i0 = cur + tid;
    if (i0 < m && (K[i0] >> 32)) atomicMin(&s_found, i0);
    __syncthreads();
    const int c = s_found;
    __syncthreads();
    if (c == 0x7fffffff) { cur += NMS_THREADS; continue; }
    // c is the first box, in visiting order, that is still valid: kept.  Boxes before it have all been visited.
    if (tid == 0) { kept[nk] = (int)(unsigned)K[c]; s_found = 0x7fffffff; }
    ++nk;
    const float4 cb = B[c];
    for (int i = c + tid; i < m; i += NMS_THREADS) {
      const u64 k = K[i];
      if ((k >> 32) && !(nms_ov(cb, B[i], a.offset) < a.overlap)) K[i] = (u64)(unsigned)k;
    }
    cur = c + 1;
    __syncthreads();
  }
  if (tid == 0) a.kept_count[f] = nk;
}

struct FoPackK {
  const float* const* maps;
  const int* kept;            // n * stride candidate indices
  const int* kept_count;
  const long long* row_first; // a frame's first row of `rows`
  float* rows;
  long long stride;
  FoGeom g;
};

// one workgroup per frame
__global__ __launch_bounds__(256) void k_fo_pack(FoPackK a) {
  const int f = blockIdx.x, nk = a.kept_count[f];
  const float* __restrict__ map = st_gl(a.maps[f]);
  for (int k = threadIdx.x; k < nk; k += 256) {
    const unsigned idx = (unsigned)a.kept[(size_t)f * a.stride + k];
    const int tv = (int)(idx / (unsigned)a.g.G), g = (int)(idx % (unsigned)a.g.G), t = a.g.valid[tv];
    float score;
    float4 box;
    (void)fo_score(map[(size_t)t * a.g.G + g], a.g.thr, &score);
    (void)fo_box(map, a.g, t, g / a.g.gh, g % a.g.gh, g, &box);
    float* r = a.rows + 5 * (size_t)(a.row_first[f] + k);
    r[0] = box.x; r[1] = box.y; r[2] = box.z; r[3] = box.w; r[4] = score;
  }
}

int launch_nms(st_ctx* ctx, const NmsK& a, int n) {
  ST_HIP(ctx, hipFuncSetAttribute((const void*)k_nms, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NMS_LDS_BYTES));
  st_timed t(ctx, ST_K_CPM2_NMS);
  hipLaunchKernelGGL(k_nms, dim3(n), dim3(NMS_THREADS), NMS_LDS_BYTES, ctx->stream, a);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}

// the kept rows' buffer holds `rows`
int rows_reserve(st_ctx* ctx, st_detect_state* s, size_t rows) {
  if (rows <= s->rows_cap) return ST_OK;
  if (s->rows) ST_HIP(ctx, hipFree(s->rows));   // the stream is synchronised where this is called
  s->rows = nullptr;
  s->rows_cap = 0;
  const size_t want = rows + rows / 4 + 256;
  const hipError_t e = hipMalloc((void**)&s->rows, want * 5 * sizeof(float));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    s->rows = nullptr;
    return st_set_error(ctx, ST_ERR_OOM, "hipMalloc(%zu) failed: %s", want * 5 * sizeof(float), hipGetErrorString(e));
  }
  s->rows_cap = want;
  return ST_OK;
}

}  // namespace

ST_EXPORT int st_facenet_output_batch(st_ctx* ctx, const float* const* maps_dev, int n, int h, int w, float scale, const float* templates,
                                      float threshold, float overlap, float offset, int32_t* counts_host) {
  ST_TRY(st_enter(ctx));
  if (!ctx->detect) ctx->detect = new st_detect_state();
  st_detect_state* s = ctx->detect;
  s->total = -1;   // a call that fails leaves nothing to fetch
  int nh = 0, nw = 0;
  if (n < 0 || !templates || st_facenet_geometry(h, w, scale, &nh, &nw) != ST_OK || !std::isfinite(threshold) || !std::isfinite(overlap) ||
      !std::isfinite(offset))
    return st_set_error(ctx, ST_ERR_INVALID, "facenet_output: bad arguments (n=%d h=%d w=%d scale=%g threshold=%g overlap=%g offset=%g)", n, h, w,
                        (double)scale, (double)threshold, (double)overlap, (double)offset);
  if (n == 0) {
    s->total = 0;
    return ST_OK;
  }
  if (!maps_dev || !counts_host) return st_set_error(ctx, ST_ERR_INVALID, "facenet_output: null argument");
  for (int i = 0; i < n; ++i)
    if (!maps_dev[i] || ((uintptr_t)maps_dev[i] & 3)) return st_set_error(ctx, ST_ERR_INVALID, "facenet_output: map %d is null or not 4-byte aligned", i);
  FoGeom g;
  const int gw = (nw + 7) / 8;   // facenet_output_kernel_cpu.cpp:44-45; the network input is a multiple of 8 already
  g.gh = (nh + 7) / 8;
  if ((long long)gw * g.gh > (1LL << 26)) return st_set_error(ctx, ST_ERR_UNSUPPORTED, "facenet_output: grid %dx%d is too large", gw, g.gh);
  g.G = gw * g.gh;
  // :66-69, :168-170
  g.nvalid = scale > 1.0f ? 8 : 15;
  for (int i = 0; i < 15; ++i) g.valid[i] = i < 8 ? 4 + i : 10 + i;
  memcpy(g.T, templates, sizeof g.T);
  g.net_w = (float)nw; g.net_h = (float)nh; g.fw = (float)w; g.fh = (float)h;
  g.thr = (double)threshold;
  const long long C = (long long)g.nvalid * g.G;   // < 2^30
  const size_t tb = st_align_up(sizeof(long long) * (size_t)n), cb = st_align_up(sizeof(int) * (size_t)n), total = (size_t)C * n;
  const float** d_maps;
  ST_TRY(st_upload_tables(ctx, n, 2 * tb + 2 * cb + st_align_up(total * sizeof(u64)) + st_align_up(total * sizeof(float4)) + st_align_up(total * sizeof(int)),
                          maps_dev, &d_maps));
  long long* d_first = (long long*)st_ws_alloc(ctx, tb);
  long long* d_rowfirst = (long long*)st_ws_alloc(ctx, tb);
  unsigned* d_count = (unsigned*)st_ws_alloc(ctx, cb);
  int* d_kept_count = (int*)st_ws_alloc(ctx, cb);
  u64* d_keys = (u64*)st_ws_alloc(ctx, total * sizeof(u64));
  float4* d_boxes = (float4*)st_ws_alloc(ctx, total * sizeof(float4));
  int* d_kept = (int*)st_ws_alloc(ctx, total * sizeof(int));
  if (!d_first || !d_rowfirst || !d_count || !d_kept_count || !d_keys || !d_boxes || !d_kept)
    return st_set_error(ctx, ST_ERR_OOM, "facenet_output: workspace exhausted");
  std::vector<long long> first(n);
  for (int i = 0; i < n; ++i) first[i] = C * i;
  ST_HIP(ctx, hipMemcpyAsync(d_first, first.data(), sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  ST_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(unsigned) * (size_t)n, ctx->stream));
  FoDecodeK d;
  d.keys = d_keys; d.stride = C; d.g = g;
  ST_TRY(st_for_launches(n, [&](int f0, int nf) -> int {
    d.maps = d_maps + f0; d.count = d_count + f0; d.keys = d_keys + (size_t)C * f0;
    st_timed t(ctx, ST_K_CPM2_NMS);
    hipLaunchKernelGGL(k_fo_decode, dim3((g.G + 255) / 256, g.nvalid, nf), dim3(256), 0, ctx->stream, d);
    ST_HIP(ctx, hipGetLastError());
    return ST_OK;
  }));
  NmsK k;
  k.count = d_count; k.first = d_first; k.keys = d_keys; k.boxes = d_boxes; k.kept = d_kept; k.kept_count = d_kept_count;
  k.rows = nullptr; k.maps = d_maps; k.overlap = overlap; k.offset = offset; k.g = g;
  ST_TRY(launch_nms(ctx, k, n));
  ST_HIP(ctx, hipMemcpyAsync(counts_host, d_kept_count, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  long long rows = 0;
  for (int i = 0; i < n; ++i) {
    first[i] = rows;
    rows += counts_host[i];
  }
  if (rows > 0) {
    ST_TRY(rows_reserve(ctx, s, (size_t)rows));
    ST_HIP(ctx, hipMemcpyAsync(d_rowfirst, first.data(), sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    FoPackK p;
    p.maps = d_maps; p.kept = d_kept; p.kept_count = d_kept_count; p.row_first = d_rowfirst; p.rows = s->rows; p.stride = C; p.g = g;
    {
      st_timed t(ctx, ST_K_CPM2_NMS);
      hipLaunchKernelGGL(k_fo_pack, dim3(n), dim3(256), 0, ctx->stream, p);
      ST_HIP(ctx, hipGetLastError());
    }
    ST_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `first` and the maps may go once the call returns
  }
  s->total = rows;
  return ST_OK;
}

ST_EXPORT int st_facenet_output_fetch(st_ctx* ctx, float* rows_host, int64_t capacity_rows) {
  ST_TRY(st_enter(ctx));
  const st_detect_state* s = ctx->detect;
  if (!s || s->total < 0) return st_set_error(ctx, ST_ERR_INVALID, "facenet_output_fetch: no st_facenet_output_batch call to fetch from");
  if (s->total == 0) return ST_OK;
  if (!rows_host || capacity_rows < s->total)
    return st_set_error(ctx, ST_ERR_INVALID, "facenet_output_fetch: %lld rows to copy, room for %lld", s->total, (long long)capacity_rows);
  ST_HIP(ctx, hipMemcpyAsync(rows_host, s->rows, sizeof(float) * 5 * (size_t)s->total, hipMemcpyDeviceToHost, ctx->stream));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ST_OK;
}

ST_EXPORT int st_bbox_nms_f32(st_ctx* ctx, const float* rows_dev, const int32_t* counts_host, int n, float overlap, float offset,
                              int32_t* kept_dev, int32_t* kept_counts_host) {
  ST_TRY(st_enter(ctx));
  if (n < 0 || !std::isfinite(overlap) || !std::isfinite(offset))
    return st_set_error(ctx, ST_ERR_INVALID, "bbox_nms: bad arguments (n=%d overlap=%g offset=%g)", n, (double)overlap, (double)offset);
  if (n == 0) return ST_OK;
  if (!counts_host || !kept_counts_host) return st_set_error(ctx, ST_ERR_INVALID, "bbox_nms: null argument");
  std::vector<long long> first(n);
  std::vector<unsigned> count(n);
  long long total = 0, spill = 0;
  for (int i = 0; i < n; ++i) {
    if (counts_host[i] < 0) return st_set_error(ctx, ST_ERR_INVALID, "bbox_nms: set %d has a negative count", i);
    first[i] = total;
    count[i] = (unsigned)counts_host[i];
    total += counts_host[i];
    if (counts_host[i] > NMS_LDS_CAP) spill = 1;
  }
  if (total > 2147483647LL) return st_set_error(ctx, ST_ERR_UNSUPPORTED, "bbox_nms: %lld rows in all", total);
  if (total > 0 && (!rows_dev || !kept_dev)) return st_set_error(ctx, ST_ERR_INVALID, "bbox_nms: null argument");
  if (total == 0) {
    for (int i = 0; i < n; ++i) kept_counts_host[i] = 0;
    return ST_OK;
  }
  const size_t tb = st_align_up(sizeof(long long) * (size_t)n), cb = st_align_up(sizeof(int) * (size_t)n);
  const size_t scratch = spill ? (size_t)total : 0;   // global keys and boxes only where a set does not fit LDS
  ST_TRY(st_ws_reserve(ctx, tb + 2 * cb + st_align_up(scratch * sizeof(u64)) + st_align_up(scratch * sizeof(float4)) + 512));
  long long* d_first = (long long*)st_ws_alloc(ctx, tb);
  unsigned* d_count = (unsigned*)st_ws_alloc(ctx, cb);
  int* d_kept_count = (int*)st_ws_alloc(ctx, cb);
  u64* d_keys = (u64*)st_ws_alloc(ctx, scratch * sizeof(u64) + 8);
  float4* d_boxes = (float4*)st_ws_alloc(ctx, scratch * sizeof(float4) + 16);
  if (!d_first || !d_count || !d_kept_count || !d_keys || !d_boxes) return st_set_error(ctx, ST_ERR_OOM, "bbox_nms: workspace exhausted");
  ST_HIP(ctx, hipMemcpyAsync(d_first, first.data(), sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  ST_HIP(ctx, hipMemcpyAsync(d_count, count.data(), sizeof(unsigned) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  NmsK k;
  memset(&k.g, 0, sizeof k.g);
  k.count = d_count; k.first = d_first; k.keys = d_keys; k.boxes = d_boxes; k.kept = kept_dev; k.kept_count = d_kept_count;
  k.rows = rows_dev; k.maps = nullptr; k.overlap = overlap; k.offset = offset;
  ST_TRY(launch_nms(ctx, k, n));
  ST_HIP(ctx, hipMemcpyAsync(kept_counts_host, d_kept_count, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `first` and `count` may go
  return ST_OK;
}
